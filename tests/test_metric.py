"""CPU tests of the diagonal-metric layer: the host restatement ``tests/metric_ref.py`` held
on its own to known answers, to the diagnostics' restatement, to exact arithmetic
(``fractions.Fraction``) inside a derived bound and to ``np.var``; the refusals of the five
entry points (host checks, fake pointers, nothing launched); and the thresholds of the
statistical GPU test (``tests/test_gpu_metric_warmup.py``) on the restatement over ten seeds.
The device is compared with the same restatement bit for bit in ``tests/test_gpu_metric.py``."""
from fractions import Fraction as Fr

import numpy as np
import pytest

import diagnostics_ref as DR
import metric_ref as MR
from binf_amd import _native
from binf_amd.samplers.warmup import window_schedule

U = Fr(1, 2 ** 53)


def gam(k):
    return k * U / (1 - k * U)


# ---------------------------------------------------------------------------
# window schedule
# ---------------------------------------------------------------------------
SCHEDULES = [
    ((1000, 75, 50, 25), [(75, 100), (100, 150), (150, 250), (250, 450), (450, 950)]),
    ((300, 20, 40, 20), [(20, 40), (40, 80), (80, 260)]),
    # n < 75 + 50 + 25: init = floor(0.15 n), term = floor(0.1 n), one window of the rest
    ((20, 75, 50, 25), [(3, 18)]),
    ((149, 75, 50, 25), [(22, 135)]),
    # n = 150: the defaults fit exactly; the doubled window [100, 150) would overrun n - term = 100
    ((150, 75, 50, 25), [(75, 100)]),
]


@pytest.mark.parametrize('args,want', SCHEDULES)
def test_window_schedule_known_answers(args, want):
    assert window_schedule(*args) == want
    assert MR.window_schedule(*args) == want


def test_window_schedule_equals_the_walked_restatement():
    """The package's closed loop over windows against the restatement's walk over transitions;
    windows follow one another without gaps, each but the last is twice its predecessor (the
    last is stretched, or cut, to end at n - term)."""
    for n in list(range(0, 260)) + [500, 1000, 1337, 5000]:
        for init, term, base in ((75, 50, 25), (20, 40, 20), (0, 0, 1), (5, 0, 3), (10, 10, 10)):
            w = window_schedule(n, init, term, base)
            assert w == MR.window_schedule(n, init, term, base), (n, init, term, base)
            for j, ((a, b), (c, d)) in enumerate(zip(w, w[1:])):
                assert b == c and (d - c == 2 * (b - a) or j == len(w) - 2)
            if w:
                assert w[-1][1] <= n and w[0][0] >= 0


# ---------------------------------------------------------------------------
# accumulate == chain_moments
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('n', [2, 5, 33])
def test_streamed_moments_equal_chain_moments(n):
    rs = np.random.RandomState(n)
    x = 1e3 + rs.standard_normal((n, 5, 7)) * rs.uniform(0.1, 50.0, size=(1, 5, 7))
    x[n // 2, 1, 3] = np.inf
    x[0, 2, 4] = np.nan
    m = MR.accumulate(x)
    want = DR.moments(x, 1)
    for got, key in ((m.k0, 'K0'), (m.s1, 's1'), (m.s2, 's2'), (m.mean(), 'mean'), (m.m2(), 'm2')):
        assert np.array_equal(np.isnan(got), np.isnan(want[key]))
        assert np.where(np.isnan(got), 0.0, got).tobytes() == np.where(np.isnan(want[key]), 0.0, want[key]).tobytes(), key


def test_one_draw():
    x = np.random.RandomState(0).standard_normal((1, 3, 4))
    m = MR.accumulate(x)
    assert np.array_equal(m.mean(), x[0]) and not m.m2().any()


# ---------------------------------------------------------------------------
# pool against exact arithmetic
# ---------------------------------------------------------------------------
def exact_pool(x, k0, n, G, regularise):
    """Exact arithmetic (Fraction) on the restatement's own rounded d = fl(x - k0), and the
    bound of :func:`test_pool_against_exact_arithmetic` beside it.  The exact values are
    Fractions; the bound is evaluated in floats from them (a sum of positive terms: no
    cancellation) and widened by 1e-9 for its own roundings.  Returns per (g, i):
    (var', bound on |scale^2 - var'|, E_W, sum over chains of m2 + n (mean - k0)^2)."""
    nT, C, D = x.shape
    assert nT == n
    Cg = C // G
    N = n * Cg
    u = float(U)
    k = min(Cg, DR.BLOCK) + (Cg + DR.BLOCK - 1) // DR.BLOCK          # adds on any term of a blocked sum
    gn1, gk = float(gam(n + 1)), float(gam(k))
    F = DR.m2_bound_factor(n)
    d = x - k0                                                       # what the restatement accumulates
    out = {}
    for g in range(G):
        for i in range(D):
            M2, Mean, S2s, e, spread = [], [], [], [], Fr(0)
            for c in range(g, C, G):
                dd = [Fr(float(v)) for v in d[:, c, i]]
                S1, S2, Sa = sum(dd), sum(v * v for v in dd), sum(abs(v) for v in dd)
                mean = Fr(float(k0[c, i])) + S1 / n
                M2.append(S2 - S1 * S1 / n)
                Mean.append(mean)
                S2s.append(S2)
                e.append(gn1 * float(Sa) / n * (1 + u) + u * abs(float(mean)))
                spread += M2[-1] + n * (mean - Fr(float(k0[c, i]))) ** 2
            assert spread == sum(S2s)                                # S2 = m2 + n (mean - k0)^2, exactly
            Wx = sum(M2)
            E_W = (F + gk * (1 + F)) * float(spread)
            Mbar = sum(Mean) / Cg
            e_bar = (sum(e) + gk * sum(abs(float(m)) + ec for m, ec in zip(Mean, e))) / Cg * (1 + u) + u * abs(float(Mbar))
            Bx, beta_sum, b_abs = Fr(0), 0.0, 0.0
            for m, ec in zip(Mean, e):
                Dl = m - Mbar
                Bx += Dl * Dl
                Dl = abs(float(Dl))
                eta = (ec + e_bar) * (1 + u) + u * Dl
                beta = eta * (2 * Dl + eta) * (1 + u) + u * Dl * Dl
                beta_sum += beta
                b_abs += Dl * Dl + beta
            E_B = beta_sum + gk * b_abs
            Y = Wx + n * Bx
            E_s = E_W + n * E_B * (1 + u) + u * n * float(Bx)
            if N == 1:
                out[g, i] = None
                continue
            Var = Y / (N - 1)
            E_var = (E_s * (1 + u) + u * abs(float(Y))) / (N - 1) * (1 + u) + u * abs(float(Var))
            if regularise:
                A, B5, c3 = Fr(N, N + 5), Fr(5, N + 5), Fr(1e-3)
                t1 = float(A) * (E_var * (1 + u) ** 2 + (2 * u + u * u) * abs(float(Var)))
                t2 = float(c3 * B5) * (2 * u + u * u)
                V = A * Var + c3 * B5
                E_V = (t1 + t2) * (1 + u) + u * abs(float(V))
            else:
                V, E_V = Var, E_var
            # scale = sqrt(v)(1 + theta): scale^2 = v (1 + theta)^2
            bound = (E_V * (1 + u) ** 2 + (2 * u + u * u) * abs(float(V))) * (1.0 + 1e-9)
            out[g, i] = (V, Fr(bound), Fr(E_W), spread)
    return out


POOL_CASES = [(1, 1, 2), (2, 1, 2), (2, 3, 1), (63, 1, 50), (64, 3, 2), (65, 1, 50), (130, 1, 50), (130, 3, 2), (7, 2, 33)]


@pytest.mark.parametrize('Cg,G,n', POOL_CASES)
@pytest.mark.parametrize('shift', [0.0, 30.0])
@pytest.mark.parametrize('regularise', [False, True])
def test_pool_against_exact_arithmetic(Cg, G, n, shift, regularise):
    """|scale^2 - var'| <= bound, var' in exact arithmetic on the restatement's own rounded
    d_t = fl(x_t - k0) (as tests/test_diagnostics.py holds the moments), with the standard model
    fl(a op b) = (a op b)(1 + delta), |delta| <= u = 2^-53, gamma_j = j u / (1 - j u):

    per chain (diagnostics_ref): |m2_c - M2_c| <= F(n) S2_c, S2_c = sum d_t^2 (F ~ (3n + 5) u), and
        |mean_c - Mean_c| <= gamma_{n+1} Sa_c / n (1 + u) + u |Mean_c| = e_c.
    blocked sum of Cg terms: a term meets at most k = min(Cg, 64) + ceil(Cg / 64) adds, so
        |W - sum M2_c| <= sum [F + gamma_k (1 + F)] S2_c = E_W;
    S2_c = M2_c + n (Mean_c - k0_c)^2 EXACTLY, so E_W is proportional to
    N (within-chain variance + (mean - k0)^2): a first draw z standard deviations out costs a
    factor 1 + z^2 (asserted: ``shift`` puts the first draw 30 sd out).
        |mbar - Mbar| <= [sum e_c + gamma_k sum (|Mean_c| + e_c)] / Cg (1 + u) + u |Mbar| = e_bar
        delta_c = fl(mean_c - mbar): |delta_c - Delta_c| <= (e_c + e_bar)(1 + u) + u |Delta_c| = eta_c
        |fl(delta_c^2) - Delta_c^2| <= eta_c (2 |Delta_c| + eta_c)(1 + u) + u Delta_c^2 = beta_c
        |B - sum Delta_c^2| <= sum beta_c + gamma_k sum (Delta_c^2 + beta_c) = E_B
        s = fl(W + fl(n B)): |s - Y| <= [E_W + n E_B (1 + u) + u n B*](1 + u) + u |Y|,  Y = W* + n B*
        var = fl(s / (N - 1)) (N - 1 exact): E_var = that / (N - 1) (1 + u) + u |Var|
        var' = fl(fl(fl(N / (N + 5)) var) + fl(1e-3 fl(5 / (N + 5)))): two roundings on each
        product, one on the sum (1e-3 is the double nearest to it, in the exact value too)
        scale = sqrt(var')(1 + theta), so scale^2 = var' (1 + theta)^2.
    The worst error / bound over these cases is printed (DESIGN quotes it)."""
    C, D = Cg * G, 3
    rs = np.random.RandomState(1000 * Cg + 10 * G + n)
    sd = np.array([0.5, 3.0, 40.0])
    x = 1e4 + rs.standard_normal((n, C, D)) * sd + 2.0 * sd * rs.standard_normal((1, C, D))
    x[0] += shift * sd                                   # the first draw (K0) far from the chain's mean
    m = MR.accumulate(x)
    prev = np.full((G, D), 7.0)
    got = MR.pool(m.k0, m.s1, m.s2, n, G, regularise, prev)
    ex = exact_pool(x, m.k0, n, G, regularise)
    worst = 0.0
    for (g, i), v in ex.items():
        if v is None:
            assert got[g, i] == 7.0
            continue
        V, bound, E_W, spread = v
        err = abs(Fr(float(got[g, i])) ** 2 - V)
        assert err <= bound, (g, i, float(err), float(bound))
        worst = max(worst, float(err / bound))
        # the shifted-data part of the bound: proportional to sum_c [m2_c + n (mean_c - k0_c)^2]
        assert spread == 0 or n * U < E_W / spread < (3 * n + 80) * U      # n = 1: every d is 0
        assert abs(float(got[g, i]) / float(V) ** 0.5 - 1.0) < 1e-9 * (1.0 + shift * shift)
    print('pool: worst error / bound %.3f (Cg=%d G=%d n=%d shift=%g reg=%d)' % (worst, Cg, G, n, shift, regularise))


def test_bound_grows_with_the_first_draws_offset():
    """The same draws with K0 30 sd out: the exact variance moves little, the bound's
    shifted-data part E_W grows by about 1 + z^2 / (1 + 1/n) -- and the error stays inside."""
    n, Cg = 50, 8
    rs = np.random.RandomState(3)
    x = rs.standard_normal((n, Cg, 1))
    parts = []
    for z in (0.0, 30.0):
        y = x.copy()
        y[0] = z
        m = MR.accumulate(y)
        parts.append(exact_pool(y, m.k0, n, 1, False)[0, 0])
    (_, _, ew0, s0), (_, _, ew30, s30) = parts
    assert 200.0 < float(ew30 / ew0) < 2000.0 and abs(float(ew30 / ew0) / float(s30 / s0) - 1.0) < 1e-12


@pytest.mark.parametrize('Cg,G,n', [(2, 1, 2), (65, 1, 50), (7, 3, 33), (130, 1, 50)])
def test_pool_against_numpy_var(Cg, G, n):
    """The restated pool (no shrinkage) against np.var(ddof=1) of the pooled draws.  The draws
    are multiples of 2^-16 below 2^10, so every d = x - k0 is exact and the exact arithmetic
    of the test above IS the variance of the draws; np.var's own error is added: its mean is
    off by at most gamma_N Xmax, which moves sum (x - mean)^2 by N (gamma_N Xmax)^2, and every
    term of that sum meets a subtraction, a product, at most N adds and the division:
    gamma_{N+4}."""
    C, D = Cg * G, 3
    rs = np.random.RandomState(Cg + n)
    x = np.round((100.0 + rs.standard_normal((n, C, D)) * np.array([0.5, 3.0, 40.0])) * 65536.0) / 65536.0
    m = MR.accumulate(x)
    assert np.array_equal(m.k0 + (x - m.k0), x)
    got = MR.pool(m.k0, m.s1, m.s2, n, G, False, np.ones((G, D)))
    ex = exact_pool(x, m.k0, n, G, False)
    N = n * Cg
    for g in range(G):
        for i in range(D):
            V, bound, _, _ = ex[g, i]
            pooled = np.ascontiguousarray(x[:, g::G, i]).reshape(-1)
            fr = [Fr(float(v)) for v in pooled]
            centre = sum(fr) / N
            assert V == sum((v - centre) ** 2 for v in fr) / (N - 1)
            xmax = Fr(float(np.max(np.abs(pooled))))
            slack = N * (gam(N) * xmax) ** 2 / (N - 1)
            np_bound = gam(N + 4) * (V + slack) + slack
            npv = Fr(float(np.var(pooled, ddof=1)))
            assert abs(Fr(float(got[g, i])) ** 2 - npv) <= bound + np_bound


def test_pool_keeps_the_scale_where_the_variance_is_no_number():
    n, C, D = 4, 6, 5
    x = np.random.RandomState(1).standard_normal((n, C, D))
    x[2, 3, 1] = np.nan                  # group 3 % 3 = 0, dimension 1
    x[1, 4, 2] = np.inf                  # group 1, dimension 2
    x[:, 2::3, 4] = 2.5                  # group 2, dimension 4: constant
    m = MR.accumulate(x)
    prev = np.arange(15, dtype=np.float64).reshape(3, 5) + 2.0
    for reg in (False, True):
        got = MR.pool(m.k0, m.s1, m.s2, n, 3, reg, prev)
        kept = got == prev
        want = np.zeros((3, 5), dtype=bool)
        want[0, 1] = want[1, 2] = True
        want[2, 4] = not reg             # the shrinkage lifts a zero variance to 1e-3 * 5 / (N + 5)
        assert np.array_equal(kept, want)
    one = MR.accumulate(x[:1, :1])
    assert np.array_equal(MR.pool(one.k0, one.s1, one.s2, 1, 1, True, prev[:1]), prev[:1])   # 0 / 0


@pytest.mark.parametrize('G', [1, 3])
def test_pooling_two_shards_equals_pooling_the_batch(G):
    """A sharded run gathers (k0, s1, s2) and pools all chains in global order: the moments
    are per chain, so the concatenated shards ARE the batch (shards of whole groups)."""
    n, C, D = 9, 12 * G, 4
    x = np.random.RandomState(G).standard_normal((n, C, D)) * 3.0 + 1.0
    cut = 5 * G
    a, b, whole = MR.accumulate(x[:, :cut]), MR.accumulate(x[:, cut:]), MR.accumulate(x)
    cat = [np.concatenate([getattr(a, k), getattr(b, k)]) for k in ('k0', 's1', 's2')]
    prev = np.ones((G, D))
    assert MR.pool(cat[0], cat[1], cat[2], n, G, True, prev).tobytes() == \
        MR.pool(whole.k0, whole.s1, whole.s2, n, G, True, prev).tobytes()


# ---------------------------------------------------------------------------
# the scaled updates
# ---------------------------------------------------------------------------
def test_unit_scale_is_the_unscaled_update():
    rs = np.random.RandomState(0)
    C, D = 6, 9
    q, p, g = rs.standard_normal((3, C, D))
    dtc = rs.uniform(0.01, 0.3, size=C)
    one = np.ones((3, D))
    for fma in (False, True):
        for dt, d in ((None, 0.07), (dtc, 0.0)):
            step = (dtc if dt is not None else np.full(C, d))[:, None]
            kq, kp = MR.kick_drift(q, p, g, one, d, dt, fma)
            if fma:
                want_p = MR.c_oracle.fma(-step, g, p)
                want_q = MR.c_oracle.fma(want_p, step, q)
            else:
                want_p = p - step * g
                want_q = q + want_p * step
            assert kp.tobytes() == want_p.tobytes() and kq.tobytes() == want_q.tobytes()
            hp = MR.kick(p, g, one, d, dt, True, fma)
            assert hp.tobytes() == (MR.c_oracle.fma(-(0.5 * step), g, p) if fma else p - (0.5 * step) * g).tobytes()


def test_restated_leapfrog_is_reversible_and_whitened():
    """With scale = sigma the whitened integrator on N(0, diag sigma^2) is the identity-mass
    integrator on N(0, I) in z = x / sigma, to rounding."""
    rs = np.random.RandomState(2)
    C, sigma = 5, MR.SIGMA8
    t = MR.DiagGaussTarget(sigma)
    q0, p0 = sigma * rs.standard_normal((C, 8)), rs.standard_normal((C, 8))
    q, p = MR.leapfrog(q0.copy(), p0.copy(), t.gradient, sigma[None], 0.3, None, 7)
    zq, zp = MR.leapfrog(q0 / sigma, p0.copy(), lambda z: z, np.ones((1, 8)), 0.3, None, 7)
    assert np.allclose(q / sigma, zq, rtol=0, atol=1e-13) and np.allclose(p, zp, rtol=0, atol=1e-13)
    qb, pb = MR.leapfrog(q.copy(), -p, t.gradient, sigma[None], 0.3, None, 7)
    assert np.allclose(qb / sigma, q0 / sigma, rtol=0, atol=1e-13) and np.allclose(-pb, p0, rtol=0, atol=1e-13)


# ---------------------------------------------------------------------------
# refusals: host checks, fake pointers, nothing is launched or dereferenced
# ---------------------------------------------------------------------------
def test_refusals_without_gpu():
    L = _native.lib()
    q, p, g, s, dtc = [(i + 1) << 40 for i in range(5)]
    C, D = 6, 8
    EX = _native.MODE_EXACT
    kick = lambda **k: L.binf_leapfrog_kick_scaled_f64(k.get('p', p), g, k.get('s', s), k.get('G', 1), 0.1, None, 0,
                                                       k.get('C', C), k.get('D', D), k.get('mode', EX), None)
    drift = lambda **k: L.binf_leapfrog_drift_scaled_f64(k.get('q', q), p, k.get('s', s), k.get('G', 1), 0.1, None,
                                                         k.get('C', C), k.get('D', D), k.get('mode', EX), None)
    both = lambda **k: L.binf_leapfrog_kick_drift_scaled_f64(k.get('q', q), p, g, k.get('s', s), k.get('G', 1), 0.1,
                                                             None, k.get('C', C), k.get('D', D), k.get('mode', EX), None)
    for f in (kick, drift, both):
        assert f(G=4) == _native.E_ARG and 'multiple of G' in _native.last_error()      # C % G != 0
        assert f(G=0) == _native.E_ARG and 'G >= 1' in _native.last_error()
        assert f(G=-2) == _native.E_ARG
        assert f(C=-1) == _native.E_ARG and f(D=-1) == _native.E_ARG
        assert f(mode=2) == _native.E_ARG and 'mode' in _native.last_error()
        assert f(mode=_native.MODE_LANE_PER_CHAIN) == _native.E_ARG
        assert f(s=None) == _native.E_ARG
        assert f(C=0) == 0 and f(D=0) == 0                  # empty: no launch, no error
    # C % G != 0 again, the same call through the dense launcher of the same check
    assert kick(G=4) == L.binf_leapfrog_kick_dense_f64(p, g, s, 4, 0.1, None, 0, C, D, EX, None) == _native.E_ARG
    assert 'multiple of G' in _native.last_error()
    # the scale overlapping what is written: p (kick, kick_drift), q (drift, kick_drift)
    last = C * D * 8 - 8
    for f, key, base in ((kick, 'p', p), (drift, 'q', q), (both, 'q', q)):
        assert f(s=base) == _native.E_ALIAS
        assert f(s=base + last) == _native.E_ALIAS
        assert f(s=base - D * 8 + 8) == _native.E_ALIAS     # its last element on the buffer's first
        assert f(s=base + last, G=3) == _native.E_ALIAS
    assert both(s=p + 16) == _native.E_ALIAS
    assert both(q=p + 8) == _native.E_ALIAS                 # q overlapping p
    assert L.binf_leapfrog_kick_scaled_f64(p, p + 8, s, 1, 0.1, None, 0, C, D, EX, None) == _native.E_ALIAS
    assert L.binf_leapfrog_kick_scaled_f64(p, g, s, 1, 0.1, p + 8, 0, C, D, EX, None) == _native.E_ALIAS

    x, k0, s1, s2, sc = [(i + 1) << 40 for i in range(5)]
    acc = lambda **k: L.binf_metric_accumulate_f64(k.get('x', x), k.get('k0', k0), s1, k.get('s2', s2), 1,
                                                   k.get('C', C), k.get('D', D), None)
    assert acc(C=-1) == _native.E_ARG and acc(D=-3) == _native.E_ARG and acc(x=None) == _native.E_ARG
    assert acc(C=0) == 0
    assert acc(k0=x + 8) == _native.E_ALIAS and acc(s2=s1 + last) == _native.E_ALIAS and acc(x=s1) == _native.E_ALIAS
    pool = lambda **k: L.binf_metric_pool_f64(k0, s1, s2, k.get('n', 5), k.get('C', C), k.get('D', D), k.get('G', 1),
                                              1, k.get('sc', sc), None)
    assert pool(G=4) == _native.E_ARG and 'multiple of G' in _native.last_error()
    assert pool(G=0) == _native.E_ARG and pool(n=0) == _native.E_ARG and pool(C=-1) == _native.E_ARG
    assert pool(D=-1) == _native.E_ARG and pool(sc=None) == _native.E_ARG
    assert pool(C=0) == 0
    assert pool(sc=s2 + last) == _native.E_ALIAS and pool(sc=k0 - 8, G=2) == _native.E_ALIAS
    assert pool(n=1 << 52) == _native.E_UNSUPPORTED
    with pytest.raises(ValueError):
        _native.check(pool(G=4), 'binf_metric_pool_f64')


def test_sampler_surface_without_gpu():
    """The keyword and the attributes exist; a host tensor is refused where the kernels would
    read it, shapes before that."""
    import torch
    from binf_amd.pdf import IsotropicGaussian
    from binf_amd.samplers.hmc import HMCSampler
    state = torch.zeros(6, 4, dtype=torch.float64)
    s = HMCSampler(IsotropicGaussian(), state, 0.1, 3, variable_name='x')
    assert s.metric_scale is None and s.inverse_mass is None and 'metric_scale' not in s.state_dict()
    s.set_metric(torch.full((4,), 2.0, dtype=torch.float64))
    assert tuple(s.metric_scale.shape) == (1, 4) and float(s.inverse_mass[0, 0]) == 4.0
    assert s._fused_spec('x', 4, 6) is None
    addr = s.metric_scale.data_ptr()
    s.set_metric(torch.full((1, 4), 3.0, dtype=torch.float64))
    assert s.metric_scale.data_ptr() == addr and float(s.metric_scale[0, 1]) == 3.0
    assert torch.equal(s.state_dict()['metric_scale'], s.metric_scale)
    s2 = HMCSampler(IsotropicGaussian(), state, 0.1, 3, variable_name='x', metric=torch.ones(3, 4, dtype=torch.float64))
    assert s2.metric_scale.shape[0] == 3
    s2.load_state_dict({k: v for k, v in s2.state_dict().items() if k != 'metric_scale'})     # a dict without the key
    for bad in (torch.ones(4, 4, dtype=torch.float64), torch.ones(5, dtype=torch.float64),
                torch.ones(4, dtype=torch.float32)):
        with pytest.raises(ValueError):
            s.set_metric(bad)
    s.set_metric(None)
    assert s.metric_scale is None and s._fused_spec('x', 4, 6) is not None


# ---------------------------------------------------------------------------
# the statistical experiment, on the restatement
# ---------------------------------------------------------------------------
def test_thresholds_of_the_warmup_experiment_hold_for_the_restatement():
    """8-dimensional Gaussian, sigma 1 ... 100, 16 chains from 3 sigma z, nsteps 5, 300 adapting
    transitions, 200 kept -- the thresholds tests/test_gpu_metric_warmup.py asserts on the
    device, over ten seeds of the restatement."""
    for seed in range(10):
        rhat_m, ratio, _ = MR.experiment(seed, True)
        rhat_0, _, _ = MR.experiment(seed, False)
        print('seed %d: max split-R^ %.4f with the metric, %.3f without; scale / sigma %.3f ... %.3f'
              % (seed, rhat_m, rhat_0, ratio.min(), ratio.max()))
        assert 0.7 <= ratio.min() and ratio.max() <= 1.4
        assert rhat_m < 1.2
        assert rhat_0 > 2.0
