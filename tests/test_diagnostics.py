"""The arithmetic contract of the convergence diagnostics, on the host: the numpy restatement
``tests/diagnostics_ref.py`` (the oracle of ``tests/test_gpu_diagnostics.py``) against exact
arithmetic and the bounds derived in its docstring, against independent formulations, and
against known answers; the refusals of the C ABI that need no launch."""
import math
from fractions import Fraction

import mpmath
import numpy as np
import pytest
import torch

import diagnostics_ref as DR
from binf_amd import _native, diagnostics

F = Fraction
U = F(1, 2 ** 53)


def gam(k):
    return k * U / (1 - k * U)


def datasets(n):
    """{name: [T x C x D]} with T = n (split = 1): two chains, two dimensions."""
    rs = np.random.RandomState(100 + n)
    z = rs.standard_normal((n, 2, 2))
    out = {'normal': z, 'scaled_up': z * 2.0 ** 300, 'scaled_down': z * 2.0 ** -300,
           'equal': np.full((n, 2, 2), 0.1)}
    o = z.copy()
    o[0] += 1000.0                                  # the shift K0 itself is the outlier
    out['outlier_first'] = o
    return out


N_CASES = (2, 3, 64, 257)
worst = {}


def note(name, err, bound):
    """error <= bound, exactly; keeps the worst error / bound ratio per quantity."""
    assert err <= bound, (name, float(err), float(bound))
    if bound > 0:
        worst[name] = max(worst.get(name, 0.0), float(err / bound))


@pytest.mark.parametrize('n', N_CASES)
def test_moments_against_exact_arithmetic(n):
    """s1, s2, mean, m2 within the derived bounds of exact sums over the restatement's own
    rounded d_t (standard model; none of the data sets underflows)."""
    for name, x in datasets(n).items():
        mo = DR.moments(x, 1)
        for m in range(2):
            for i in range(2):
                d = [F(float(v)) for v in mo['d'][:, m, i]]
                K0 = F(float(mo['K0'][m, i]))
                S1, S2, Sa = sum(d), sum(v * v for v in d), sum(abs(v) for v in d)
                s1, s2 = F(float(mo['s1'][m, i])), F(float(mo['s2'][m, i]))
                mean, m2 = F(float(mo['mean'][m, i])), F(float(mo['m2'][m, i]))
                note('s1', abs(s1 - S1), gam(n) * Sa)
                note('s2', abs(s2 - S2), gam(n + 1) * S2)
                note('mean', abs(mean - (K0 + S1 / n)), gam(n + 1) * Sa / n + U * abs(mean) / (1 - U))
                gn, gn1, g2 = gam(n), gam(n + 1), gam(2)
                factor = gn1 + gn * (2 + gn) + g2 * (1 + gn) ** 2 + U * ((1 + gn1) + (1 + g2) * (1 + gn) ** 2)
                note('m2', abs(m2 - (S2 - S1 * S1 / n)), factor * S2)
                assert abs(float(factor) - DR.m2_bound_factor(n)) <= 1e-12 * float(factor)
        if name == 'equal':
            assert np.all(mo['m2'] == 0.0) and np.all(mo['mean'] == 0.1)
    print('worst error / bound at n = %d: %s' % (n, {k: '%.3f' % v for k, v in sorted(worst.items())}))


@pytest.mark.parametrize('n', N_CASES)
def test_autocovariance_against_exact_arithmetic(n):
    """a_m(k) within gamma_{n+2} sum |c_i c_{i+k}| / n of the exact sum over the restatement's
    own rounded c_i; every lag for n <= 64, a spread of lags (tile edges of 16 included) above."""
    lags = list(range(n)) if n <= 64 else [0, 1, 2, 7, 15, 16, 17, 31, 32, 33, 100, n - 2, n - 1]
    for name, x in datasets(n).items():
        mo = DR.moments(x, 1)
        a = DR.autocov_chains(x, 1, mo['mean'], n - 1)
        c = DR.centred(x, 1, mo['mean'])
        for m in range(2):
            for i in range(2):
                ci = [F(float(v)) for v in c[:, m, i]]
                for k in lags:
                    exact = sum(ci[j] * ci[j + k] for j in range(n - k)) / n
                    mag = sum(abs(ci[j] * ci[j + k]) for j in range(n - k)) / n
                    note('a(k)', abs(F(float(a[k, m, i])) - exact), gam(n + 2) * mag)
    print('worst error / bound at n = %d: a(k) %.3f' % (n, worst.get('a(k)', 0.0)))


def test_split_drops_the_middle_draw_and_orders_the_chains():
    x = np.arange(7 * 3 * 2, dtype=np.float64).reshape(7, 3, 2)
    s = DR.segments(x, 2)
    assert s.shape == (3, 6, 2)
    assert np.array_equal(s[:, :3], x[:3]) and np.array_equal(s[:, 3:], x[4:])
    with pytest.raises(AssertionError):
        DR.segments(x[:3], 2)


def test_blocked_sum_is_the_stated_order():
    rs = np.random.RandomState(3)
    for M in (1, 63, 64, 65, 130, 200):
        v = rs.standard_normal(M) * 10.0 ** rs.randint(-8, 8, size=M)
        blocks = []
        for b in range(0, M, 64):
            acc = 0.0
            for q in v[b:b + 64]:
                acc = acc + float(q)
            blocks.append(acc)
        total = 0.0
        for q in blocks:
            total = total + q
        assert float(DR.blocked_sum(v[:, None])[0]) == total
    assert math.copysign(1.0, float(DR.seq_sum(np.array([[-0.0]]))[0])) == 1.0      # from +0.0


def python_tail(W, varplus, A, n, M):
    """Geyer's initial monotone sequence once more, on plain Python floats."""
    W, varplus = float(W), float(varplus)
    rho = [1.0 - (W - (float(a) * float(n)) / float(n - 1)) / varplus for a in A]
    pairs = [rho[2 * j] + rho[2 * j + 1] for j in range(len(rho) // 2)]
    kept, hit = [], False
    for j, P in enumerate(pairs):
        if P < 0.0:
            hit = True
            break
        kept.append(P if j == 0 or not (kept[-1] < P) else kept[-1])
    total = 0.0
    for P in kept:
        total = total + P
    tau = -1.0 + 2.0 * total
    ess = (float(M) * float(n)) / tau
    return ess, math.sqrt(varplus / ess), 0 if hit else 1


@pytest.mark.parametrize('phi,K', [(0.0, 64), (0.5, 64), (0.9, 64), (0.5, 7), (0.5, 8), (0.9, 1)])
def test_tail_equals_an_independent_loop_bit_for_bit(phi, K):
    x = DR.ar1(phi, 400, 8, 3)
    r = DR.diagnose(x, 2, K)
    for i in range(3):
        ess, mcse, trunc = python_tail(r['W'][i], r['varplus'][i], r['A'][:, i], r['n'], r['M'])
        assert (ess, mcse, trunc) == (float(r['ess'][i]), float(r['mcse'][i]), int(r['truncated'][i]))


def test_max_lag_zero_has_no_pair():
    r = DR.diagnose(DR.ar1(0.0, 40, 4, 2), 2, 0)
    assert np.all(r['truncated'] == 1) and np.all(r['ess'] == -float(r['M'] * r['n']))


@pytest.mark.parametrize('T,C,D', [(400, 64, 3), (130, 5, 2)])
def test_w_bn_rhat_against_numpy_formulations(T, C, D):
    """W, Bn and rhat against np.var / np.mean.  Tolerances, from the bounds of the
    restatement's docstring (gamma_k as there, every term a first-order upper bound):
      W : the mean over chains of the m2 bound, factor(n) S2 / (n - 1), for our side; numpy's
          two-pass variance is within gamma_{n+4} of itself (n adds at most on every term, a
          product, a division, the centring; its pairwise order only lowers that); the sums
          and divisions over M chains add gamma_{M+3} W on either side.
      Bn: both sides are sums of M squared deviations of the SAME means, within gamma_{M+4} Bn
          each, plus the effect of the two grand means differing by at most
          2 gamma_{M+1} max|mean|, which enters squared (times M / (M - 1)).
      rhat = sqrt(varplus / W): sqrt((1 + e_v) / (1 - e_w)) - 1 plus two roundings."""
    x = DR.ar1(0.3, T, C, D)
    r = DR.diagnose(x, 2, 1)
    n, M = r['n'], r['M']
    s = DR.segments(x, 2)
    mo = DR.moments(x, 2)
    W_np = np.mean(np.var(s, axis=0, ddof=1), axis=0)
    S2 = np.sum(mo['d'] ** 2, axis=0)
    tol_W = np.mean(DR.m2_bound_factor(n) * S2 / (n - 1), axis=0) * (1 + DR.gamma(M + 3)) \
        + DR.gamma(n + 4) * W_np + 2 * DR.gamma(M + 3) * W_np
    assert np.all(np.abs(r['W'] - W_np) <= tol_W), (np.abs(r['W'] - W_np) / tol_W).max()
    Bn_np = np.var(r['chain_mean'], axis=0, ddof=1)
    tol_B = 2 * DR.gamma(M + 4) * Bn_np + M / (M - 1.0) * (2 * DR.gamma(M + 1) * np.abs(r['chain_mean']).max(axis=0)) ** 2
    assert np.all(np.abs(r['Bn'] - Bn_np) <= tol_B), (np.abs(r['Bn'] - Bn_np) / tol_B).max()
    vp_np = (n - 1.0) / n * W_np + Bn_np
    e_w = tol_W / W_np
    e_v = (tol_W + tol_B) / vp_np + 3 * DR.U
    tol_r = (np.sqrt((1 + e_v) / (1 - e_w)) - 1 + 2 * DR.U) * np.sqrt(vp_np / W_np)
    assert np.all(np.abs(r['rhat'] - np.sqrt(vp_np / W_np)) <= tol_r)
    print('W: worst |diff| / tol %.3f; Bn: %.3f' % ((np.abs(r['W'] - W_np) / tol_W).max(),
                                                     (np.abs(r['Bn'] - Bn_np) / tol_B).max()))
    # the square root itself, against mpmath at 60 digits: correctly rounded
    mpmath.mp.dps = 60
    for i in range(D):
        q = float(r['varplus'][i] / r['W'][i])
        assert float(r['rhat'][i]) == float(mpmath.sqrt(mpmath.mpf(q)))


# ---------------------------------------------------------------------------
# known answers: AR(1), RandomState(5), 200 warm-up draws discarded, max_lag = 64
# ---------------------------------------------------------------------------
KNOWN_SHAPES = ((1000, 32, 4), (400, 64, 3))


@pytest.mark.parametrize('T,C,D', KNOWN_SHAPES)
@pytest.mark.parametrize('phi', [0.0, 0.5])
def test_known_ess_and_rhat_of_ar1(phi, T, C, D):
    """ess / (M n) within 25 % of (1 - phi) / (1 + phi), truncated == 0, rhat < 1.02."""
    r = DR.diagnose(DR.ar1(phi, T, C, D), 2, 64)
    ratio = r['ess'] / (r['M'] * r['n'])
    want = (1 - phi) / (1 + phi)
    print('phi %.1f (%d, %d, %d): ess / (M n) %s, rhat %s' % (phi, T, C, D, ratio, r['rhat']))
    assert np.all(np.abs(ratio / want - 1.0) <= 0.25)
    assert np.all(r['truncated'] == 0)
    assert np.all(r['rhat'] < 1.02)
    assert np.array_equal(r['mcse'], np.sqrt(r['varplus'] / r['ess']))


@pytest.mark.parametrize('T,C,D', KNOWN_SHAPES)
def test_slow_chain_is_reported_truncated(T, C, D):
    """phi = 0.9 keeps its pair sums positive beyond 64 lags in most dimensions: truncated says
    so exactly where the pair sums of the restatement's own rho stay non-negative."""
    r = DR.diagnose(DR.ar1(0.9, T, C, D), 2, 64)
    n, M = r['n'], r['M']
    want = []
    for i in range(D):
        rho = 1.0 - (r['W'][i] - (r['A'][:, i] * n) / (n - 1.0)) / r['varplus'][i]
        pairs = rho[0:64:2] + rho[1:65:2]
        want.append(0 if np.any(pairs < 0.0) else 1)
    assert list(r['truncated']) == want
    assert sum(want) >= 1
    trunc = r['truncated'] == 1
    assert np.all(r['ess'][trunc] / (M * n) > 0.0)


def test_known_rhat_of_shifted_chains():
    """Chains alternately shifted by 3 sigma: varplus / W -> 1 + (3/2)^2 = 3.25."""
    T, C, D = 400, 64, 3
    shift = np.where(np.arange(C) % 2 == 0, 0.0, 3.0)[None, :, None]
    r = DR.diagnose(DR.ar1(0.0, T, C, D, shift=shift), 2, 64)
    print('shifted chains: rhat', r['rhat'])
    assert np.all(np.abs(r['rhat'] - math.sqrt(3.25)) <= 0.05)


# ---------------------------------------------------------------------------
# refusals that need no launch (fake pointers, never dereferenced)
# ---------------------------------------------------------------------------
BASE = 1 << 40


def moments_rc(T=8, C=4, D=3, split=2, st=None, sc=None, si=1, draws=BASE, mean=BASE + (1 << 30),
               m2=BASE + (2 << 30)):
    sc = D if sc is None else sc
    st = C * sc if st is None else st
    return _native.lib().binf_chain_moments_f64(draws, st, sc, si, T, C, D, split, mean, m2, None)


def test_moments_refusals_without_gpu():
    E = _native.E_ARG
    assert moments_rc(T=3, split=2) == E and 'n >= 2' in _native.last_error()
    assert moments_rc(T=1, split=1) == E
    assert moments_rc(C=0) == E and moments_rc(D=0) == E
    assert moments_rc(split=3) == E and 'split' in _native.last_error()
    assert moments_rc(si=2) == E and 'inner stride' in _native.last_error()
    assert moments_rc(st=-12) == E and 'negative' in _native.last_error()
    assert moments_rc(sc=-3) == E
    assert moments_rc(sc=2) == E and 'overlapping' in _native.last_error()          # rows of 3 every 2
    assert moments_rc(st=11) == E and 'overlapping' in _native.last_error()         # draws of 12 every 11
    assert moments_rc(st=0) == E
    assert moments_rc(draws=None) == E and moments_rc(mean=None) == E
    assert moments_rc(T=1 << 40, C=1 << 30, D=1 << 20) == _native.E_UNSUPPORTED
    # chain-major draws (a transposed record) are admissible: the refusal is then the alias
    assert moments_rc(st=3, sc=8 * 3, mean=BASE + 8) == _native.E_ALIAS
    # outputs against the draws (a view's span: the last element counts) and each other
    span = (8 - 1) * 24 + (4 - 1) * 6 + 3                                             # st 24, sc 6
    assert moments_rc(st=24, sc=6, mean=BASE + 8 * (span - 1)) == _native.E_ALIAS
    assert moments_rc(st=24, sc=6, m2=BASE - 8 * 24 + 8) == _native.E_ALIAS
    assert moments_rc(m2=BASE + (1 << 30) + 8 * 23) == _native.E_ALIAS and 'm2' in _native.last_error()


def test_autocov_refusals_without_gpu():
    L = _native.lib()
    T, C, D = 10, 4, 3
    need = L.binf_chain_autocov_workspace_bytes(2 * C, D, 4)
    assert need == 1 * 5 * D * 8
    assert L.binf_chain_autocov_workspace_bytes(65, 7, 9) == 2 * 10 * 7 * 8
    mean, ws = BASE + (1 << 30), BASE + (2 << 30)

    def rc(K=4, split=2, mean_=mean, ws_=ws, bytes_=need, T_=T):
        return L.binf_chain_autocov_f64(BASE, C * D, D, 1, T_, C, D, split, mean_, K, ws_, bytes_, None)
    assert rc(K=5) == _native.E_ARG and 'max_lag' in _native.last_error()           # n = 5: K <= 4
    assert rc(K=-1) == _native.E_ARG
    assert rc(bytes_=need - 8) == _native.E_ARG and 'workspace' in _native.last_error()
    assert rc(ws_=None) == _native.E_ARG
    assert rc(mean_=None) == _native.E_ARG
    assert rc(T_=3) == _native.E_ARG
    assert rc(ws_=BASE + 8 * (T * C * D - 1)) == _native.E_ALIAS
    assert rc(ws_=mean + 8) == _native.E_ALIAS


def test_summary_refusals_without_gpu():
    L = _native.lib()
    M, D, n, K = 6, 3, 5, 4
    need = L.binf_diag_summary_workspace_bytes(M, D)
    assert need == 3 * 1 * D * 8 and L.binf_diag_summary_workspace_bytes(130, 2) == 3 * 3 * 2 * 8
    p = [BASE + (i << 24) for i in range(13)]

    def rc(M_=M, n_=n, K_=K, **over):
        a = dict(mean=p[0], m2=p[1], autocov=p[2], post_mean=p[3], varplus=p[4], sd=p[5], W=p[6],
                 rhat=p[7], ess=p[8], mcse=p[9], truncated=p[10], ws=p[11], bytes=need)
        a.update(over)
        return L.binf_diag_summary_f64(a['mean'], a['m2'], a['autocov'], n_, M_, D, K_, a['post_mean'],
                                       a['varplus'], a['sd'], a['W'], a['rhat'], a['ess'], a['mcse'],
                                       a['truncated'], a['ws'], a['bytes'], None)
    assert rc(M_=1) == _native.E_ARG and 'M >= 2' in _native.last_error()
    assert rc(n_=1) == _native.E_ARG
    assert rc(K_=5) == _native.E_ARG and rc(K_=-1) == _native.E_ARG
    assert rc(ess=None) == _native.E_ARG and rc(rhat=None) == _native.E_ARG
    assert rc(ws=None) == _native.E_ARG and rc(bytes=need - 1) == _native.E_ARG
    assert rc(rhat=p[0] + 8 * (M * D - 1)) == _native.E_ALIAS                        # output in an input
    assert rc(truncated=p[2] + 8 * (K + 1) * D - 1) == _native.E_ALIAS               # the last byte of autocov
    assert rc(ess=p[9] + 8) == _native.E_ALIAS                                       # output in an output
    assert rc(ws=p[6] + 16) == _native.E_ALIAS                                       # workspace in an output
    assert rc(truncated=p[3] + 8 * D - 1) == _native.E_ALIAS
    # R^ only: the ESS outputs are neither required nor compared
    assert rc(autocov=None, ess=None, mcse=None, truncated=None, K_=99, rhat=p[0] + 8) == _native.E_ALIAS


def test_python_layer_refuses_host_and_misshapen_draws():
    x = torch.zeros((8, 4, 3), dtype=torch.float64)
    for fn in (diagnostics.summary, diagnostics.split_rhat, diagnostics.effective_sample_size,
               diagnostics.chain_moments):
        with pytest.raises(ValueError, match='GPU memory'):
            fn(x)
    with pytest.raises(TypeError):
        diagnostics.summary(np.zeros((8, 4, 3)))
    from binf_amd.dist import SampleStore
    store = SampleStore(8, 4, 3, device='cpu')
    store.extend(x)
    with pytest.raises(ValueError, match='GPU memory'):
        store.summary(columns=slice(0, 2))
    assert diagnostics.default_max_lag(5) == 4 and diagnostics.default_max_lag(1000) == 64


def test_summary_prints_as_a_table():
    D = 3
    s = diagnostics.Summary(torch.tensor([0.1, -2.0, 3.0], dtype=torch.float64), torch.ones(D, dtype=torch.float64),
                            torch.tensor([1.001, 1.2, float('nan')], dtype=torch.float64),
                            torch.tensor([900.0, 12.5, 4.0], dtype=torch.float64),
                            torch.full((D,), 0.03, dtype=torch.float64), torch.tensor([0, 1, 0], dtype=torch.uint8))
    text = str(s)
    lines = text.splitlines()
    assert lines[0].split() == ['dim', 'mean', 'sd', 'rhat', 'ess', 'mcse']
    assert len(lines) == 1 + D + 1 and '12.5+' in lines[2] and 'upper bound' in lines[-1]
    assert '1.0010' in lines[1] and 'nan' in lines[3]
