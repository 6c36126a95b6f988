"""The dense-metric layer without a GPU: the host restatement ``tests/dense_metric_ref.py`` is
held to exact rational arithmetic inside derived bounds, the window bookkeeping to one pass over
the stacked record, the windowed covariance warm-up to the statistical experiment it was built
for, and the C ABI to its refusals (host checks: nothing is launched or dereferenced).

u = 2^-53, gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms,
2nd ed., section 3.1).  A dot product of D terms accumulated in any order has
|computed - exact| <= gamma_D sum |L||g| (ibid. (3.5)); a Cholesky factor computed in any order
of the inner sums has |L L^T - A| <= gamma_{D+1} |L||L^T| (ibid. theorem 10.3)."""
from fractions import Fraction

import numpy as np
import pytest

import dense_metric_ref as DM
import metric_ref as MR
from binf_amd import _native

U = 2.0 ** -53
NAMES = ['binf_leapfrog_kick_dense_f64', 'binf_leapfrog_drift_dense_f64', 'binf_leapfrog_kick_drift_dense_f64',
         'binf_metric_comoments_f64', 'binf_metric_factor_f64']


def gamma(k):
    return Fraction(k) * Fraction(U) / (1 - Fraction(k) * Fraction(U))


def frac(a):
    return np.vectorize(Fraction, otypes=[object])(np.asarray(a, dtype=np.float64))


def test_signatures_hold_the_five_entry_points():
    raw = _native.lib()
    for n in NAMES:
        assert n in _native.SIGNATURES and hasattr(raw, n), n
    assert _native.ABI_VERSION == 7 and raw.binf_abi_version() == 7


# ---------------------------------------------------------------------------
# the restatement against exact arithmetic
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('fma', [False, True])
@pytest.mark.parametrize('D', [1, 2, 7, 17])
def test_matvecs_inside_the_dot_product_bound(D, fma):
    rs = np.random.RandomState(D)
    C, G = 4, 2
    chol = np.tril(rs.standard_normal((G, D, D)) * rs.uniform(0.1, 10.0, size=(G, D, 1)))
    chol[:, np.triu(np.ones((D, D), dtype=bool), 1)] = np.nan            # never read
    g = rs.standard_normal((C, D)) * 3.0
    t, v = DM.lt_matvec(chol, g, fma), DM.l_matvec(chol, g, fma)
    assert np.isfinite(t).all() and np.isfinite(v).all()
    for c in range(C):
        L = frac(np.tril(np.nan_to_num(chol[c % G])))
        x = frac(g[c])
        for want, got, A in ((L.T.dot(x), t[c], L.T), (L.dot(x), v[c], L)):
            bound = gamma(D) * np.abs(A).dot(np.abs(x))
            for i in range(D):
                assert abs(Fraction(got[i]) - want[i]) <= bound[i], (c, i)


def test_matvec_order_is_the_stated_chain():
    """Scalar loops written straight from the header against the vectorised restatement."""
    rs = np.random.RandomState(3)
    D = 6
    L, g = np.tril(rs.standard_normal((D, D))), rs.standard_normal((1, D))
    t, v = np.empty(D), np.empty(D)
    for i in range(D):
        a = L[i, i] * g[0, i]
        for j in range(i + 1, D):
            a = a + L[j, i] * g[0, j]
        t[i] = a
        b = L[i, 0] * g[0, 0]
        for j in range(1, i + 1):
            b = b + L[i, j] * g[0, j]
        v[i] = b
    assert DM.lt_matvec(L, g)[0].tobytes() == t.tobytes() and DM.l_matvec(L, g)[0].tobytes() == v.tobytes()


def test_identity_factor_gives_the_unscaled_updates_and_diagonal_differs():
    rs = np.random.RandomState(4)
    C, D = 5, 9
    q, p, g = rs.standard_normal((3, C, D))
    one, eye = np.ones((1, D)), np.eye(D)
    for fma in (False, True):
        assert DM.kick(p, g, eye, 0.173, None, True, fma).tobytes() == MR.kick(p, g, one, 0.173, None, True, fma).tobytes()
        assert DM.drift(q, p, eye, 0.173, None, fma).tobytes() == MR.drift(q, p, one, 0.173, None, fma).tobytes()
    # L = diag(s): d * (s * g) here, (d * s) * g there -- close, not equal
    s = rs.uniform(0.3, 30.0, size=(1, D))
    a, b = DM.kick(p, g, np.diag(s[0]), 0.173), MR.kick(p, g, s, 0.173)
    assert a.tobytes() != b.tobytes() and np.allclose(a, b, rtol=1e-14, atol=0)


@pytest.mark.parametrize('D', [1, 2, 3, 8, 12])
def test_factor_inside_highams_bound(D):
    rs = np.random.RandomState(10 + D)
    B = rs.standard_normal((D, D + 3)) * rs.uniform(0.1, 10.0, size=(D, 1))
    A = B @ B.T
    A = 0.5 * (A + A.T)
    L, ok = DM.cholesky_lower(A)
    assert ok and L.tobytes() == DM.cholesky_columns(A).tobytes()            # the header's statement, literally
    assert np.all(np.triu(L, 1) == 0.0) and not np.signbit(np.triu(L, 1)).any()
    Ln = np.linalg.cholesky(A)
    Lf, Lnf, Af = frac(L), frac(Ln), frac(A)
    res, bound = np.abs(Lf.dot(Lf.T) - Af), gamma(D + 1) * np.abs(Lf).dot(np.abs(Lf).T)
    resn, boundn = np.abs(Lnf.dot(Lnf.T) - Af), gamma(D + 1) * np.abs(Lnf).dot(np.abs(Lnf).T)
    between = np.abs(Lf.dot(Lf.T) - Lnf.dot(Lnf.T))
    for i in range(D):
        for j in range(i + 1):
            assert res[i, j] <= bound[i, j] and resn[i, j] <= boundn[i, j]
            assert between[i, j] <= bound[i, j] + boundn[i, j]


def test_factor_flags_what_has_no_factor():
    A = np.array([[4.0, 0, 0], [2.0, 1.0, 0], [0.0, 0.0, 1.0]])               # second pivot 1 - 1 = 0
    assert not DM.cholesky_lower(A)[1]
    assert not DM.cholesky_lower(np.array([[0.0]]))[1] and not DM.cholesky_lower(np.array([[np.inf]]))[1]
    assert not DM.cholesky_lower(np.array([[1.0, 0], [np.nan, 1.0]]))[1]
    assert DM.cholesky_lower(np.array([[1.0, np.nan], [0.5, 1.0]]))[1]         # above the diagonal: not read
    prev = np.arange(8.0).reshape(2, 2, 2)
    s1, s2 = np.zeros((2, 2)), np.array([[[3.0, 0], [1.0, 2.0]], [[3.0, 0], [1.0, 0.0]]])
    chol, work, status = DM.factor(s1, s2, 2, 4, False, prev)                  # N = 4
    assert status.tolist() == [0, 1] and chol[1].tobytes() == prev[1].tobytes()
    assert chol[0].tobytes() == work[0].tobytes() and np.allclose(chol[0] @ chol[0].T, [[1.0, 1 / 3.0], [1 / 3.0, 2 / 3.0]])


@pytest.mark.parametrize('Cg,G,n', [(5, 1, 3), (70, 2, 2), (130, 1, 1)])
def test_covariance_against_np_cov_inside_a_derived_tolerance(Cg, G, n):
    """d = x - k0 carries one rounding, a product of two of them three, and a sum of N terms in
    any order at most N - 1 more: every entry of s2 and of s1 is inside gamma_{N+2} of its
    exact value relative to the sum of magnitudes; (s1_i s1_j) / N, the subtraction and the
    division add four.  Hence, with room,
        |cov_ij - exact| <= gamma_{2N+16} (sum |d_i d_j| + sum |d_i| sum |d_j| / N) / (N - 1),
    and numpy's two-pass estimate is inside the same expression in its centred data."""
    C, D = Cg * G, 6
    rs = np.random.RandomState(Cg + n)
    A = rs.standard_normal((D, D))
    x = 5.0 + rs.standard_normal((n, C, D)) @ A.T
    m = DM.comoments(x, G)
    N = n * Cg
    cov = DM.covariance(m.s1, m.s2, n, C, False)
    g2 = float(gamma(2 * N + 16))
    for g in range(G):
        rec = x[:, g::G].reshape(N, D)
        want = np.cov(rec.T).reshape(D, D)
        d, e = np.abs(rec - m.k0[g]), np.abs(rec - rec.mean(axis=0))
        tol = g2 * (d.T @ d + np.outer(d.sum(0), d.sum(0)) / N) / (N - 1) + g2 * 2.0 * (e.T @ e) / (N - 1)
        low = np.tril(np.ones((D, D), dtype=bool))
        assert np.all(np.abs(cov[g] - want)[low] <= tol[low])
        assert np.all(cov[g][~low] == 0.0)
        # Stan's shrinkage on top
        reg = DM.covariance(m.s1, m.s2, n, C, True)[g]
        wreg = (N / (N + 5.0)) * want + 1e-3 * (5.0 / (N + 5.0)) * np.eye(D)
        assert np.all(np.abs(reg - wreg)[low] <= tol[low] + 4 * U * np.abs(wreg)[low])


def test_exact_bits_on_small_integer_data():
    """Small integers: every difference, product and sum is exact, so the restatement must give
    the integer results themselves whatever its order of operations."""
    rs = np.random.RandomState(7)
    n, Cg, G, D = 4, 67, 2, 5
    C = Cg * G
    x = rs.randint(-20, 21, size=(n, C, D)).astype(np.float64)
    m = DM.comoments(x, G)
    for g in range(G):
        d = (x[:, g::G] - x[0, g]).reshape(-1, D).astype(np.int64)
        assert np.array_equal(m.k0[g], x[0, g]) and np.array_equal(m.s1[g], d.sum(0))
        assert np.array_equal(np.tril(m.s2[g]), np.tril(d.T @ d))
    L0 = np.tril(rs.randint(-4, 5, size=(D, D))).astype(np.float64)
    L0[np.diag_indices(D)] = rs.randint(1, 5, size=D)
    L, ok = DM.cholesky_lower(L0 @ L0.T)
    assert ok and L.tobytes() == L0.tobytes()
    g = rs.randint(-9, 10, size=(3, D)).astype(np.float64)
    for fma in (False, True):
        assert np.array_equal(DM.lt_matvec(L0, g, fma), g @ L0) and np.array_equal(DM.l_matvec(L0, g, fma), g @ L0.T)
        assert np.array_equal(DM.kick(g, g, L0, 0.5, None, True, fma), g - 0.25 * (g @ L0))


def test_window_bookkeeping_n_calls_equal_one_pass_over_the_record():
    """n ``add`` calls of a window against ONE pass over the stacked [n * Cg x D] record of each
    group: bit for bit on integer data (every operation exact), inside the summation bound
    on real data; a window's first call forgets the window before it, and what lies above
    the diagonal of s2 is left as it was given."""
    rs = np.random.RandomState(8)
    n, Cg, G, D = 5, 66, 3, 4
    C = Cg * G
    xi = rs.randint(-30, 31, size=(n, C, D)).astype(np.float64)
    xr = 2.0 + rs.standard_normal((n, C, D))
    for x, exact in ((xi, True), (xr, False)):
        m = DM.CoMoments(G, above=np.nan)
        m.add(rs.standard_normal((C, D)) * 1e6)                      # an earlier window
        for t in range(n):
            m.add(x[t], first=t == 0)
        assert m.n == n
        for g in range(G):
            rec = x[:, g::G].reshape(n * Cg, D)
            d = rec - x[0, g]
            one1, one2 = d.sum(0), d.T @ d
            low = np.tril(np.ones((D, D), dtype=bool))
            assert np.isnan(m.s2[g][~low]).all()
            if exact:
                assert np.array_equal(m.s1[g], one1) and np.array_equal(m.s2[g][low], one2[low])
            else:
                k = float(gamma(n * Cg + 2))
                assert np.all(np.abs(m.s1[g] - one1) <= 2 * k * np.abs(d).sum(0))
                assert np.all(np.abs(m.s2[g] - one2)[low] <= 2 * k * (np.abs(d).T @ np.abs(d))[low])
    # ... and a whole restated warm-up counts its windows' draws the same way
    hmc = DM.DenseHMC(MR.GaussTarget(), rs.standard_normal((4, 3)), 0.2, 2, np.eye(3))
    w = DM.DenseWarmup(hmc, 40, 5, 5, 10)
    assert w.windows == [(5, 15), (15, 35)]
    for t in range(40):
        w.step(rs.standard_normal((4, 3)), rs.uniform(size=4))
        inside = [a for a, b in w.windows if a <= t < b]
        assert w.mom.n == (t - inside[0] + 1 if inside else (0 if t < 5 else 20))
    assert len(w.factors) == 2 and w.status.tolist() == [0]


# ---------------------------------------------------------------------------
# the statistical experiment (8 dimensions, sigma 1 ... 100, rotated; 16 chains from
# 3 sigma, 300 adapting transitions, windows (20, 40, 20), rates 1.02 / 0.9, 200 kept draws)
# ---------------------------------------------------------------------------
SEEDS = list(range(10))


def test_rotated_target_is_what_it_says():
    S, P, Ls = DM.rotated_target()
    assert np.allclose(np.linalg.eigvalsh(S), MR.SIGMA8 ** 2, rtol=1e-9) and np.allclose(S @ P, np.eye(8), atol=1e-9)
    sd = np.sqrt(np.diag(S))
    assert sd.max() / sd.min() < 4.0                  # marginal widths nearly alike: nothing for a diagonal metric


def test_dense_warmup_cures_the_rotated_gaussian_and_the_diagonal_one_does_not():
    """Bars: dense max split-R^ <= 1.1, diagonal >= 2, whitened eigenvalues of the learnt
    M^-1 inside [0.5, 2], over seeds 0 ... 9.  Measured with this restatement (DESIGN.md has
    the same figures): printed below, read with ``pytest -s``."""
    dense = [DM.experiment(s, 'dense')[:2] for s in SEEDS]
    diag = [DM.experiment(s, 'diag')[:2] for s in SEEDS]
    dr, de = [r for r, _ in dense], np.array([e for _, e in dense])
    gr, ge = [r for r, _ in diag], np.array([e for _, e in diag])
    print('dense:    max split-R^ %.3f ... %.3f, whitened eigenvalues %.3g ... %.3g' % (min(dr), max(dr), de.min(), de.max()))
    print('diagonal: max split-R^ %.3f ... %.3f, whitened eigenvalues %.3g ... %.3g' % (min(gr), max(gr), ge.min(), ge.max()))
    assert max(dr) <= 1.1
    assert min(gr) >= 2.0
    assert de.min() >= 0.5 and de.max() <= 2.0
    assert ge.max() / ge.min() > 100.0                # the diagonal metric leaves the condition number where it was


def test_no_metric_does_not_converge_either():
    r = [DM.experiment(s, 'none')[0] for s in SEEDS[:3]]
    print('none: max split-R^ %s' % ' '.join('%.3f' % v for v in r))
    assert min(r) >= 2.0


# ---------------------------------------------------------------------------
# refusals of the C ABI: host checks, nothing is launched (fake addresses)
# ---------------------------------------------------------------------------
def test_refusals_without_gpu():
    L = _native.lib()
    base = 1 << 40
    q, p, g, chol, dtc, work, s1, s2 = (base + (i << 32) for i in range(8))
    C, D, G = 6, 16, 3
    kick = lambda **k: L.binf_leapfrog_kick_dense_f64(k.get('p', p), k.get('g', g), k.get('chol', chol), k.get('G', G), 0.1,
                                                      k.get('dtc', None), 0, k.get('C', C), k.get('D', D),
                                                      k.get('mode', 0), None)
    drift = lambda **k: L.binf_leapfrog_drift_dense_f64(k.get('q', q), k.get('p', p), k.get('chol', chol), G, 0.1,
                                                        k.get('dtc', None), C, k.get('D', D), 0, None)
    kd = lambda **k: L.binf_leapfrog_kick_drift_dense_f64(k.get('q', q), k.get('p', p), k.get('g', g), k.get('chol', chol),
                                                          G, 0.1, k.get('dtc', None), C, k.get('D', D), 0, None)
    # sizes
    for f in (kick, drift, kd):
        assert f(D=1025) == _native.E_UNSUPPORTED and '1024' in _native.last_error()
        assert f(D=0) == 0
    assert kick(C=0) == 0 and kick(C=7) == _native.E_ARG and kick(G=0) == _native.E_ARG and kick(mode=5) == _native.E_ARG
    assert kick(C=-1) == _native.E_ARG and kick(p=None) == _native.E_ARG
    # the two overflows in their order: C*D is tested first, G*D*D where C*D fits
    big = lambda Cx: L.binf_leapfrog_kick_dense_f64(p, g, chol, 1 << 44, 0.1, None, 0, Cx, 1024, 0, None)
    assert big(1 << 60) == _native.E_ARG and 'C*D overflows' in _native.last_error()
    assert big(1 << 44) == _native.E_ARG and 'G*D*D overflows' in _native.last_error()
    # the same call with G not dividing C, through the scaled and the dense launcher of the one check
    for piece, bufs in (('kick', (p, g)), ('drift', (q, p)), ('kick_drift', (q, p, g))):
        tail = (0.1, None) + ((0,) if piece == 'kick' else ()) + (C, D, 0, None)
        for suffix in ('scaled', 'dense'):
            rc = getattr(L, 'binf_leapfrog_%s_%s_f64' % (piece, suffix))(*bufs, chol, 4, *tail)
            assert rc == _native.E_ARG and 'C = 6 is not a multiple of G = 4' in _native.last_error(), (piece, suffix)
    # aliases: those of the scaled entry points, the factor in the scale's place
    CD, n = C * D * 8, C * D
    assert kick(chol=p + CD - 8) == _native.E_ALIAS and kick(chol=p - G * D * D * 8 + 8) == _native.E_ALIAS
    assert drift(chol=q + 8) == _native.E_ALIAS and kd(chol=q + 8) == _native.E_ALIAS and kd(chol=p + 8) == _native.E_ALIAS
    assert kick(dtc=p + 8) == _native.E_ALIAS and drift(dtc=q + 8) == _native.E_ALIAS
    assert drift(p=q + 8) == _native.E_ALIAS and kd(p=q + CD - 8) == _native.E_ALIAS
    assert kick(g=p + 8) == _native.E_ALIAS and kd(g=q + 8) == _native.E_ALIAS and kd(g=q) == _native.E_ALIAS
    # the co-moments
    com = lambda **k: L.binf_metric_comoments_f64(k.get('x', q), k.get('k0', p), k.get('s1', s1), k.get('s2', s2), 1,
                                                  k.get('C', C), k.get('D', D), k.get('G', G), None)
    assert com(D=1025) == _native.E_UNSUPPORTED and com(C=0) == 0 and com(D=0) == 0
    assert com(C=7) == _native.E_ARG and com(G=0) == _native.E_ARG and com(x=None) == _native.E_ARG
    assert com(k0=q + 8) == _native.E_ALIAS and com(s1=s2 + G * D * D * 8 - 8) == _native.E_ALIAS
    assert com(s2=q - 8) == _native.E_ALIAS and com(k0=s1 + 8) == _native.E_ALIAS
    # the factor
    fac = lambda **k: L.binf_metric_factor_f64(k.get('s1', s1), k.get('s2', s2), k.get('n', 5), k.get('C', C),
                                               k.get('D', D), k.get('G', G), 1, k.get('chol', chol),
                                               k.get('work', work), None, None)
    assert fac(D=1025) == _native.E_UNSUPPORTED and fac(C=0) == 0 and fac(D=0) == 0
    assert fac(n=0) == _native.E_ARG and fac(C=7) == _native.E_ARG and fac(work=None) == _native.E_ARG
    assert fac(n=1, C=3) == _native.E_ARG and 'N' in _native.last_error()       # N = 1
    assert fac(n=(1 << 53) // 2 + 1) == _native.E_UNSUPPORTED and '2^53' in _native.last_error()
    assert fac(work=chol + 8) == _native.E_ALIAS and fac(chol=s2 + 8) == _native.E_ALIAS
    assert fac(work=s1 + 8) == _native.E_ALIAS and fac(chol=s1 - 8) == _native.E_ALIAS
    with pytest.raises(NotImplementedError):
        _native.check(fac(D=1025), 'binf_metric_factor_f64')
