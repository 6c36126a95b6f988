"""CPU tests that hold the restatement of PSIS-LOO (tests/loo_ref.py) honest: against a model
whose leave-one-out densities have a closed form, against tails of known shape, against the
integers of the contract and against itself at 50 digits.  The last part also carries the
library's host-side refusals, which need no device.

``host_error`` (loo_ref) is the helper the GPU tests take their e_host from: the largest
|double restatement - exact| per output over the columns of one record."""
import math

import numpy as np
import pytest

import loo_ref as R
from binf_amd import _native
from loo_ref import host_error  # noqa: F401  (tests/test_gpu_loo.py imports it from here)


def test_tail_length_and_plan_integers():
    got = [R.tail_len(S) for S in (5, 24, 25, 26, 100, 225, 226, 4097)]
    assert got == [1, 4, 5, 5, 20, 45, 45, 193]
    assert R.tail_len(2) == 0 and R.tail_len(4) == 0 and R.tail_len(20000) == 425
    assert R.plan(1 << 22) == (6144, 30 + 78, 1536)
    assert R.plan(4000) == (190, 43, 48) and R.plan(51200) == (679, 56, 170)
    for M in range(5, 40):                       # q = floor(M / 4 + 0.5), in integers
        assert (M + 2) // 4 == int(M / 4 + 0.5)


def test_fixed_orders():
    """tree_sum is what it says: accumulator e mod W, then neighbours."""
    x = np.random.RandomState(0).standard_normal(1000)
    acc = np.zeros(64)
    for e, v in enumerate(x):
        acc[e % 64] += v
    while len(acc) > 1:
        acc = np.array([acc[2 * i] + acc[2 * i + 1] for i in range(len(acc) // 2)])
    assert R.tree_sum(x, 64, R.F64) == acc[0]
    big = np.random.RandomState(1).standard_normal(20000)
    want = 0.5
    for lo in range(0, 20000, 8192):
        want = want + R.tree_sum(big[lo:lo + 8192], 256, R.F64)
    assert R.chunked_sum(big, 0.5, R.F64) == want


def test_analytic_loo_of_the_conjugate_model():
    """y_i ~ N(mu, 1), flat prior, N = 40, one point at 4.5 sigma; S = 4000 exact posterior draws.
    Every elpd_i within 6 Monte-Carlo standard errors of log N(y_i | ybar_(-i), 1 + 1 / (N - 1));
    the standard error of log(sum w p / sum w) by the delta method on the self-normalised raw
    weights w = 1 / p: w p is constant, so se = sd(w) / (mean(w) sqrt(S)).  Every khat < 0.5."""
    N, S = 40, 4000
    y = R.gaussian_data(N)
    ll = R.gaussian_model(S, N)
    exact = R.gaussian_exact_elpd(y)
    got = R.psis_record(ll)
    w = np.exp(-(ll - ll.min(0)))
    se = w.std(0, ddof=1) / (w.mean(0) * math.sqrt(S))
    err = np.abs(got['elpd_loo'] - exact)
    print('analytic: sum exact %.4f, restatement %.4f; worst |elpd_i - exact| %.4f (%.2f se); largest khat %.3f'
          % (exact.sum(), got['elpd_loo'].sum(), err.max(), (err / se).max(), got['khat'].max()))
    assert np.all(err <= 6.0 * se), (err / se).max()
    assert abs(got['elpd_loo'].sum() - exact.sum()) <= 6.0 * se.sum()
    assert np.all(got['khat'] < 0.5)
    assert np.all(got['tail_len'] == 190)
    # the outlier is the hardest point and shows it
    assert np.argmax(got['khat']) == N - 1 and np.argmin(got['elpd_loo']) == N - 1
    # WAIC's pieces: lppd above elpd_loo, p_waic positive, elpd_waic close to elpd_loo
    assert np.all(got['lppd'] > got['elpd_loo']) and np.all(got['p_waic'] > 0)
    assert abs((got['lppd'] - got['p_waic']).sum() - got['elpd_loo'].sum()) < 0.5
    assert np.all(got['n_eff'] > 1.0) and np.all(got['n_eff'] <= S)


def test_tail_shape_is_recovered():
    """ll = -k E, E ~ Exp(1): Pareto ratios of shape k.  |khat - k| <= 4 (1 + k) / sqrt(M), four
    asymptotic standard deviations of the shape estimate, M = 190; the mean khat rises with k
    (the prior pulls 0.9 towards 0.5: that is the algorithm)."""
    S, M = 4000, 190
    means = []
    for k in (0.2, 0.5, 0.9):
        kh = R.psis_record(R.pareto_tail(S, 20, seed=3, k=k))['khat']
        dev = np.abs(kh - k).max()
        print('k = %.1f: worst |khat - k| %.3f against %.3f, mean khat %.3f' % (k, dev, 4 * (1 + k) / math.sqrt(M), kh.mean()))
        assert dev <= 4.0 * (1.0 + k) / math.sqrt(M)
        means.append(kh.mean())
    assert means[0] < means[1] < means[2]


def test_edge_columns():
    S = 100
    c = R.psis_column(np.full(S, -0.75))
    assert c['khat'] == np.inf and c['elpd_loo'] == -0.75 and c['lppd'] == -0.75 and c['n_eff'] == S
    assert c['p_waic'] == 0.0 and c['tail_len'] == 20
    short = R.psis_column(np.sort(np.random.RandomState(2).standard_normal(24)))     # M = 4: no fit
    assert short['khat'] == np.inf and short['tail_len'] == 4 and np.isfinite(short['elpd_loo'])
    a = np.sort(np.random.RandomState(3).standard_normal(S))
    for bad in (np.nan, np.inf, -np.inf):
        b = a.copy()
        b[0 if bad == -np.inf else S - 1] = bad
        r = R.psis_column(b)
        assert all(r[k] != r[k] for k in R.FIELDS) and r['tail_len'] == 20
    # raw importance sampling where nothing is smoothed: elpd_loo = -log mean exp(-a)
    two = R.psis_column(np.array([-2.0, -1.0]))
    assert abs(two['elpd_loo'] + math.log(0.5 * (math.exp(2.0) + math.exp(1.0)))) < 1e-15


@pytest.mark.parametrize('name', sorted(R.BUILDERS))
def test_double_restatement_against_50_digits(name):
    """e_host per output on every builder the GPU tests use.  On the well-conditioned builders it
    stays below S 2^-53 (1 + |value|) x 100: at most S roundings in any sum, each a relative
    2^-53, and the fit's amplification (measured against 80 bits on the analytic case: 2e-15 on
    elpd, 3e-15 on khat) inside the factor 100.  near_flat_tail is ill-conditioned by
    construction (exceedances of a few 2^-53): its e_host is only recorded."""
    worst = {k: 0.0 for k in R.FIELDS}
    for S, N in ((26, 3), (226, 3), (1000, 2)):
        ll = R.BUILDERS[name](S, N)
        f, e, exact = host_error(ll, mp_columns=range(N))
        for i, ex in exact.items():
            assert ex['tail_len'] == f['tail_len'][i] == R.tail_len(S)
        for k in R.FIELDS:
            worst[k] = max(worst[k], e[k])
            if name != 'near_flat_tail':
                scale = 1.0 + max(abs(float(v)) for v in f[k] if np.isfinite(v)) if np.any(np.isfinite(f[k])) else 1.0
                assert e[k] <= 100.0 * S * R.U * scale, (name, S, k, e[k])
    print('%s: e_host %s' % (name, ', '.join('%s %.2e' % kv for kv in sorted(worst.items()))))


def degree_data(seed=11):
    """(xs, ys): N = 60 points of the cubic 2 - 4 x + x^2 + 1.5 x^3 on [-2, 2] with noise of
    precision 2.5 -- the data of the end-to-end test (tests/test_gpu_loo.py)."""
    rs = np.random.RandomState(seed)
    xs = np.linspace(-2.0, 2.0, 60)
    ys = np.polynomial.polynomial.polyval(xs, [2.0, -4.0, 1.0, 1.5]) + rs.standard_normal(60) / math.sqrt(2.5)
    return xs, ys


def host_gibbs(xs, ys, degree, n_draws, seed):
    """Exact Gibbs draws on the host of the example's posterior as its conditionals are written
    (binf_amd/example/samplers.py): coefficients | tau Gaussian (prior variance 5), tau |
    coefficients Gamma(n / 2, 1 + chi^2 / 2).  (coefficients [S x K], precision [S])."""
    rs = np.random.RandomState(seed)
    A = np.vstack([xs ** k for k in range(degree + 1)]).T
    tau, cs, ts = 1.0, [], []
    for it in range(n_draws + 50):
        prec = tau * A.T.dot(A) + np.eye(degree + 1) / 5.0
        cov = np.linalg.inv(prec)
        c = rs.multivariate_normal(cov.dot(tau * A.T.dot(ys)), cov)
        tau = rs.gamma(0.5 * len(ys)) / (1.0 + 0.5 * np.sum((A.dot(c) - ys) ** 2))
        if it >= 50:
            cs.append(c)
            ts.append(tau)
    return np.array(cs), np.array(ts)


def test_the_cubic_beats_the_quadratic_on_host_draws():
    """The margin the end-to-end GPU test pins, checked here first with the restatement on
    host-generated posterior draws: degree 3 beats degree 2 by far more than 2 se_diff on the
    data of ``degree_data`` (the cubic term is 1.5 x^3 on [-2, 2] against noise of sd 0.63)."""
    xs, ys = degree_data()
    elpd = {}
    for degree in (2, 3):
        c, tau = host_gibbs(xs, ys, degree, 2000, seed=degree)
        mock = np.array([np.polynomial.polynomial.polyval(xs, ci) for ci in c])
        r = R.psis_record(R.pointwise_terms(mock, tau, ys))
        elpd[degree] = r['elpd_loo']
        print('degree %d: elpd_loo %.3f, max khat %.3f' % (degree, r['elpd_loo'].sum(), r['khat'].max()))
    s, ss = R.totals(elpd[3] - elpd[2])
    print('degree 3 against 2: elpd_diff %.3f, se_diff %.3f' % (s, R.se_of(ss, 60)))
    assert s > 2.0 * R.se_of(ss, 60)


def test_pointwise_bound_holds_for_numpy():
    """numpy's evaluation of the record is inside pointwise_bound of the exact value (its log is
    within an ulp as well), and the non-finite cases fall as the contract says."""
    rs = np.random.RandomState(5)
    S, N = 7, 9
    mock, ys = rs.standard_normal((S, N)) * 3, rs.standard_normal(N)
    tau = np.array([1.0, 2.5, 1e-300, 1e300, 0.3, 7.0, 1.0])
    got = R.pointwise_terms(mock, tau, ys)
    for s in range(S):
        for i in range(N):
            ex, a, h = R.pointwise_exact(mock[s, i], ys[i], tau[s])
            assert abs(float(got[s, i] - ex)) <= R.pointwise_bound(a, h, tau[s]), (s, i)
    bad = R.pointwise_terms(mock, np.array([-1.0, 0.0, 1, 1, 1, 1, 1.0]), ys)
    assert np.all(np.isnan(bad[0])) and np.all(bad[1] == -np.inf) and np.all(np.isfinite(bad[2:]))


def test_library_refusals_need_no_device():
    """Every refusal of the new entry points is decided on the host, before anything is touched:
    fake pointers are never dereferenced."""
    L = _native.lib()
    base = 1 << 40
    S, N = 1000, 7
    need = L.binf_psis_loo_workspace_bytes(S, N)
    assert need == R.workspace_bytes(S, N) == 8 * N * (8 + 4) and need > 0
    assert L.binf_psis_loo_workspace_bytes(20000, 3) == 8 * 3 * (8 + 4 * 3)
    for s, n in ((1, N), (S, 0), ((1 << 22) + 1, N), (S, 1 << 31)):
        assert L.binf_psis_loo_workspace_bytes(s, n) == 0
    assert L.binf_psis_loo_workspace_bytes(1 << 22, 1) == 8 * (8 + 4 * 512)
    srt = base
    outs = [base + (1 << 30) + (i << 20) for i in range(6)]
    ws = base + (2 << 30)

    def call(S_=S, N_=N, srt_=srt, outs_=outs, ws_=ws, wb=need):
        return L.binf_psis_loo_f64(srt_, S_, N_, *(list(outs_) + [ws_, wb, None]))
    assert call(S_=1) == _native.E_ARG and 'S>=2' in _native.last_error()
    assert call(N_=0) == _native.E_ARG
    assert call(S_=(1 << 22) + 1, wb=1 << 40) == _native.E_UNSUPPORTED and '2^22' in _native.last_error()
    assert call(wb=need - 8) == _native.E_ARG and 'workspace' in _native.last_error()
    assert call(ws_=None) == _native.E_ARG
    assert call(ws_=ws + 4) == _native.E_ARG and 'aligned' in _native.last_error()
    assert call(ws_=srt + 8 * S * N - 8) == _native.E_ALIAS               # the workspace on the input's last value
    assert call(ws_=outs[2] - need + 8) == _native.E_ALIAS                # ... on an output
    assert call(outs_=[outs[0], outs[0] + 8] + outs[2:]) == _native.E_ALIAS
    assert call(outs_=outs[:5] + [outs[4] + 8 * N - 4]) == _native.E_ALIAS     # tail_len (int32) on p_waic's end
    assert call(outs_=[srt + 8] + outs[1:]) == _native.E_ALIAS
    assert call(outs_=[None] + outs[1:]) == _native.E_ARG
    with pytest.raises(NotImplementedError):
        _native.check(call(S_=(1 << 22) + 1, wb=1 << 40), 'x')
    # the record and the totals
    m, p, y, o = (base + (i << 32) for i in range(4))
    rec = L.binf_gauss_pointwise_loglik_f64
    assert rec(m, p, y, o, -1, 3, 0.9, None) == _native.E_ARG
    assert rec(m, p, y, None, 4, 3, 0.9, None) == _native.E_ARG
    assert rec(m, p, y, m + 8, 4, 3, 0.9, None) == _native.E_ALIAS
    assert rec(m, p, y, p, 4, 3, 0.9, None) == _native.E_ALIAS
    assert rec(m, p, y, y - 8 * 11, 4, 3, 0.9, None) == _native.E_ALIAS
    assert rec(m, p, y, o, 0, 3, 0.9, None) == 0 and rec(m, p, y, o, 4, 0, 0.9, None) == 0
    tot = L.binf_pointwise_totals_f64
    assert tot(m, None, 0, 5, None, 0.7, o, None) == _native.E_ARG
    assert tot(m, None, 2, 0, None, 0.7, o, None) == _native.E_ARG
    assert tot(m, None, 2, 5, None, 0.7, None, None) == _native.E_ARG
    assert tot(m, None, 2, 5, None, 0.7, m + 8 * 9, None) == _native.E_ALIAS
    assert tot(m, None, 2, 5, y, 0.7, y - 8 * 4, None) == _native.E_ALIAS      # out[4], the count, on khat[0]


def test_host_tensors_and_other_error_models_are_refused():
    import torch
    from binf_amd import loo
    from binf_amd.model.errormodels import AbstractErrorModel
    with pytest.raises((TypeError, ValueError)):
        loo.loo(torch.zeros((10, 3), dtype=torch.float64))
    with pytest.raises(TypeError):
        loo.loo(np.zeros((10, 3)))
    with pytest.raises(TypeError):
        loo.pointwise_log_likelihood(torch.zeros((4, 3), dtype=torch.float64), torch.ones(4, dtype=torch.float64),
                                     torch.zeros(3, dtype=torch.float64))

    class Other(AbstractErrorModel):
        def __init__(self):
            super(Other, self).__init__('other')

    class FakeLikelihood(object):
        error_model = Other()
        forward_model = None
    with pytest.raises(TypeError, match='loo\\(\\) directly'):
        loo.pointwise_log_likelihood(FakeLikelihood(), (None, None))
