"""``binf_gauss_pointwise_loglik_f64``, ``binf_psis_loo_f64``, ``binf_pointwise_totals_f64`` and
their host layer ``binf_amd/loo.py`` against the restatement of tests/loo_ref.py.

The record: every element inside ``loo_ref.pointwise_bound`` of the mpmath value (a sample of
the elements; all of them within twice the bound of numpy's, which the CPU tests hold to the
same bound), and EQUAL to numpy's bits wherever ``precision[s]`` is 1.0.

PSIS: per output |device - 50-digit value| <= 32 x max(e_host, 2^-53 |value|), e_host the
restatement's own largest error on the same record (``test_loo.host_error``; never measured by
device code).  Why 32: the device library's exp, log, log1p and expm1 may be an ulp or two off
where numpy's are within one, and each enters at first order with a small constant, as the
restatement's do; an algorithmic slip (a wrong M, candidate grid or quartile index, a missing
prior term, the tail paired the wrong way round) moves khat by 1e-3 or more, twelve orders
above.  Columns without an mpmath value are held to 33 x the same against the double
restatement (loo_ref's docstring).  ``tail_len`` is equal.  The calls go through the C ABI with
every output and the workspace between sentinels.

``loo()`` itself is then held to properties that need no tolerance (a permutation of the draws,
a column alone or among 65, strided views, a NaN or an inf in one column) and to an end-to-end
run on polynomial fits.

Worst |device - reference| / bar on an MI355X over S in {5 .. 20000} x N in {1, 3, 64, 65}, from
the tests' own printout: pareto_tail_02 0.069, one_dominant 0.061, pareto_tail_09 0.061,
pareto_tail_05 0.058, gaussian_model 0.051, near_flat_tail 0.032, flat 0.031, wide 0.031;
S = 2^22: every output equal to the double restatement's bits; ``loo()`` on the analytic
record 0.060, the end-to-end fits 0.072 (degree 2) and 0.053 (degree 3).  The record: worst
|device - exact| / bound 0.565 (257 x 64), 0.515 (300 x 1000), 0.423 (17 x 65), 0.325 (1 x 1),
0.218 (5 x 3).  Each test prints its own.
"""
import math

import numpy as np
import pytest
import torch

import loo_ref as R
from binf_amd import _native, loo
from binf_amd.example.likelihood import POLYVAL, make_likelihood
from test_loo import degree_data, host_error

pytestmark = pytest.mark.gpu

SENT = -7.25
U = R.U


def dev_t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device)


def carve(a, device, before=0, after=0):
    """``a`` on the device inside a larger sentinel-filled buffer: (view, whole buffer)."""
    flat = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    whole = torch.full((before + flat.size + after,), SENT, dtype=torch.float64, device=device)
    view = whole[before:before + flat.size]
    view.copy_(torch.from_numpy(flat))
    return view, whole


def guards_intact(whole, before, n):
    w = whole.cpu().numpy()
    return bool(np.all(w[:before] == SENT) and np.all(w[before + n:] == SENT))


# ---------------------------------------------------------------------------
# the record
# ---------------------------------------------------------------------------
def abi_record(device, mock, tau, ys, rc_want=0):
    L = _native.lib()
    S, N = mock.shape
    md, mw = carve(mock, device, 1, 1)
    td, tw = carve(tau, device, 3, 1)
    yd, yw = carve(ys, device, 1, 2)
    od, ow = carve(np.full(S * N, SENT), device, 3, 5)
    kept = [w.clone() for w in (mw, tw, yw)]
    rc = L.binf_gauss_pointwise_loglik_f64(md.data_ptr(), td.data_ptr(), yd.data_ptr(), od.data_ptr(), S, N,
                                           R.HALF_LOG_2PI, _native.stream_handle(device))
    assert rc == rc_want, _native.last_error()
    torch.cuda.synchronize()
    assert guards_intact(ow, 3, S * N)
    for w, k in zip((mw, tw, yw), kept):
        assert torch.equal(w.view(torch.int64), k.view(torch.int64))
    return od.cpu().numpy().reshape(S, N)


@pytest.mark.parametrize('S,N', [(1, 1), (5, 3), (17, 65), (257, 64), (300, 1000)])
def test_pointwise_record_inside_its_bound_and_equal_to_numpy_at_unit_precision(device, S, N):
    rs = np.random.RandomState(S * 31 + N)
    mock, ys = rs.standard_normal((S, N)) * 2, rs.standard_normal(N)
    tau = rs.gamma(4.0, 0.5, size=S)
    tau[::3] = 1.0
    if S >= 5:
        tau[1], tau[4] = -2.0, 0.0
        mock[3, N - 1] = np.nan                   # a row of unit precision
        tau[2] = 1e-300
    got = abi_record(device, mock, tau, ys)
    want = R.pointwise_terms(mock, tau, ys)
    unit = tau == 1.0
    assert unit.any() and np.array_equal(got[unit], want[unit], equal_nan=True)
    if S >= 5:
        assert np.all(np.isnan(got[1])) and np.all(got[4] == -np.inf) and np.isnan(got[3, N - 1])
        assert np.all(np.isfinite(got[3, :N - 1]))
    ok = (tau > 0)[:, None] & np.isfinite(mock)
    with np.errstate(all='ignore'):
        a = 0.5 * (mock - ys[None]) ** 2 * tau[:, None]
        h = np.broadcast_to((0.5 * np.log(tau))[:, None], a.shape)
        bound = 1.01 * (U * (6.0 * a + 4.0 * np.abs(h) + R.HALF_LOG_2PI) + R.Q * (0.5 * tau[:, None] + 1.0))
    assert np.all(np.abs(got[ok] - want[ok]) <= 2.0 * bound[ok])
    worst = 0.0
    flat = np.flatnonzero(ok.reshape(-1))
    for e in flat[::max(1, flat.size // 60)]:
        s, i = divmod(int(e), N)
        ex, am, hm = R.pointwise_exact(mock[s, i], ys[i], tau[s])
        b = R.pointwise_bound(am, hm, tau[s])
        assert abs(b - bound[s, i]) <= 1e-9 * b
        ratio = float(abs(float(got[s, i]) - ex)) / b
        assert ratio <= 1.0, (s, i, got[s, i], ratio)
        worst = max(worst, ratio)
    print('record %d x %d: worst |device - exact| / bound = %.3f' % (S, N, worst))


def test_pointwise_convenience_form(device):
    """(likelihood, samples): the forward kernels for the polynomial and the 'linear' kind, any
    other forward model as given; BinfState sequences as predict_grid takes them."""
    from binf_amd.model.linear import LinearForwardModel
    from binf_amd.example.likelihood import ForwardModel, GaussianErrorModel
    from binf_amd.pdf.likelihoods import Likelihood
    from binf_amd.samplers import BinfState
    rs = np.random.RandomState(4)
    xs, ys = np.linspace(-1, 1, 11), rs.standard_normal(11)
    c, tau = dev_t(rs.standard_normal((6, 3)), device), dev_t(rs.gamma(4.0, 0.5, size=6), device)
    lik = make_likelihood(xs, ys, POLYVAL)
    want = loo.pointwise_log_likelihood(_native.poly_forward(c, dev_t(xs, device)), tau, dev_t(ys, device))
    assert want.shape == (6, 11)
    assert torch.equal(loo.pointwise_log_likelihood(lik, (c, tau)), want)
    states = [BinfState(dict(coefficients=c[i:i + 2], precision=tau[i:i + 2])) for i in (0, 2, 4)]
    assert torch.equal(loo.pointwise_log_likelihood(lik, states), want)
    host = R.pointwise_terms(np.array([[np.polynomial.polynomial.polyval(x, ci) for x in xs] for ci in c.cpu().numpy()]),
                             tau.cpu().numpy(), ys)
    assert np.all(np.abs(want.cpu().numpy() - host) <= 1e-13 * (1.0 + np.abs(host)))
    design = np.vstack([xs ** k for k in range(3)])
    lin = Likelihood('points', LinearForwardModel('basis', design, variable='coefficients'), GaussianErrorModel(ys))
    assert torch.equal(loo.pointwise_log_likelihood(lin, (c, tau)),
                       loo.pointwise_log_likelihood(_native.linear_forward(c, dev_t(design, device)), tau,
                                                    dev_t(ys, device)))
    calls = []

    def own(xses, coefficients):
        calls.append(tuple(coefficients.shape))
        return _native.poly_forward(coefficients, dev_t(xses, device))
    other = Likelihood('points', ForwardModel(xs, own), GaussianErrorModel(ys))
    assert torch.equal(loo.pointwise_log_likelihood(other, (c, tau)), want) and calls == [(6, 3)]


# ---------------------------------------------------------------------------
# PSIS through the C ABI
# ---------------------------------------------------------------------------
def abi_psis(device, ll):
    """binf_psis_loo_f64 of the record ``ll [S x N]`` (sorted here, on the host) on carved
    buffers: dict of numpy arrays; guards and the input checked."""
    L = _native.lib()
    S, N = ll.shape
    srt = np.ascontiguousarray(np.sort(ll, axis=0).T)
    sd, sw = carve(srt, device, 1, 1)
    outs = [carve(np.full(N, SENT), device, 1 + k % 2, 3) for k in range(5)]
    tl_whole = torch.full((N + 5,), -77, dtype=torch.int32, device=device)
    tl = tl_whole[2:2 + N]
    need = L.binf_psis_loo_workspace_bytes(S, N)
    assert need == R.workspace_bytes(S, N) and need > 0
    wd, ww = carve(np.full(need // 8, SENT), device, 1, 5)
    kept = sw.clone()
    rc = L.binf_psis_loo_f64(sd.data_ptr(), S, N, *([o.data_ptr() for o, _ in outs] +
                                                    [tl.data_ptr(), wd.data_ptr(), need, _native.stream_handle(device)]))
    assert rc == 0, _native.last_error()
    torch.cuda.synchronize()
    for k, (o, w) in enumerate(outs):
        assert guards_intact(w, 1 + k % 2, N)
    assert guards_intact(ww, 1, need // 8)
    t = tl_whole.cpu().numpy()
    assert np.all(t[:2] == -77) and np.all(t[2 + N:] == -77)
    assert torch.equal(sw.view(torch.int64), kept.view(torch.int64))
    res = {k: o.cpu().numpy().copy() for k, (o, _) in zip(R.FIELDS, outs)}
    res['tail_len'] = t[2:2 + N].copy()
    return res


def ratio_to_bar(g, ref, e, factor):
    """|g - ref| / (factor x max(e, 2^-53 |ref|)); NaN and infinities must be equal."""
    ref_f = float(ref)
    if ref_f != ref_f:
        assert g != g, (g, ref_f)
        return 0.0
    if math.isinf(ref_f):
        assert g == ref_f, (g, ref_f)
        return 0.0
    if g == ref:
        return 0.0
    assert g == g and not math.isinf(g), (g, ref_f)
    bar = factor * max(e, U * abs(ref_f))
    return float(abs(g - ref)) / bar


def hold_record(got, cols, f, e, exact, label):
    """Columns ``cols`` of the base record: 33 x against the double restatement, 32 x against
    mpmath where there is a value.  The worst ratio."""
    import mpmath
    worst = 0.0
    assert np.array_equal(got['tail_len'], f['tail_len'][cols]), label
    for k in R.FIELDS:
        for n, i in enumerate(cols):
            g = float(got[k][n])
            r = ratio_to_bar(g, f[k][i], e[k], 33.0)
            assert r <= 1.0, (label, k, i, g, f[k][i], e[k], r)
            if i in exact:
                with mpmath.workdps(50):
                    r = ratio_to_bar(mpmath.mpf(g) if g == g and not math.isinf(g) else g, exact[i][k], e[k], 32.0)
                assert r <= 1.0, (label, k, i, g, float(exact[i][k]), e[k], r)
            worst = max(worst, r)
    return worst


SIZES = (5, 24, 25, 26, 100, 225, 226, 1000, 4097, 20000)
NS = (1, 3, 64, 65)


@pytest.mark.parametrize('S', SIZES)
@pytest.mark.parametrize('name', sorted(R.BUILDERS))
def test_psis_against_the_restatement(device, name, S):
    """One base record [S x 65] per builder and size; the calls with N = 1, 3, 64, 65 take its
    first N columns, so e_host is measured once, on the same inputs."""
    base = R.BUILDERS[name](S, 65)
    mp_cols = (0, 64) if S <= 1000 else (2,)
    f, e, exact = host_error(base, mp_columns=mp_cols)
    assert np.all(f['tail_len'] == R.tail_len(S))
    worst = 0.0
    for N in NS:
        got = abi_psis(device, base[:, :N])
        worst = max(worst, hold_record(got, list(range(N)), f, e, exact, '%s S=%d N=%d' % (name, S, N)))
    if name == 'flat':
        assert np.all(np.isinf(got['khat'])) and np.array_equal(got['elpd_loo'], base[0])
        assert np.array_equal(got['lppd'], base[0]) and np.all(got['n_eff'] == S)
    if S < 25:
        assert np.all(np.isinf(got['khat']))
    elif name not in ('flat',):
        assert np.all(np.isfinite(got['khat']))
    print('%s S=%d: worst |device - reference| / bar = %.3f; e_host %s'
          % (name, S, worst, ', '.join('%s %.1e' % kv for kv in sorted(e.items()))))


def test_psis_at_the_largest_supported_size(device):
    """S = 2^22: M = 6144, 48 KiB of LDS, 512 chunks.  ll = -0.5 E on a fixed grid of exponential
    quantiles (no host sort of 4 M random numbers): khat near 0.5, against the double
    restatement of the one column."""
    S = 1 << 22
    p = (np.arange(S, dtype=np.float64) + 0.5) / S
    ll = (0.5 * np.log1p(-p[::-1]))[:, None]                   # -0.5 E, ascending
    assert np.all(np.diff(ll[:, 0]) >= 0)
    got = abi_psis(device, ll)
    f = R.psis_record(ll, R.F64)
    g = R.psis_record(ll, R.F80)
    assert got['tail_len'][0] == 6144 == f['tail_len'][0]
    for k in R.FIELDS:
        e = abs(float(f[k][0]) - float(g[k][0]))
        r = ratio_to_bar(float(got[k][0]), f[k][0], e, 33.0)
        print('S = 2^22 %s: device %.17g restatement %.17g ratio %.3f' % (k, got[k][0], f[k][0], r))
        assert r <= 1.0, (k, got[k][0], f[k][0], e)
    assert abs(got['khat'][0] - 0.5) < 4 * 1.5 / math.sqrt(6144)


# ---------------------------------------------------------------------------
# loo(): properties that need no tolerance
# ---------------------------------------------------------------------------
def same(a, b):
    """Two LOOResult / WAICResult equal bit for bit (NaN == NaN)."""
    for x, y in zip(a, b):
        if isinstance(x, torch.Tensor):
            if x.dtype == torch.float64:
                if not torch.equal(x.view(torch.int64), y.view(torch.int64)):
                    # NaNs need not share a payload
                    if not bool(((x == y) | (x.isnan() & y.isnan())).all()):
                        return False
            elif not torch.equal(x, y):
                return False
        elif not (x == y or (x != x and y != y)):
            return False
    return True


@pytest.fixture(scope='module')
def record(device):
    return dev_t(R.gaussian_model(1000, 65, seed=1), device)


def test_loo_matches_the_restatement_and_its_own_scalars(device, record):
    ll = record.cpu().numpy()
    f, e, _ = host_error(ll)
    r, w = loo.loo(record), loo.waic(record)
    got = dict(elpd_loo=r.elpd_i, khat=r.khat, n_eff=r.n_eff, lppd=w.lppd_i, p_waic=w.p_waic_i)
    got = {k: v.cpu().numpy() for k, v in got.items()}
    got['tail_len'] = r.tail_len.cpu().numpy()
    assert r.tail_len.dtype == torch.int32
    worst = hold_record(got, list(range(65)), f, e, {}, 'loo()')
    # the scalars are the fixed-order reductions of the device's own pointwise values
    s, ss = R.totals(got['elpd_loo'])
    sl, _ = R.totals(got['lppd'])
    assert r.elpd == s and r.se == R.se_of(ss, 65) and r.p_loo == sl - s
    assert r.n_bad == int((got['khat'] > 0.7).sum())
    sw, ssw = R.totals(got['lppd'] - got['p_waic'])
    assert w.elpd == sw and w.se == R.se_of(ssw, 65) and w.p_waic == R.totals(got['p_waic'])[0]
    d, sd = loo.compare(r, w)
    sdiff, ssd = R.totals(got['elpd_loo'] - (got['lppd'] - got['p_waic']))
    assert d == sdiff and sd == R.se_of(ssd, 65)
    assert loo.compare(r, r) == (0.0, 0.0)
    text = str(r)
    assert 'khat' in text and 'elpd_loo' in text and len(text.splitlines()) == 67
    assert 'p_waic' in w.table(names=['y%d' % i for i in range(65)])
    print('loo(): worst ratio %.3f; elpd %.4f +- %.4f, p_loo %.3f, n_bad %d' % (worst, r.elpd, r.se, r.p_loo, r.n_bad))


def test_a_permutation_of_the_draws_changes_no_bit(device, record):
    perm = torch.from_numpy(np.random.RandomState(7).permutation(record.shape[0])).to(device)
    assert same(loo.loo(record), loo.loo(record[perm].contiguous()))
    assert same(loo.waic(record), loo.waic(record[perm].contiguous()))


def test_a_column_alone_equals_the_column_among_65(device, record):
    whole, w_whole = loo.loo(record), loo.waic(record)
    for i in (0, 37, 64):
        for view in (record[:, i:i + 1], record[:, i:i + 1].contiguous()):
            one, w_one = loo.loo(view), loo.waic(view)
            for a, b in ((one.elpd_i, whole.elpd_i), (one.khat, whole.khat), (one.n_eff, whole.n_eff),
                         (w_one.lppd_i, w_whole.lppd_i), (w_one.p_waic_i, w_whole.p_waic_i)):
                assert torch.equal(a.view(torch.int64), b[i:i + 1].view(torch.int64)), i
            assert int(one.tail_len[0]) == int(whole.tail_len[i])


def test_strided_views_equal_their_contiguous_copies(device):
    rs = np.random.RandomState(11)
    wide = dev_t(-rs.exponential(size=(600, 90)) * 0.4, device)
    view = wide[:, 5:40]
    assert not view.is_contiguous()
    assert same(loo.loo(view), loo.loo(view.contiguous()))
    assert same(loo.waic(view), loo.waic(view.contiguous()))
    tcn = dev_t(-rs.exponential(size=(50, 12, 9)) * 0.4, device)                  # [T x C x N], C > 1
    flat = loo.loo(tcn.reshape(600, 9))
    assert same(loo.loo(tcn), flat)
    sub = tcn[:, 1::2, 2:7]                                                         # every other chain, a column slice
    assert not sub.is_contiguous()
    assert same(loo.loo(sub), loo.loo(sub.contiguous()))
    assert same(loo.loo(sub), loo.loo(sub.contiguous().reshape(300, 5)))


@pytest.mark.parametrize('bad', [float('nan'), float('inf'), float('-inf')])
def test_a_nan_or_an_inf_spoils_its_column_and_no_other_bit(device, record, bad):
    clean, w_clean = loo.loo(record), loo.waic(record)
    ll = record.clone()
    ll[123, 17] = bad
    r, w = loo.loo(ll), loo.waic(ll)
    keep = torch.ones(65, dtype=torch.bool, device=device)
    keep[17] = False
    for a, b in ((r.elpd_i, clean.elpd_i), (r.khat, clean.khat), (r.n_eff, clean.n_eff),
                 (w.lppd_i, w_clean.lppd_i), (w.p_waic_i, w_clean.p_waic_i)):
        assert bool(a[17].isnan())
        assert torch.equal(a[keep].view(torch.int64), b[keep].view(torch.int64))
    assert torch.equal(r.tail_len, clean.tail_len)
    assert r.elpd != r.elpd and w.elpd != w.elpd and r.n_bad == clean.n_bad


# ---------------------------------------------------------------------------
# end to end: polynomial fits of degree 2 and 3 to data from a cubic
# ---------------------------------------------------------------------------
def fit_degree(device, xs, ys, degree, seed):
    from binf_amd.example.priors import GammaPrior, GaussianPrior
    from binf_amd.example.samplers import make_hmc_sampler
    from binf_amd.pdf.posteriors import Posterior
    from binf_amd.samplers import BinfState
    from binf_amd.samplers.rng import DeviceRNG
    K, C = degree + 1, 256
    lik = make_likelihood(xs, ys, POLYVAL)
    pp, cp = GammaPrior(1.0, 0.2), GaussianPrior(np.zeros(K), np.ones(K) * 5)
    post = Posterior({lik.name: lik}, {pp.name: pp, cp.name: cp})
    start = BinfState(dict(coefficients=torch.ones((C, K), dtype=torch.float64, device=device),
                           precision=torch.ones(C, dtype=torch.float64, device=device)))
    gips = make_hmc_sampler(post, 0.01, 40, start, rng=DeviceRNG(seed, device))
    gips.sample_n(400, record=False)
    rec = gips.sample_n(200, thin=10)
    return lik, rec['coefficients'], rec['precision']


def test_polynomial_degrees_end_to_end(device):
    xs, ys = degree_data()
    results, records = {}, {}
    for degree in (2, 3):
        lik, c, tau = fit_degree(device, xs, ys, degree, seed=5)
        assert c.shape == (20, 256, degree + 1) and tau.shape == (20, 256)
        ll = loo.pointwise_log_likelihood(lik, (c, tau.reshape(-1)))
        assert ll.shape == (5120, 60)
        explicit = loo.pointwise_log_likelihood(
            _native.poly_forward(c.reshape(-1, degree + 1).contiguous(), dev_t(xs, device)), tau.reshape(-1).contiguous(),
            dev_t(ys, device))
        assert torch.equal(ll, explicit)
        r = loo.loo(ll.view(20, 256, 60))
        assert same(r, loo.loo(ll))
        f, e, _ = host_error(ll.cpu().numpy())
        got = dict(elpd_loo=r.elpd_i, khat=r.khat, n_eff=r.n_eff)
        w = loo.waic(ll)
        got.update(lppd=w.lppd_i, p_waic=w.p_waic_i)
        got = {k: v.cpu().numpy() for k, v in got.items()}
        got['tail_len'] = r.tail_len.cpu().numpy()
        worst = hold_record(got, list(range(60)), f, e, {}, 'degree %d' % degree)
        # n_bad only where no reference khat is within its bar of the threshold
        if np.all(np.abs(f['khat'] - 0.7) > 33.0 * np.maximum(e['khat'], U * np.abs(f['khat']))):
            assert r.n_bad == int((f['khat'] > 0.7).sum())
        print('degree %d: elpd_loo %.3f +- %.3f, p_loo %.2f, elpd_waic %.3f, max khat %.3f, n_bad %d; worst ratio %.3f'
              % (degree, r.elpd, r.se, r.p_loo, w.elpd, float(r.khat.max()), r.n_bad, worst))
        results[degree], records[degree] = r, f
    diff, se_diff = loo.compare(results[3], results[2])
    d_ref = records[3]['elpd_loo'] - records[2]['elpd_loo']
    s_ref, ss_ref = R.totals(d_ref)
    assert abs(diff - s_ref) <= 1e-9 * abs(s_ref) and abs(se_diff - R.se_of(ss_ref, 60)) <= 1e-9 * se_diff
    print('degree 3 against 2: elpd_diff %.3f, se_diff %.3f' % (diff, se_diff))
    assert diff > 2.0 * se_diff


# ---------------------------------------------------------------------------
# guards, on real buffers between sentinels
# ---------------------------------------------------------------------------
def test_refusals_touch_nothing(device):
    L = _native.lib()
    S, N = 300, 5
    srt = np.sort(R.pareto_tail(S, N), axis=0).T
    sd, sw = carve(srt, device, 1, 1)
    outs = [carve(np.full(N, SENT), device, 1, 3) for _ in range(6)]           # the sixth serves tail_len
    need = L.binf_psis_loo_workspace_bytes(S, N)
    wd, ww = carve(np.full(need // 8, SENT), device, 1, 5)
    st = _native.stream_handle(device)

    def call(S_=S, N_=N, o=None, ws=None, wb=need):
        o = [x.data_ptr() for x, _ in outs] if o is None else o
        return L.binf_psis_loo_f64(sd.data_ptr(), S_, N_, *(o + [wd.data_ptr() if ws is None else ws, wb, st]))
    ptrs = [x.data_ptr() for x, _ in outs]
    assert call(S_=1) == _native.E_ARG and call(N_=0) == _native.E_ARG
    assert call(S_=(1 << 22) + 1) == _native.E_UNSUPPORTED
    assert call(wb=need - 8) == _native.E_ARG
    assert call(ws=wd.data_ptr() + 4) == _native.E_ARG
    assert call(ws=ptrs[1]) == _native.E_ALIAS and call(ws=sd.data_ptr()) == _native.E_ALIAS
    assert call(o=[ptrs[0], ptrs[0]] + ptrs[2:]) == _native.E_ALIAS
    torch.cuda.synchronize()
    for o, w in outs:
        assert guards_intact(w, 1, N) and bool((o == SENT).all())
    assert guards_intact(ww, 1, need // 8) and bool((wd == SENT).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((outs[0][0] != SENT).all())
    # the host layer
    with pytest.raises(ValueError):
        loo.loo(torch.zeros((1, 4), dtype=torch.float64, device=device))           # S < 2
    with pytest.raises(NotImplementedError):
        _native.psis_loo(torch.zeros((1, (1 << 22) + 1), dtype=torch.float64, device=device))
    with pytest.raises(ValueError):
        loo.loo(torch.zeros((10, 4), dtype=torch.float32, device=device))
    with pytest.raises((TypeError, ValueError)):
        loo.loo(torch.zeros((10, 4), dtype=torch.float64))                         # a host tensor
    with pytest.raises(ValueError):
        loo.compare(torch.zeros(4, dtype=torch.float64, device=device), torch.zeros(5, dtype=torch.float64, device=device))

    from binf_amd.model.errormodels import AbstractErrorModel

    class Other(AbstractErrorModel):
        def __init__(self):
            super(Other, self).__init__('other')

    class Fake(object):
        error_model, forward_model = Other(), None
    with pytest.raises(TypeError, match='loo\\(\\) directly'):
        loo.pointwise_log_likelihood(Fake(), (None, None))
