"""Device run of tests/poly_range.py: the polynomial log-prob kernels (csrc/poly.hip), the row
reductions they go through (csrc/rowsum.hpp) and the Gaussian epilogue they share with the
pair-distance likelihood, fed the values where floating point goes wrong -- +-0, subnormals,
squares that underflow and overflow, the largest double, infinities, NaN -- and held to numpy bit
for bit wherever the arithmetic is numpy's (Horner at every KMAX instantiation exactly full and
first padded, chi^2 on every route of the reduction, the error-model gradient, the Gibbs rate)
and to exact arithmetic inside derived bounds where the device library's log enters (the epilogue
at general precision, the Gamma prior).  Ladders, cases, bounds and the assertion functions are
poly_range's; tests/test_poly_range.py shows on numpy alone that they reject subtly wrong kernels.

Every entry point is called through the C ABI.  ``Device(device, guarded=True)`` carves every
input and output from a NaN sentinel buffer, checks both guard zones after the call and that the
inputs kept their bits (``test_kernels_stay_inside_their_buffers``).

Largest measured fractions of the bounds, as printed by these tests (MI355X): DESIGN section 3.1."""
import numpy as np
import pytest
import torch

import poly_range as P
from binf_amd import _native
from binf_amd.example.priors import GammaPrior
from test_gpu_guards import Guarded, plain

pytestmark = pytest.mark.gpu
worst = {}


def _note(part, key, value):
    worst[(part, key)] = max(worst.get((part, key), 0.0), float(value))


def _report(part):
    print('largest fraction of the exact bound so far, %s: %s'
          % (part, ', '.join('%s %.3f' % (k[1], v) for k, v in sorted(worst.items()) if k[0] == part)))


def _ptr(t):
    return None if t is None else t.data_ptr()


class _Call(object):
    """The buffers of one group of C-ABI calls: plain tensors, or windows between guard zones."""

    def __init__(self, be):
        self.device = be.device
        self.guard = Guarded(be.device) if be.guarded else None
        self.inputs = []

    def _make(self, a, dtype):
        return self.guard(a, dtype) if self.guard is not None else plain(a, self.device, dtype)

    def put(self, a, dtype=torch.float64):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        t = self._make(a, dtype)
        self.inputs.append((t, a))
        return t

    def out(self, shape, fill=77.0, dtype=torch.float64):
        return self._make(np.full(shape, fill, dtype=np.uint8 if dtype == torch.uint8 else np.float64), dtype)

    def done(self):
        if self.guard is None:
            torch.cuda.synchronize()
            return
        self.guard.check()
        for t, a in self.inputs:
            back = t.cpu().numpy()
            if a.dtype == np.float64:
                assert np.array_equal(back.view(np.int64), a.view(np.int64)), 'an input changed'
            else:
                assert np.array_equal(back, a), 'an input changed'


class Device(object):
    """poly_range's backend interface on the device, through the C ABI."""

    def __init__(self, device, guarded=False):
        self.device, self.guarded = device, guarded
        self.L = _native.lib()
        self.st = _native.stream_handle(device)

    @staticmethod
    def _tau(call, tau):
        return (0.0, call.put(tau)) if np.ndim(tau) else (float(tau), None)

    @staticmethod
    def _host(t):
        return t.cpu().numpy().copy()

    def forward(self, theta, xs):
        (C, K), N = theta.shape, len(xs)
        call = _Call(self)
        th, x, o = call.put(theta), call.put(xs), call.out((C, N))
        assert self.L.binf_poly_forward_f64(_ptr(th), _ptr(x), _ptr(o), C, K, N, self.st) == 0
        call.done()
        return self._host(o)

    def err_grad(self, mock, ys, tau):
        C, N = mock.shape
        call = _Call(self)
        m, y, o = call.put(mock), call.put(ys), call.out((C, N))
        ts, tc = self._tau(call, tau)
        assert self.L.binf_gauss_err_grad_f64(_ptr(m), _ptr(y), ts, _ptr(tc), _ptr(o), C, N, self.st) == 0
        call.done()
        return self._host(o)

    def logp_routes(self, case, tau):
        (C, K), N = case['theta'].shape, len(case['xs'])
        call = _Call(self)
        th, x, y, m = call.put(case['theta']), call.put(case['xs']), call.put(case['ys']), call.put(case['mock'])
        ts, tc = self._tau(call, tau)
        o = [call.out(C) for _ in P.LOGP_ROUTES]
        L, st = self.L, self.st
        assert L.binf_gauss_err_logp_f64(_ptr(m), _ptr(y), ts, _ptr(tc), _ptr(o[0]), C, N, st) == 0
        assert L.binf_poly_gauss_logp_f64(_ptr(th), _ptr(x), _ptr(y), ts, _ptr(tc), _ptr(o[1]), C, K, N, st) == 0
        mc, ms = call.out((2, C, K), P.NAN), call.out((2, C), P.NAN)
        sk = call.out((2, C), 0, torch.uint8)
        reused = []
        for out in o[2:]:
            assert L.binf_poly_gauss_logp_memo_f64(_ptr(th), _ptr(x), _ptr(y), ts, _ptr(tc), _ptr(out), _ptr(mc),
                                                   _ptr(ms), _ptr(sk), C, K, N, st) == 0
            reused.append(sk[0].cpu().numpy().copy())
        call.done()
        # the first call summed every chain, the second reused every stored chi^2
        assert not reused[0].any() and reused[1].all()
        return dict((r, self._host(t)) for r, t in zip(P.LOGP_ROUTES, o))

    def chi2_routes(self, case):
        C, N = case['mock'].shape
        call = _Call(self)
        m, y, w = call.put(case['mock']), call.put(case['ys']), call.put(case['weights'])
        o = [call.out(C), call.out(C)]
        assert self.L.binf_row_sumsq_diff_f64(_ptr(m), _ptr(y), None, _ptr(o[0]), C, N, 1.0, self.st) == 0
        assert self.L.binf_row_sumsq_diff_f64(_ptr(m), _ptr(y), _ptr(w), _ptr(o[1]), C, N, 1.0, self.st) == 0
        call.done()
        return dict((r, self._host(t)) for r, t in zip(P.CHI2_ROUTES, o))

    def pairdist_logp(self, x, ys, tau):
        C, n = x.shape[0], x.shape[1] // 3
        I, J = np.triu_indices(n, 1)
        assert len(I) == len(ys)
        call = _Call(self)
        tx, ty = call.put(x), call.put(ys)
        ti, tj = call.put(I.astype(np.int32), torch.int32), call.put(J.astype(np.int32), torch.int32)
        ts, tc = self._tau(call, tau)
        o = call.out(C)
        ws, nbytes = _native._pairdist_chi2_workspace(C, n, len(I), self.device)
        assert self.L.binf_pairdist_gauss_logp_f64(_ptr(tx), _ptr(ti), _ptr(tj), _ptr(ty), ts, _ptr(tc), _ptr(o),
                                                   C, n, len(I), ws, nbytes, self.st) == 0
        call.done()
        return self._host(o)

    def gamma_logp(self, tau, shape, rate):
        call = _Call(self)
        t, o = call.put(tau), call.out(len(tau))
        assert self.L.binf_gamma_logp_f64(_ptr(t), float(shape), float(rate), _ptr(o), len(tau), self.st) == 0
        call.done()
        return self._host(o)

    def gamma_update(self, g, lp, rate):
        call = _Call(self)
        tg, tl, o = call.put(g), call.put(lp), call.out(len(g))
        assert self.L.binf_gamma_precision_update_f64(_ptr(tg), _ptr(tl), float(rate), _ptr(o), len(g), self.st) == 0
        call.done()
        return self._host(o)


# ---------------------------------------------------------------------------
# a. forward
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('K', P.K_LIST)
def test_forward_is_polyval_on_the_ladder(device, K):
    """binf_poly_forward_f64 at every KMAX instantiation exactly full and at its first padded K,
    xs the edge ladder: POLYVAL's bits on class F and O, the sign of a zero result and the overflow
    pattern included; class X: a non-finite coefficient stays in its chain, x = +-inf or NaN gives a
    NaN column (the padding's 0 + 0 * x too) and leaves the other columns alone."""
    be = Device(device)
    P.check_forward(be, P.forward_case('F', K), 'F K=%d' % K)
    P.check_forward(be, P.forward_case('O', K), 'O K=%d' % K)
    P.check_forward_spoiled(be, P.forward_case('F', K), 'K=%d' % K)


def test_forward_and_error_gradient_beyond_one_grid(device):
    """N = 65536 + 300: the grid of poly_forward_kernel and gauss_err_grad_kernel is capped at
    256 x 256 threads, and their stride loops turn."""
    be = Device(device)
    s = P.stride_case()
    P.check_forward(be, s, 'N = %d' % len(s['xs']))
    for tau in (2.5, np.array([0.3, -1.7])):
        P.check_err_grad(be, s['mock'], s['ys'], tau, 'N = %d' % len(s['xs']))


# ---------------------------------------------------------------------------
# b. the error model's gradient
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('C', (1, 9))
def test_error_gradient_on_every_pair_of_edges(device, C):
    """binf_gauss_err_grad_f64 == (mock - ys) * tau with mock, ys and tau over LADDER u NONFINITE:
    all 23 x 23 pairs of (mock, ys) at each of the 23 precisions, scalar, and per chain."""
    be = Device(device)
    mock, ys, scalars, vectors = P.err_grad_case(C)
    assert mock.shape == (C, 529)
    for tau in scalars + vectors:
        P.check_err_grad(be, mock, ys, tau, 'C=%d tau=%r' % (C, tau))


# ---------------------------------------------------------------------------
# c. chi^2 at precision 1
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('N', P.N_LIST)
@pytest.mark.parametrize('cls', ('F', 'O'))
def test_chi2_is_numpy_on_every_route(device, cls, N):
    """Every route of the reduction (leaf with and without tail, H = 1, 2, 3, the block kernel,
    height 7, two numpy chunks; the memo variant is the block kernel at every N): gauss_err_logp,
    poly_gauss_logp, the memo variant's first and reusing call, row_sumsq_diff with and without
    weights (d * d / w: class F weights positive and finite, so finite distinct sums; class O
    weights the whole ladder, zero included; class F with one weight at an edge) -- numpy's bits,
    1, 9 and 70 chains."""
    be = Device(device)
    for K in P.CHI_K:
        for C in P.C_LIST:
            P.check_chi2_unit(be, P.case(cls, K, N, C), '%s K=%d N=%d C=%d' % (cls, K, N, C))
    if N >= 1:
        P.check_chi2_unit(be, P.case('F', 5, N, 70, small_ys=True), 'F small ys N=%d' % N)
        if cls == 'F':
            for K, C in ((5, 9), (33, 70)):
                P.check_weight_edges(be, P.case('F', K, N, C), 'K=%d N=%d C=%d' % (K, N, C))


@pytest.mark.parametrize('cls', ('F', 'O'))
def test_chi2_is_numpy_at_every_instantiation(device, cls):
    be = Device(device)
    for K in P.K_LIST:
        P.check_chi2_unit(be, P.case(cls, K, 9, 9), '%s K=%d N=9' % (cls, K), poly_only=True)


# ---------------------------------------------------------------------------
# d. containment
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('N', P.SHARED_N)
def test_non_finite_rows_stay_in_their_row(device, N):
    """8, 4, 2 or 1 rows share a wave (H = 0 .. 3) and exchange partial sums by shuffles; N = 1025
    is the block kernel.  A chain spoiled with NaN, inf or -inf at row 0, 3 or 8 leaves every other
    row of every route its class F bits; a bad xs[n] makes every log-prob NaN, a bad ys[n] what
    numpy says."""
    be = Device(device)
    for K in (5, 33):
        cs = P.case('F', K, N, 9)
        P.check_containment(be, cs, 'K=%d N=%d' % (K, N))
        P.check_bad_datum(be, cs, 'K=%d N=%d' % (K, N))


# ---------------------------------------------------------------------------
# e. the epilogue at general precision
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('N', P.N_LIST)
@pytest.mark.parametrize('cls', ('F', 'F small ys', 'O'))
def test_epilogue_against_exact_arithmetic(device, cls, N):
    """lp = -0.5 chi2 tau + N 0.5 log(tau) on every polynomial route, scalar and per-chain
    precisions (1 +- one ulp, subnormal, 1e+-300, the largest double, 200 log-uniform in
    e^+-700; +-0, negative, inf, NaN): inside ``poly_range.logp_bound`` of exact arithmetic on
    chi2_f = -2 lp(tau = 1), numpy's own -inf / NaN where the result is not finite."""
    be = Device(device)
    cs = P.case(cls[0], 5, N, 70, small_ys=cls.endswith('ys'))
    w, held = P.check_epilogue(be, cs, '%s N=%d' % (cls, N))
    assert held > 0 or cls == 'O'
    for r, f in w.items():
        _note('e', r, f)
    print('%s N=%d: %d log-probs held to the bound, worst %s' % (cls, N, held, w))
    _report('e')


@pytest.mark.parametrize('cls', ('F', 'O'))
def test_epilogue_of_the_pair_distance_likelihood(device, cls):
    """The same epilogue behind binf_pairdist_gauss_logp_f64: 5 beads, all 10 pairs."""
    be = Device(device)
    for C in (9, 70):
        f, held = P.check_epilogue_pairdist(be, P.pairdist_case(cls, C), '%s C=%d' % (cls, C))
        assert held > 0 or cls == 'O'
        _note('e', 'pairdist_gauss_logp', f)
    _report('e')


# ---------------------------------------------------------------------------
# f, g. the Gamma prior and the Gibbs rate
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('shape,rate', P.GAMMA_PARAMS)
def test_gamma_prior_against_exact_arithmetic(device, shape, rate):
    """binf_gamma_logp_f64 with tau over the ladder (C = 1: each on its own; C = 257: then
    log-uniform fill): inside ``poly_range.gamma_bound``; numpy's own value at tau = +-0 (0 * -inf
    = NaN at shape = 1), negative, inf, NaN, and where tau * rate overflows.  GammaPrior.log_prob
    returns the same bits."""
    be = Device(device)
    for C in (1, 257):
        for tau in P.gamma_taus(C):
            _note('f', 'gamma_logp', P.check_gamma_logp(be, tau, shape, rate, 'C=%d' % C))
    tau = P.gamma_taus(257)[0]
    prior = GammaPrior(shape, rate)
    via = prior.log_prob(precision=plain(tau, device)).cpu().numpy()
    P.assert_same_bits(via, be.gamma_logp(tau, shape, rate), 'GammaPrior.log_prob')
    _report('f')


@pytest.mark.parametrize('rate', P.UPDATE_RATES)
def test_gibbs_rate_on_every_pair_of_edges(device, rate):
    """binf_gamma_precision_update_f64 == g / (-lp + rate), g and lp over LADDER u NONFINITE, all
    529 pairs in launches of 257, 257 and 15 chains."""
    be = Device(device)
    g, lp = P.update_pairs()
    assert len(g) == 529
    for a in range(0, len(g), 257):
        P.check_gamma_update(be, g[a:a + 257], lp[a:a + 257], rate, 'chains %d..' % a)


# ---------------------------------------------------------------------------
# h. guard zones
# ---------------------------------------------------------------------------
def test_kernels_stay_inside_their_buffers(device):
    """A share of (a) - (g) with every buffer a window between NaN guard zones: both zones of every
    buffer untouched, every input bit-identical afterwards, and the same assertions as on plain
    tensors (an out-of-bounds read that reaches the arithmetic shows as a differing bit)."""
    be = Device(device, guarded=True)
    for K in (5, 24, 37):
        P.check_forward(be, P.forward_case('F', K), 'guarded F K=%d' % K)
        P.check_forward(be, P.forward_case('O', K), 'guarded O K=%d' % K)
    s = P.stride_case()
    P.check_forward(be, s, 'guarded stride')
    P.check_err_grad(be, s['mock'], s['ys'], np.array([0.3, -1.7]), 'guarded stride')
    mock, ys, scalars, vectors = P.err_grad_case(9)
    for tau in scalars[::6] + vectors[:1]:
        P.check_err_grad(be, mock, ys, tau, 'guarded')
    for N in P.N_LIST:
        for cls in ('F', 'O'):
            P.check_chi2_unit(be, P.case(cls, 5, N, 9), 'guarded %s N=%d' % (cls, N))
    P.check_chi2_unit(be, P.case('F', 64, 1025, 3), 'guarded K=64')
    P.check_containment(be, P.case('F', 5, 129, 9), 'guarded')
    P.check_weight_edges(be, P.case('F', 5, 300, 9), 'guarded')
    scalars, vectors = P.tau_sets(9)
    w, held = P.check_epilogue(be, P.case('F', 5, 9, 9), 'guarded', scalars[::12], vectors[::5])
    assert held > 0
    f, held = P.check_epilogue_pairdist(be, P.pairdist_case('F', 9), 'guarded')
    assert held > 0
    for shape, rate in P.GAMMA_PARAMS[:2]:
        P.check_gamma_logp(be, P.gamma_taus(257)[0], shape, rate, 'guarded')
    g, lp = P.update_pairs()
    P.check_gamma_update(be, g[:257], lp[:257], 1.0, 'guarded')


def test_wrappers_return_the_bits_of_the_c_abi(device):
    """Beyond the issue's list (which asks this of GammaPrior.log_prob alone): the tests above call
    the C ABI directly, the class stack calls binf_amd._native's launchers -- the same bits."""
    be = Device(device)
    up = lambda a: plain(a, device)
    host = lambda t: t.cpu().numpy()
    cs = P.case('O', 5, 300, 9)
    tau = P.tau_sets(9)[1][0]
    got = be.logp_routes(cs, tau)
    th, xs, ys, mock, tt = up(cs['theta']), up(cs['xs']), up(cs['ys']), up(cs['mock']), up(tau)
    P.assert_same_bits(host(_native.poly_forward(th, xs)), be.forward(cs['theta'], cs['xs']), 'poly_forward')
    P.assert_same_bits(host(_native.gauss_err_logp(mock, ys, tt)), got['gauss_err_logp'], 'gauss_err_logp')
    P.assert_same_bits(host(_native.poly_gauss_logp(th, xs, ys, tt)), got['poly_gauss_logp'], 'poly_gauss_logp')
    memo = _native.new_chi2_memo(9, 5, device)
    for r in P.LOGP_ROUTES[2:]:
        P.assert_same_bits(host(_native.poly_gauss_logp_memo(th, xs, ys, tt, memo)), got[r], r)
    P.assert_same_bits(host(_native.gauss_err_grad(mock, ys, tt)), be.err_grad(cs['mock'], cs['ys'], tau), 'gauss_err_grad')
    chi = be.chi2_routes(cs)
    P.assert_same_bits(host(_native.row_sumsq_diff(mock, ys)), chi['row_sumsq_diff'], 'row_sumsq_diff')
    P.assert_same_bits(host(_native.row_sumsq_diff(mock, ys, weights=up(cs['weights']))),
                       chi['row_sumsq_diff weights'], 'row_sumsq_diff weights')
    g, lp = P.update_pairs()
    P.assert_same_bits(host(_native.gamma_precision_update(up(g[:257]), up(lp[:257]), -1.0)),
                       be.gamma_update(g[:257], lp[:257], -1.0), 'gamma_precision_update')
