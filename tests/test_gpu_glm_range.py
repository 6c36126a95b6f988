"""Device tests of the generalised-linear kernels (csrc/glm.hip, csrc/glm_term.hpp) over the
whole range of their term and on the contracts their linear-Gaussian twins are held to:

B.  the edge ladder (``glm_bounds.edge_ladder`` / ``edge_case``): every eta at which the term
    changes behaviour -- +-0.0, subnormals, where 1 + t rounds to 1, where t goes subnormal and
    then to 0, exp's overflow, 1e300 -- put exactly into the element-wise kernel, the fused
    log-prob, the fused gradient and the leapfrog.  (eta = -0.0 reaches the element-wise kernel
    only: the fused kernels form eta in a zero-initialised accumulator, +0.0 for a coefficient
    of either sign.)  Two Poisson rules, and no other exception:
    a chain with an eta above 700 is held by the per-datum bound of the element-wise kernel
    alone (``logp_bound``'s sum of e+ overflows there); a datum beyond exp's overflow
    (eta > 709.78) is ll = -inf, g = +inf exactly, its chain's log-prob -inf, its gradient an
    infinity of the design row's sign, never NaN, and its neighbours' bits unchanged.
C.  non-finite coefficients stay in their chain and fall as numpy says; guard zones round every
    buffer of the four entry points; the gradient's order contract (the splits follow from
    (C, N) alone: a chain's row does not depend on its place in a batch of the same C); the error
    models behind the polynomial forward model, as written.

Every tolerance is a derived bound of tests/glm_bounds.py.  Largest measured fractions of the
bound, as printed by these tests (MI355X): see DESIGN section 4.7."""
import math

import numpy as np
import pytest
import torch

import glm_bounds as G
import glm_ref as R
import poly_bounds as PB
from binf_amd import _native
from binf_amd.example.likelihood import POLYVAL, ForwardModel
from binf_amd.model.glm import BinomialLogitErrorModel, PoissonLogErrorModel
from binf_amd.model.linear import LinearForwardModel
from binf_amd.pdf import IsotropicGaussian
from binf_amd.pdf.likelihoods import Likelihood
from binf_amd.pdf.posteriors import Posterior
from binf_amd.samplers.hmc import HMCSampler
from test_gpu_guards import Guarded, plain

pytestmark = pytest.mark.gpu
NAMES = ('binomial', 'poisson')
worst = {}                     # largest error / bound seen by this module's bound tests, per part


def up(x, device):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(device)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int64)


def host(t):
    return t.detach().cpu().numpy()


def _model(family, ys, m, off):
    return BinomialLogitErrorModel(ys, m, off) if family == R.BINOMIAL_LOGIT else PoissonLogErrorModel(ys, off)


def _note(part, key, value):
    worst[(part, key)] = max(worst.get((part, key), 0.0), float(value))


def _report():
    print('largest fraction of the exact bound so far: %s'
          % ', '.join('%s/%s %.3f' % (k[0], k[1], v) for k, v in sorted(worst.items())))


# ---------------------------------------------------------------------------
# B. the edge ladder
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('family', R.FAMILIES)
def test_edge_ladder_pointwise(device, family):
    """binf_glm_pointwise_f64 handed the edge etas themselves as its mock tensor, no offset --
    the only route that can receive -0.0 (the check reads the tensor back from the device and
    holds it to the ladder's bits, sign of zero included): ``glm_bounds.edge_pointwise_check`` on
    every datum of every edge (the rules are stated there), the count of edges asserted at their
    own value against the length of the ladder; the ll-only and the g-only instantiations give
    the bits of the joint one."""
    data = G.edge_case(family, 1)
    _, ys, m, _, _ = data
    mock, dy, dm = up(G.edge_eta(data), device), up(ys, device), up(m, device)
    ll, g = _native.glm_pointwise(mock, dy, dm, None, family, None, want_ll=True, want_grad=True)
    assert bool(torch.signbit(mock[1]).all()) and not bool(torch.signbit(mock[0]).any())
    fig = G.edge_pointwise_check(family, data, host(mock), host(ll), host(g))
    print(NAMES[family], fig)
    assert fig['edges'] == len(G.edge_ladder())
    assert (fig['overflowed'] > 0) == (family == R.POISSON_LOG)
    ll1, none = _native.glm_pointwise(mock, dy, dm, None, family, None, want_ll=True, want_grad=False)
    assert none is None and torch.equal(bits(ll1), bits(ll))
    none, g1 = _native.glm_pointwise(mock, dy, dm, None, family, None, want_ll=False, want_grad=True)
    assert none is None and torch.equal(bits(g1), bits(g))
    _note('B', 'pointwise ll', fig['ll'])
    _note('B', 'pointwise g', fig['g'])
    _report()


@pytest.mark.parametrize('variant', (1, 2, 3))
@pytest.mark.parametrize('family', R.FAMILIES)
def test_edge_ladder_fused(device, family, variant):
    """binf_linear_glm_logp_f64 and binf_linear_glm_grad_f64 with chain c at edge c (variant 1:
    K = 1 and ``mock = theta * A`` exact; variant 2: K = 2 and an offset, both parts of eta
    nonzero; variant 3: K = 1 unscaled, so that Poisson chains sit between eta = 700 and exp's
    overflow): ``glm_bounds.edge_chain_check``, the counts it reports against those that follow
    from the ladder alone.  These kernels form eta in a zero-initialised accumulator: a -0.0
    coefficient gives eta = +0.0, so of the two zero edges they meet +0.0 twice.  The
    overflowed Poisson chains' neighbours are compared with a launch in which those chains'
    coefficients are zero: the same C, the same tiles."""
    data = G.edge_case(family, variant)
    A, ys, m, off, theta = data
    ln = _model(family, ys, m, off).log_norm
    dA, dy, dm, do = up(A, device), up(ys, device), up(m, device), up(off, device)

    def run(th):
        d = up(th, device)
        return (host(_native.linear_glm_logp(d, dA, dy, dm, do, family, ln)),
                host(_native.linear_glm_grad(d, dA, dy, dm, do, family)))

    lp, gr = run(theta)
    over = G.edge_overflow_chains(family, data)
    clean = None
    if over:
        th = theta.copy()
        th[over] = 0.0
        clean = run(th)
        # (finite wherever the dirty launch must be: its chains are compared with these bit for
        # bit below; the unscaled ladder's chains above eta = 700 may sum to -inf in both)
        assert np.all(np.isfinite(clean[0][over])) and np.all(np.isfinite(clean[1][over]))
    fig = G.edge_chain_check(family, data, ln, lp, gr, clean)
    print(NAMES[family], 'variant', variant, fig)
    assert (fig['edges'], fig['full'], fig['overflowed'], fig['pointwise_only']) == G.edge_counts(family, data)
    assert fig['edges'] + fig['pointwise_only'] == len(G.edge_ladder())
    assert (len(over) > 0) == (family == R.POISSON_LOG)
    assert (fig['pointwise_only'] > 0) == (family == R.POISSON_LOG and variant == 3)
    _note('B', 'logp', fig['logp'])
    _note('B', 'grad', fig['grad'])
    _report()


def _posterior(family, A, ys, m, off, prior):
    lik = Likelihood('outcomes', LinearForwardModel('covariates', A), _model(family, ys, m, off))
    priors = {'prior': IsotropicGaussian(prior[0], prior[1], name='prior', variable_name='coefficients')} \
        if prior else {}
    return Posterior({'outcomes': lik}, priors)


@pytest.mark.parametrize('variant', (1, 2))
@pytest.mark.parametrize('family', R.FAMILIES)
def test_edge_ladder_leapfrog(device, family, variant):
    """One step of binf_linear_glm_leapfrog_f64 from q = the ladder's edges with |eta| <= 700
    against the per-step sequence (HMCSampler._leapfrog with the fused leapfrog disabled): the
    same bits, EXACT and FMA, with and without the prior."""
    data = G.edge_case(family, variant)
    A, ys, m, off, theta = data
    chains = G.edge_moderate_chains(data)
    assert len(chains) >= 16
    theta = theta[chains]
    p0 = np.random.RandomState(3 + variant).standard_normal(theta.shape)
    for prior in (None, (0.7, 0.25)):
        post = _posterior(family, A, ys, m, off, prior)
        for mode in ('exact', 'fma'):
            res = []
            for fused in (True, False):
                s = HMCSampler(post, up(theta, device), 1e-3, 1, variable_name='coefficients', mode=mode)
                s.fused_leapfrog = fused
                q, p = up(theta, device), up(p0, device)
                s._leapfrog(q, p, 1e-3, 1)
                res.append((q, p))
            (qf, pf), (qs, ps) = res
            assert bool(torch.isfinite(qf).all()) and bool(torch.isfinite(pf).all())
            assert not torch.equal(qf, up(theta, device))
            assert torch.equal(bits(qf), bits(qs)) and torch.equal(bits(pf), bits(ps)), (prior, mode)


# ---------------------------------------------------------------------------
# C1. non-finite coefficients
# ---------------------------------------------------------------------------
def _same_non_finite(got, want, at):
    """NaN where numpy's value is NaN, equal to it where that is an infinity, finite elsewhere."""
    got, want = np.asarray(got), np.asarray(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), at
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]), at


@pytest.mark.parametrize('family', R.FAMILIES)
@pytest.mark.parametrize('K,N,C', [(7, 37, 40), (33, 1027, 40), (5, 19, 4100)])
def test_non_finite_coefficients(device, family, K, N, C):
    """One chain with +inf, one with -inf and one with NaN in one coefficient: their log-prob is
    not finite, and log-prob, gradient row and element-wise record are NaN where glm_ref.term on
    numpy's ``dirty @ A`` gives NaN and equal to it where that gives an infinity; every other
    chain carries the bits of the clean launch (the same C, so the same splits).

    (The binomial g is FINITE at eta = +-inf -- the logistic saturates at 0 and 1 -- so the
    gradient row of a binomial chain with an infinite coefficient is finite, as numpy's is: what
    is asserted of a gradient row is numpy's pattern, non-finite where numpy's row is.)"""
    A, ys, m, off, theta = G.case(family, K, N, C, 11 + K)
    em = _model(family, ys, m, off)
    ln, lc = em.log_norm, em.pointwise_constants
    c_inf, c_nan, c_minf = 5, 21, C - 2
    k_inf, k_nan = K // 2, K - 1
    dirty = theta.copy()
    dirty[c_inf, k_inf] = np.inf
    dirty[c_nan, k_nan] = np.nan
    dirty[c_minf, k_inf] = -np.inf
    touched = [c_inf, c_nan, c_minf]
    others = np.setdiff1d(np.arange(C), touched)
    dA, dy, dm, do, dlc = up(A, device), up(ys, device), up(m, device), up(off, device), up(lc, device)

    def run(th):
        d = up(th, device)
        with np.errstate(all='ignore'):
            mock = th.dot(A)
        ll, g = _native.glm_pointwise(up(mock, device), dy, dm, do, family, dlc, want_ll=True, want_grad=True)
        return [host(x) for x in (_native.linear_glm_logp(d, dA, dy, dm, do, family, ln),
                                  _native.linear_glm_grad(d, dA, dy, dm, do, family), ll, g)]

    clean, got = run(theta), run(dirty)
    with np.errstate(all='ignore'):
        wll, wg = R.term(family, R.eta_of(dirty.dot(A), off), ys, m)
        want = [np.sum(wll, axis=1) + ln, wg.dot(A.T), wll + lc, wg]
    assert np.isnan(want[0][c_nan]) and np.all(np.isnan(want[1][c_nan]))
    for c in touched:
        assert not np.isfinite(want[0][c]) and not np.isfinite(got[0][c]), c
        for name, a, b in zip(('logp', 'grad', 'll', 'g'), got, want):
            _same_non_finite(a[c], b[c], (name, c))
        if family == R.POISSON_LOG or c == c_nan:
            assert not np.any(np.isfinite(want[1][c])) and not np.any(np.isfinite(got[1][c])), c
    for a, b in zip(got, clean):
        assert np.array_equal(a[others].view(np.int64), b[others].view(np.int64))
        assert np.all(np.isfinite(b))


# ---------------------------------------------------------------------------
# C2. guard zones
# ---------------------------------------------------------------------------
GUARD_SHAPES = [(1, 1, 1), (5, 17, 3), (18, 35, 70), (36, 129, 3), (50, 48, 19), (64, 1025, 9), (5, 2049, 17),
                (33, 17, 4100)]


@pytest.mark.parametrize('family', R.FAMILIES)
@pytest.mark.parametrize('K,N,C', GUARD_SHAPES)
def test_kernels_stay_inside_their_buffers(device, family, K, N, C):
    """binf_glm_pointwise_f64, binf_linear_glm_logp_f64, binf_linear_glm_grad_f64 and
    binf_linear_glm_leapfrog_f64 with every input (theta, A, ys, trials, offset, lconst, dt_chain),
    every output and every workspace a window between NaN guard zones, with trials, offset and
    constants present and with all three null (the staging's "legal then unused" load through
    ys): the guard zones untouched, no NaN in any output, the bits of the same calls on plain
    tensors.  (64, 1025, 9): two log-prob pieces; (5, 2049, 17): 64 data splits over 129 tiles of
    which 21 are empty; (33, 17, 4100): two chain tiles per wave, one split."""
    L = _native.lib()
    st = _native.stream_handle(device)
    _, ys, m, off, _ = G.case(family, K, N, C, 7 + K + N)
    if m is None:
        m = np.ones(N)                              # the Poisson kernels stage trials and ignore them
    rs = np.random.RandomState(K * N + C)
    A = rs.standard_normal((K, N))                  # a gentle design: a trajectory that stays finite
    theta = 0.3 * rs.standard_normal((C, K)) / math.sqrt(K)
    p0, dtc = rs.standard_normal((C, K)), rs.uniform(5e-4, 2e-3, size=C)
    lc = _model(family, ys, m if family == R.BINOMIAL_LOGIT else None, off).pointwise_constants
    mock = theta.dot(A)
    need_lp = L.binf_linear_glm_logp_workspace_bytes(C, K, N)
    need_gr = L.binf_linear_glm_grad_workspace_bytes(C, K, N)
    need_lf = L.binf_linear_glm_leapfrog_workspace_bytes(C, K, N)
    tiles = (N + 15) // 16
    wgx = -(-C // (128 if C >= 4096 else 64))
    splits = max(1, min(64, tiles, -(-512 // wgx)))
    assert need_lp == (0 if N <= 1024 else -(-N // 1024) * C * 8)
    assert need_lf == splits * C * K * 8 and need_gr == (need_lf if splits > 1 else 0)
    if (K, N, C) == (5, 2049, 17):
        assert splits == 64 and 64 - -(-tiles // -(-tiles // 64)) == 21
    P = lambda x: None if x is None else x.data_ptr()
    for extras in (True, False):
        outs = []
        for make in (Guarded(device), None):
            t = make if make is not None else (lambda a: plain(a, device))
            th, Ad, yd, mk = t(theta), t(A), t(ys), t(mock)
            md, od, ld = (t(m), t(off), t(lc)) if extras else (None, None, None)
            ll, g = t(np.zeros((C, N))), t(np.zeros((C, N)))
            assert L.binf_glm_pointwise_f64(P(mk), P(yd), P(md), P(od), P(ld), family, P(ll), P(g), C, N, st) == 0
            lp, wlp = t(np.zeros(C)), t(np.zeros(max(1, need_lp // 8)))
            assert L.binf_linear_glm_logp_f64(P(th), P(Ad), P(yd), P(md), P(od), family, 0.75, P(lp),
                                              P(wlp) if need_lp else None, need_lp, C, K, N, st) == 0
            gr, wgr = t(np.zeros((C, K))), t(np.zeros(max(1, need_gr // 8)))
            assert L.binf_linear_glm_grad_f64(P(th), P(Ad), P(yd), P(md), P(od), family, P(gr),
                                              P(wgr) if need_gr else None, need_gr, C, K, N, st) == 0
            q, p, dt, wlf = t(theta), t(p0), t(dtc), t(np.zeros(need_lf // 8))
            assert L.binf_linear_glm_leapfrog_f64(P(q), P(p), P(Ad), P(yd), P(md), P(od), family, 1, 0.7, 0.25,
                                                  P(wlf), need_lf, C, K, N, 1e-3, P(dt), 2, _native.MODE_EXACT,
                                                  st) == 0
            if make is not None:
                make.check()
            else:
                torch.cuda.synchronize()
            outs.append([x.clone().cpu() for x in (ll, g, lp, wlp, gr, wgr, q, p, wlf, dt)])
        for a, b in zip(*outs):
            assert torch.equal(bits(a), bits(b)) and not torch.isnan(a).any()
        assert not torch.equal(outs[0][6], torch.from_numpy(theta))


# ---------------------------------------------------------------------------
# C3. the gradient's order contract
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('family', R.FAMILIES)
@pytest.mark.parametrize('K,N,C', [(33, 1027, 65), (5, 272, 4100)])
def test_gradient_row_does_not_depend_on_its_place(device, family, K, N, C):
    """The data splits follow from (C, N) alone and a chain's sums touch no other chain's: in a
    batch of the same C the gradient row of a chain carries the same bits wherever it stands --
    the chains permuted; one chain moved to rows 0, 16, 63, 64 and C - 1 -- and two calls give
    the same bits.  (Nothing is asserted across different C: the contract does not promise it.)"""
    A, ys, m, off, theta = G.case(family, K, N, C, 91 + K)
    dA, dy, dm, do = up(A, device), up(ys, device), up(m, device), up(off, device)
    f = lambda th: bits(_native.linear_glm_grad(up(th, device), dA, dy, dm, do, family))
    whole = f(theta)
    assert torch.equal(f(theta), whole)
    perm = np.random.RandomState(C).permutation(C)
    assert not np.array_equal(perm, np.arange(C))
    assert torch.equal(f(theta[perm]), whole[torch.from_numpy(perm)])
    for c in (0, 17, C - 1):
        for place in (0, 16, 63, 64, C - 1):
            batch = theta.copy()
            batch[place] = theta[c]
            assert torch.equal(f(batch)[place], whole[c]), (c, place)


# ---------------------------------------------------------------------------
# C4. behind another forward model
# ---------------------------------------------------------------------------
class _Spy(object):
    def __init__(self, monkeypatch, names):
        self.calls = []
        for n in names:
            monkeypatch.setattr(_native, n, self._wrap(n, getattr(_native, n)))

    def _wrap(self, name, fn):
        def spy(*a, **k):
            self.calls.append(name)
            return fn(*a, **k)
        return spy


SPIED = ('poly_forward', 'linear_forward', 'glm_pointwise', 'row_sum', 'jacobian_contract', 'linear_glm_logp',
         'linear_glm_grad', 'linear_glm_leapfrog')


@pytest.mark.parametrize('family', R.FAMILIES)
@pytest.mark.parametrize('K', [4, 7])
def test_error_models_behind_the_polynomial_forward_model(device, monkeypatch, family, K):
    """``Likelihood(ForwardModel(xs, polyval), BinomialLogitErrorModel / PoissonLogErrorModel)``:
    log_prob and gradient run as written (binf_poly_forward_f64, binf_glm_pointwise_f64, then
    binf_row_sum_f64 / binf_jacobian_contract_f64; none of the linear_glm entry points) and are
    held to ExactGLM on the Vandermonde design ``poly_bounds.design(xs, K)``.

    The mock datum's error model: csrc/poly.hip evaluates by Horner in polyval's order,
    ``v = c[K-1] + x * 0`` (exact) and K - 1 steps ``v = c[i] + v * x`` of one product and one
    addition each: 2 (K - 1) roundings, ``gamma_{2K-2} sum_k |theta_k| |x|^k`` (Higham, Accuracy
    and Stability, section 5.1).  The exact value is taken on the design's doubles
    ``fl(x**k)``, each within one ulp (2u, relative) of ``x**k``: 2u of the same sum.  Together
    ``gamma_{2K} S_n`` -- ``ExactGLM(..., roundings=2 K)``; everything after the mock datum is the
    model of glm_bounds unchanged."""
    N, C = 37, 19
    xs = np.linspace(-1.0, 1.0, N)
    _, ys, m, off, _ = G.case(family, K, N, C, 5 + K)
    theta = np.random.RandomState(40 + K).standard_normal((C, K)) * (30.0 / math.sqrt(K))
    em = _model(family, ys, m, off)
    lc = em.pointwise_constants
    lik = Likelihood('outcomes', ForwardModel(xs, POLYVAL), em)
    spy = _Spy(monkeypatch, SPIED)
    x = up(theta, device)
    lp = host(lik.log_prob(coefficients=x))
    assert spy.calls == ['poly_forward', 'glm_pointwise', 'row_sum'], spy.calls
    del spy.calls[:]
    gr = host(lik.gradient(coefficients=x))
    assert spy.calls == ['poly_forward', 'glm_pointwise', 'jacobian_contract'], spy.calls
    assert lp.shape == (C,) and gr.shape == (C, K) and np.all(np.isfinite(lp)) and np.all(np.isfinite(gr))
    A = PB.design(xs, K)
    eta = theta.dot(A) + off
    assert eta.min() < -30.0 and eta.max() > 30.0
    ex = G.ExactGLM(family, A, ys, m, off, roundings=2 * K)
    M = R.mp()
    for c in G.exact_chains(C, N):
        e = ex.chain(theta[c], 0.0)
        Bpe = G.pointwise_bound(e['B'], e['mag'], lc)
        total = M.fsum(e['ll']) + M.fsum(M.mpf(float(k)) for k in lc)
        s = G.err(lp[c], total) / float(G.rowsum_bound(Bpe, e['mag'], lc, N))
        j = max(G.err(a, w) / bd for a, w, bd in zip(gr[c], e['force'], e['force_bound']))
        assert s <= 1.0 and j <= 1.0, (c, s, j)
        _note('C4', 'rowsum', s)
        _note('C4', 'contract', j)
    _report()
