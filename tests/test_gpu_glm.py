"""Device tests of the generalised-linear kernels (csrc/glm.hip) and of the layers that carry
them: derived bounds against exact arithmetic (tests/glm_bounds.py), the order contracts bit
for bit, the refusals, the dispatch, stationarity against closed forms, and the LOO wiring.

The bound test runs over this module's own axes and over ``glm_bounds.force_cases()``, which
reaches every (KS, KV) x CT x family instantiation of the two dispatch tables
(``glm_bounds.table_row``: the tables restated on the host).  The edges of the term's range
(``glm_bounds.edge_case``, with its two Poisson rules: above eta = 700 only the per-datum bound,
beyond exp's overflow -inf / +inf exactly), non-finite coefficients, guard zones, the gradient's
order contract and the error models behind the polynomial forward model are in
tests/test_gpu_glm_range.py.

Largest measured fraction of the bound, as printed by the bound tests (MI355X): see DESIGN
section 4.7."""
import math

import numpy as np
import pytest
import torch
from scipy.special import polygamma, psi

import glm_bounds as G
import glm_ref as R
from binf_amd import _native, diagnostics, loo
from binf_amd.model import glm, linear
from binf_amd.model.glm import BinomialLogitErrorModel, PoissonLogErrorModel
from binf_amd.model.linear import LinearForwardModel
from binf_amd.pdf import IsotropicGaussian
from binf_amd.pdf.likelihoods import Likelihood
from binf_amd.pdf.posteriors import Posterior
from binf_amd.samplers import NUTSSampler
from binf_amd.samplers.hmc import HMCSampler
from binf_amd.samplers.rng import DeviceRNG

pytestmark = pytest.mark.gpu

K_AXIS = (1, 4, 5, 16, 17, 18, 33, 64)
N_AXIS = (1, 15, 16, 17, 1024, 1025, 2049)
C_AXIS = (1, 15, 17, 64, 65, 4096 + 17)


def _cases():
    """Every value of each axis at least once, and the corners K = 64 x N = 2049 and
    C = 4113 x N = 17."""
    cases = [(K, 17, 15) for K in K_AXIS] + [(5, N, 17) for N in N_AXIS] + \
        [(5, 17, C) for C in C_AXIS] + [(64, 2049, 17), (33, 17, 4113)]
    seen, out = set(), []
    for c in cases:
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


CASES = _cases()
FORCE_CASES = G.force_cases()
BOUND_CASES = CASES + [c for c in FORCE_CASES if c not in CASES]
worst = {}                     # largest error / bound seen by this module's bound tests, per part


def up(x, device):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(device)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int64)


def _model(family, ys, m, off):
    return BinomialLogitErrorModel(ys, m, off) if family == R.BINOMIAL_LOGIT else PoissonLogErrorModel(ys, off)


_exact_chains = G.exact_chains


def _note(part, key, value):
    worst[(part, key)] = max(worst.get((part, key), 0.0), float(value))


def test_bound_cases_reach_every_instantiation():
    """Every (KS, KV) row of glm_logp_dispatch / glm_grad_dispatch_k with one and with two chain
    tiles per wave, computed from (K, C) by the host restatement of the tables; the bound test
    below runs each case for both families."""
    reached = set((G.table_row(K), G.chain_tiles(C)) for K, N, C in BOUND_CASES)
    assert reached == set((row, ct) for row in G.TABLE_ROWS for ct in (1, 2)) and len(reached) == 26


# ---------------------------------------------------------------------------
# 1. bounds
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('family', R.FAMILIES)
@pytest.mark.parametrize('K,N,C', BOUND_CASES)
def test_fused_and_as_written_within_the_bound(device, family, K, N, C):
    """binf_linear_glm_logp_f64, binf_linear_glm_grad_f64 and the as-written path (forward,
    pointwise, row sum / Jacobian contraction) against the exact value within glm_bounds, with
    and without trials and offset.

    The cases: this module's axes (CASES), and ``glm_bounds.force_cases()``.  Of the latter,
    ``(K, 35, 19)`` and ``(K, 48, 19)`` launch the CT = 1 instantiation of K's row
    (``glm_bounds.table_row``) on a ragged and on a whole-tile N:
        K = 1, 4 -> (1, 0);  5, 8 -> (2, 0);  9, 16 -> (4, 0);  17 -> (4, 1);  18 -> (4, 2);
        19, 32 -> (8, 0);  33 -> (8, 1);  34 -> (8, 2);  35, 36 -> (9, 0);  37, 48 -> (12, 0);
        49 -> (12, 1);  50 -> (12, 2);  51, 64 -> (16, 0),
    and ``(K, 17, 4100)`` for K = 4, 8, 16, 17, 18, 32, 33, 34, 36, 48, 49, 50, 64 launches the
    CT = 2 instantiation of each row in that order.  A row that loses a coefficient leaves the
    bound by eleven orders of magnitude (tests/test_glm.py)."""
    part = 'A' if (K, N, C) in FORCE_CASES else 'axes'
    for extras in (True, False):
        A, ys, m, off, theta = G.case(family, K, N, C, 1000 * K + N + C + extras, trials=extras, offset=extras)
        em = _model(family, ys, m, off)
        ln, lc = em.log_norm, em.pointwise_constants
        dA, dth = up(A, device), up(theta, device)
        dy, dm, do, dlc = up(ys, device), up(m, device), up(off, device), up(lc, device)
        lp = _native.linear_glm_logp(dth, dA, dy, dm, do, family, ln).cpu().numpy()
        gr = _native.linear_glm_grad(dth, dA, dy, dm, do, family).cpu().numpy()
        mock = _native.linear_forward(dth, dA)
        ll_d, g_d = _native.glm_pointwise(mock, dy, dm, do, family, dlc, want_ll=True, want_grad=True)
        lp2 = _native.row_sum(ll_d).cpu().numpy()
        gr2 = _native.jacobian_contract(dA, g_d).cpu().numpy()
        ll_h = ll_d.cpu().numpy()
        assert np.all(np.isfinite(lp)) and np.all(np.isfinite(gr))

        # every chain: the float form of the bound around numpy's values
        f = G.float_case(family, theta, A, ys, m, off, ln)
        Bp = G.pointwise_bound(f['B'], f['mag'], lc)
        rb = G.rowsum_bound(Bp, f['mag'], lc, N)
        r = [np.max(np.abs(lp - f['lp']) / (2 * f['lp_bound'])),
             np.max(np.abs(gr - f['force']) / (2 * f['force_bound'])),
             np.max(np.abs(ll_h - (f['ll'] + lc)) / (2 * Bp)),
             np.max(np.abs(lp2 - np.sum(f['ll'] + lc, axis=1)) / (2 * rb)),
             np.max(np.abs(gr2 - f['force']) / (2 * f['force_bound']))]
        print('%s K=%d N=%d C=%d extras=%d float: logp %.3g grad %.3g pointwise %.3g rowsum %.3g contract %.3g'
              % (('binomial', 'poisson')[family], K, N, C, extras, *r))
        assert max(r) <= 1.0, r

        # the sampled chains: exact arithmetic carried through mpmath
        ex = G.ExactGLM(family, A, ys, m, off)
        M = R.mp()
        for c in _exact_chains(C, N):
            e = ex.chain(theta[c], ln)
            a = G.err(lp[c], e['lp']) / e['lp_bound']
            b = max(G.err(x, w) / bd for x, w, bd in zip(gr[c], e['force'], e['force_bound']))
            Bpe = G.pointwise_bound(e['B'], e['mag'], lc)
            p = max(G.err(x, w + M.mpf(float(k))) / bd for x, w, k, bd in zip(ll_h[c], e['ll'], lc, Bpe))
            total = M.fsum(e['ll']) + M.fsum(M.mpf(float(k)) for k in lc)
            s = G.err(lp2[c], total) / float(G.rowsum_bound(Bpe, e['mag'], lc, N))
            j = max(G.err(x, w) / bd for x, w, bd in zip(gr2[c], e['force'], e['force_bound']))
            for key, v in (('logp', a), ('grad', b), ('pointwise', p), ('rowsum', s), ('contract', j)):
                _note(part, key, v)
            assert max(a, b, p, s, j) <= 1.0, (c, a, b, p, s, j)
    print('largest fraction of the exact bound so far: %s'
          % ', '.join('%s/%s %.3f' % (k[0], k[1], v) for k, v in sorted(worst.items())))


# ---------------------------------------------------------------------------
# 2. order contracts, bit for bit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('family', R.FAMILIES)
@pytest.mark.parametrize('K,N', [(5, 2049), (33, 17), (64, 1025)])
def test_logp_of_a_chain_does_not_depend_on_its_batch(device, family, K, N):
    """Alone, in a batch of 17, in a batch of 4113, at any place in the batch: the same bits."""
    A, ys, m, off, theta = G.case(family, K, N, 4113, 77 + K)
    dA, dy, dm, do = up(A, device), up(ys, device), up(m, device), up(off, device)
    f = lambda th: _native.linear_glm_logp(up(th, device), dA, dy, dm, do, family, 0.75)
    whole = f(theta)
    for c in (0, 16, 4096, 4112):
        alone = f(theta[c:c + 1])
        assert torch.equal(bits(alone), bits(whole[c:c + 1])), c
        for place in (0, 5, 16):
            batch = np.roll(theta[:17], place, axis=0).copy()
            batch[place] = theta[c]
            assert torch.equal(bits(f(batch)[place:place + 1]), bits(alone)), (c, place)
    shard = f(theta[2000:3000])
    assert torch.equal(bits(shard), bits(whole[2000:3000]))


def test_short_or_missing_workspace_is_refused_and_out_untouched(device):
    L = _native.lib()
    K, N, C = 5, 2049, 17
    A, ys, m, off, theta = G.case(R.POISSON_LOG, K, N, C, 5)
    dA, dy, do, dth = up(A, device), up(ys, device), up(off, device), up(theta, device)
    st = _native.stream_handle(device)
    out = torch.full((C,), -7.25, dtype=torch.float64, device=device)
    need = L.binf_linear_glm_logp_workspace_bytes(C, K, N)
    ws = torch.zeros(need // 8, dtype=torch.float64, device=device)
    p = lambda t: t.data_ptr()
    for w, wb in ((None, need), (p(ws), need - 8), (None, 0)):
        rc = L.binf_linear_glm_logp_f64(p(dth), p(dA), p(dy), None, p(do), 1, 0.0, p(out), w, wb, C, K, N, st)
        assert rc == _native.E_ARG
    gout = torch.full((C, K), -7.25, dtype=torch.float64, device=device)
    gneed = L.binf_linear_glm_grad_workspace_bytes(C, K, N)
    gws = torch.zeros(gneed // 8, dtype=torch.float64, device=device)
    for w, wb in ((None, gneed), (p(gws), gneed - 8)):
        rc = L.binf_linear_glm_grad_f64(p(dth), p(dA), p(dy), None, p(do), 1, p(gout), w, wb, C, K, N, st)
        assert rc == _native.E_ARG
    q, mom = dth.clone(), torch.ones_like(dth)
    lneed = L.binf_linear_glm_leapfrog_workspace_bytes(C, K, N)
    rc = L.binf_linear_glm_leapfrog_f64(p(q), p(mom), p(dA), p(dy), None, p(do), 1, 0, 0.0, 0.0, p(gws),
                                        lneed - 8, C, K, N, 0.01, None, 2, 0, st)
    assert rc == _native.E_ARG
    torch.cuda.synchronize()
    assert bool((out == -7.25).all()) and bool((gout == -7.25).all())
    assert torch.equal(q, dth) and bool((mom == 1.0).all())
    # with the workspace the same call goes through
    rc = L.binf_linear_glm_logp_f64(p(dth), p(dA), p(dy), None, p(do), 1, 0.0, p(out), p(ws), need, C, K, N, st)
    assert rc == 0 and bool(torch.isfinite(out).all())


def _posterior(family, A, ys, m, off, prior):
    fwm = LinearForwardModel('covariates', A)
    lik = Likelihood('outcomes', fwm, _model(family, ys, m, off))
    priors = {'prior': IsotropicGaussian(prior[0], prior[1], name='prior', variable_name='coefficients')} \
        if prior else {}
    return Posterior({'outcomes': lik}, priors)


def _leapfrog_both_ways(device, family, K, N, C, priors, steps):
    _, ys, m, off, _ = G.case(family, K, N, C, 31 + K)
    rs = np.random.RandomState(K + N)
    A = rs.standard_normal((K, N))         # a gentle design and moderate eta: trajectories that stay finite
    theta = 0.3 * rs.standard_normal((C, K)) / math.sqrt(K)
    p0 = rs.standard_normal((C, K))
    dts = [1e-3, up(rs.uniform(5e-4, 2e-3, size=C), device)]
    for prior in priors:
        post = _posterior(family, A, ys, m, off, prior)
        for mode in ('exact', 'fma'):
            for nsteps in steps:
                dt = dts[nsteps % 2]
                res = []
                for fused in (True, False):
                    s = HMCSampler(post, up(theta, device), 1e-3, nsteps, variable_name='coefficients', mode=mode)
                    s.fused_leapfrog = fused
                    q, p = up(theta, device), up(p0, device)
                    s._leapfrog(q, p, dt, nsteps)
                    res.append((q, p))
                (qf, pf), (qs, ps) = res
                assert bool(torch.isfinite(qf).all()) and not torch.equal(qf, up(theta, device))
                assert torch.equal(bits(qf), bits(qs)) and torch.equal(bits(pf), bits(ps)), (prior, mode, nsteps)


@pytest.mark.parametrize('family', R.FAMILIES)
@pytest.mark.parametrize('K,N,C', [(5, 35, 17), (33, 1025, 19), (18, 272, 4100)])
def test_fused_leapfrog_equals_the_per_step_sequence(device, family, K, N, C):
    """binf_linear_glm_leapfrog_f64 against HMCSampler._leapfrog with the fused leapfrog
    disabled (the GLM gradient, Posterior.gradient's sum, kick and drift): the same bits at
    nsteps 1, 2, 7, EXACT and FMA, with and without the prior, with a per-chain dt."""
    _leapfrog_both_ways(device, family, K, N, C, (None, (0.7, 0.25)), (1, 2, 7))


@pytest.mark.parametrize('family', R.FAMILIES)
@pytest.mark.parametrize('K', G.ROW_KS)
def test_fused_leapfrog_equals_the_per_step_sequence_on_every_row(device, family, K):
    """The same on ``(K, 35, 19)`` for one K per row of the gradient's dispatch table: EXACT and
    FMA, with the prior, nsteps = 2."""
    _leapfrog_both_ways(device, family, K, 35, 19, ((0.7, 0.25),), (2,))


# ---------------------------------------------------------------------------
# 3. refusals, through _native
# ---------------------------------------------------------------------------
def test_refusals_through_native(device):
    A, ys, m, off, theta = G.case(R.BINOMIAL_LOGIT, 3, 20, 4, 9)
    dA, dy, dm, do, dth = (up(x, device) for x in (A, ys, m, off, theta))
    with pytest.raises(ValueError):
        _native.linear_glm_logp(dth, dA, dy, dm, do, 2, 0.0)                    # bad family
    with pytest.raises(ValueError):
        _native.linear_glm_grad(dth, dA, dy, dm, do, -1)
    with pytest.raises(ValueError):
        _native.linear_glm_leapfrog(dth.clone(), dth.clone(), dA, dy, dm, do, 7, None, 0.1, None, 2)
    with pytest.raises(ValueError):
        _native.linear_glm_leapfrog(dth.clone(), dth.clone(), dA, dy, dm, do, 0, None, 0.1, None, 0)   # nsteps
    with pytest.raises(ValueError):
        _native.linear_glm_leapfrog(dth.clone(), dth.clone(), dA, dy, dm, do, 0, None, 0.1, None, 2, mode=5)
    q = dth.clone()
    with pytest.raises(ValueError):
        _native.linear_glm_leapfrog(q, q, dA, dy, dm, do, 0, None, 0.1, None, 2)                    # BINF_E_ALIAS
    with pytest.raises(ValueError):
        _native.glm_pointwise(dth, dy, dm, do, 0)                                # shapes disagree
    mock = _native.linear_forward(dth, dA)
    with pytest.raises(ValueError):
        _native.glm_pointwise(mock, dy, dm, do, 0, want_ll=False, want_grad=False)  # no output
    with pytest.raises(ValueError):
        _native.glm_pointwise(mock, dy, dm, do, 3)
    big = torch.zeros((4, 65), dtype=torch.float64, device=device)
    bigA = torch.zeros((65, 20), dtype=torch.float64, device=device)
    for call in (lambda: _native.linear_glm_logp(big, bigA, dy, dm, do, 0, 0.0),
                 lambda: _native.linear_glm_grad(big, bigA, dy, dm, do, 0),
                 lambda: _native.linear_glm_leapfrog(big, big.clone(), bigA, dy, dm, do, 0, None, 0.1, None, 2)):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(ValueError):
        _native.linear_glm_logp(dth, dA[:, :19].contiguous(), dy, dm, do, 0, 0.0)   # design shape


# ---------------------------------------------------------------------------
# 4. dispatch
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


SPIED = ('linear_glm_logp', 'linear_glm_grad', 'linear_glm_leapfrog', 'glm_pointwise', 'linear_forward',
         'jacobian_contract', 'poly_leapfrog', 'linear_gauss_logp')


@pytest.mark.parametrize('family', R.FAMILIES)
def test_dispatch(device, monkeypatch, family):
    A, ys, m, off, theta = G.case(family, 5, 40, 9, 3)
    theta = theta * 0.05
    x = up(theta, device)
    spy = _Spy(monkeypatch, SPIED)
    post = _posterior(family, A, ys, m, off, None)
    lik = post.likelihoods['outcomes']
    kind = lik.error_model.kind
    # 9 chains x 40 points is one workgroup: the log-prob hook declines (the as-written path is
    # the faster launch there); the gradient hook does not
    assert not glm.logp_covers(kind, 9, 40)
    lp = lik.log_prob(coefficients=x)
    assert spy.calls == ['linear_forward', 'glm_pointwise'] and lp.shape == (9,)
    del spy.calls[:]
    g = lik.gradient(coefficients=x)
    assert spy.calls == ['linear_glm_grad'] and g.shape == x.shape
    one = lik.gradient(coefficients=x[0])
    assert one.shape == (5,) and torch.equal(bits(one), bits(g[0]))

    # a subclass overriding _evaluate: the models as written
    class Mine(LinearForwardModel):
        def _evaluate(self, **variables):
            return LinearForwardModel._evaluate(self, **variables)

    del spy.calls[:]
    written = Likelihood('outcomes', Mine('covariates', A), _model(family, ys, m, off))
    lp_w = written.log_prob(coefficients=x)
    assert spy.calls == ['linear_forward', 'glm_pointwise'] and torch.equal(bits(lp_w), bits(lp))
    del spy.calls[:]
    g_w = written.gradient(coefficients=x)
    assert spy.calls == ['linear_forward', 'glm_pointwise', 'jacobian_contract']
    f = G.float_case(family, theta, A, ys, m, off, lik.error_model.log_norm)
    assert np.all(np.abs((g - g_w).cpu().numpy()) <= 4 * f['force_bound'])

    # a shape that fills the chip (8 pieces x 32 workgroups): the fused log-prob
    Cb, Nb = 4096, 8192
    assert glm.logp_covers(kind, Cb, Nb) and not glm.logp_covers(kind, Cb, 1024)
    Ab, yb, mb, ob, tb = G.case(family, 5, Nb, Cb, 4)
    tb = tb * 0.05
    xb = up(tb, device)
    big = Likelihood('outcomes', LinearForwardModel('covariates', Ab), _model(family, yb, mb, ob))
    del spy.calls[:]
    lp_b = big.log_prob(coefficients=xb)
    assert spy.calls == ['linear_glm_logp'] and lp_b.shape == (Cb,)
    del spy.calls[:]
    lp_bw = Likelihood('outcomes', Mine('covariates', Ab), _model(family, yb, mb, ob)).log_prob(coefficients=xb[:64])
    assert spy.calls == ['linear_forward', 'glm_pointwise']
    em = big.error_model
    fb = G.float_case(family, tb[:64], Ab, yb, mb, ob, em.log_norm)
    lc = em.pointwise_constants
    rb = G.rowsum_bound(G.pointwise_bound(fb['B'], fb['mag'], lc), fb['mag'], lc, Nb)
    assert np.all(np.abs((lp_b[:64] - lp_bw).cpu().numpy()) <= 2 * fb['lp_bound'] + 2 * rb + G.U * abs(em.log_norm))

    # the leapfrog: fused for the matched posterior, per step with a second differentiable component
    for prior in (None, (0.5, 0.0)):
        del spy.calls[:]
        s = HMCSampler(_posterior(family, A, ys, m, off, prior), x.clone(), 1e-3, 3, variable_name='coefficients')
        s._leapfrog(x.clone(), torch.ones_like(x), 1e-3, 3)
        assert spy.calls == ['linear_glm_leapfrog'], (prior, spy.calls)
    fwm = LinearForwardModel('covariates', A)
    two = Posterior({'outcomes': Likelihood('outcomes', fwm, _model(family, ys, m, off))},
                    {'a': IsotropicGaussian(0.5, 0.0, name='a', variable_name='coefficients'),
                     'b': IsotropicGaussian(0.25, 1.0, name='b', variable_name='coefficients')})
    del spy.calls[:]
    s = HMCSampler(two, x.clone(), 1e-3, 3, variable_name='coefficients')
    s._leapfrog(x.clone(), torch.ones_like(x), 1e-3, 3)
    assert spy.calls == ['linear_glm_grad'] * 4
    # resident=True with a GLM error model behaves as without the flag
    res = Posterior({'outcomes': Likelihood('outcomes', LinearForwardModel('covariates', A, resident=True),
                                            _model(family, ys, m, off))}, {})
    assert res.native_hmc_spec('coefficients') is None
    assert res.native_leapfrog_spec('coefficients')[0] == 'linear_glm'


# ---------------------------------------------------------------------------
# 5. stationarity against closed forms
# ---------------------------------------------------------------------------
N_OBS, CHAINS, N_WARM, N_KEEP, SEED = 24, 512, 150, 200, 20240


def _closed_form(family):
    rs = np.random.RandomState(SEED)
    if family == R.POISSON_LOG:
        ys = rs.poisson(3.0, size=N_OBS).astype(np.float64)
        s = float(ys.sum())
        # exp(theta) ~ Gamma(sum y, N): E theta = psi(sum y) - ln N, Var theta = psi_1(sum y)
        return ys, float(psi(s)) - math.log(N_OBS), float(polygamma(1, s))
    ys = (rs.uniform(size=N_OBS) < 0.4).astype(np.float64)
    s = float(ys.sum())
    assert 0 < s < N_OBS
    # logistic(theta) ~ Beta(s, N - s) under the flat prior on theta
    return ys, float(psi(s) - psi(N_OBS - s)), float(polygamma(1, s) + polygamma(1, N_OBS - s))


class _HostPDF(object):
    """The same intercept-only model as a user's torch PDF, with the error term's gradient
    multiplied by ``sign`` (-1: the sign error the margin must see)."""

    def __init__(self, family, ys, sign):
        self.family, self.ys, self.sign = family, ys, sign

    def _eta(self, coefficients):
        return coefficients.reshape(-1, 1).expand(-1, self.ys.shape[0])

    def log_prob(self, coefficients):
        eta = self._eta(coefficients)
        if self.family == R.POISSON_LOG:
            return (self.ys * eta - torch.exp(eta)).sum(dim=1)
        return (self.ys * eta - torch.nn.functional.softplus(eta)).sum(dim=1)

    def gradient(self, coefficients):
        eta = self._eta(coefficients)
        g = torch.exp(eta) - self.ys if self.family == R.POISSON_LOG else torch.sigmoid(eta) - self.ys
        return self.sign * g.sum(dim=1, keepdim=True)


def _stationarity(device, family, sampler, pdf=None):
    """``(passes, figures)`` of the check on one run."""
    ys, mean, var = _closed_form(family)
    sd = math.sqrt(var)
    rs = np.random.RandomState(SEED + 1)
    q0 = up(mean + sd * (1.0 + rs.standard_normal((CHAINS, 1))), device)      # started one sd off
    if pdf is None:
        pdf = _posterior(family, np.ones((1, N_OBS)), ys, None, None, None)
    rng = DeviceRNG(SEED, device)
    if sampler == 'hmc':
        s = HMCSampler(pdf, q0, 0.375 * sd, 4, variable_name='coefficients', rng=rng)
    else:
        # In one dimension a NUTS draw is positively correlated with the last one at small steps
        # (the host restatement tests/nuts_ref.py on the same targets: lag-1 autocorrelation 0.57
        # and split-R^ 1.0135 over 2 x 100 draws at 0.5 sd, 0.30 and 1.004 ... 1.006 at 1.5 sd,
        # three seeds, both families), so the step is 1.5 sd -- a setting of the run, not of the check.
        s = NUTSSampler(pdf, q0, 1.5 * sd, max_tree_depth=5, variable_name='coefficients', rng=rng)
    s.sample_n(N_WARM, record=False)
    kept = s.sample_n(N_KEEP)
    centred = kept - kept.mean()
    both = torch.cat((kept, centred * centred), dim=2).contiguous()
    d = diagnostics.summary(both).cpu()
    fig = dict(mean=float(d.mean[0]), want_mean=mean, mcse=float(d.mcse[0]), var=float(d.mean[1]), want_var=var,
               var_se=float(d.mcse[1]), rhat=float(d.rhat[0]))
    ok = abs(fig['mean'] - mean) <= 5 * fig['mcse'] and abs(fig['var'] - var) <= 5 * fig['var_se'] and \
        fig['rhat'] < 1.01 and all(math.isfinite(v) for v in fig.values())
    return ok, fig, s


@pytest.mark.parametrize('sampler', ['hmc', 'nuts'])
@pytest.mark.parametrize('family', R.FAMILIES)
def test_stationarity_against_closed_forms(device, monkeypatch, family, sampler):
    """Intercept-only design, no prior: the posterior of the intercept is known in closed form.
    512 chains, 150 + 200 transitions, one seed: the mean within 5 MCSE, the pooled variance
    within 5 of its standard errors (ESS of the squared deviations), split-R^ < 1.01."""
    spy = _Spy(monkeypatch, ('linear_glm_leapfrog', 'linear_glm_grad', 'linear_glm_logp'))
    ok, fig, _ = _stationarity(device, family, sampler)
    print(sampler, ('binomial', 'poisson')[family], fig)
    assert ok, fig
    assert ('linear_glm_leapfrog' if sampler == 'hmc' else 'linear_glm_grad') in spy.calls


@pytest.mark.parametrize('family', R.FAMILIES)
def test_the_margin_sees_a_flipped_sign(device, family):
    """The same check on a host-side torch PDF: passes as written, fails with the error term's
    gradient flipped.  No kernel is mutated.  (The accept step still uses the right log-prob, so
    a flipped force leaves the target invariant -- the mean stays -- but nearly every proposal
    climbs in energy and is refused: the chains hardly move, and split-R^ reads 1.15 ... 1.19
    against the 1.01 allowed, the variance several of its standard errors off.)"""
    ys, _, _ = _closed_form(family)
    y = up(ys, device)
    ok, fig, _ = _stationarity(device, family, 'hmc', _HostPDF(family, y, 1.0))
    assert ok, fig
    bad, fig, _ = _stationarity(device, family, 'hmc', _HostPDF(family, y, -1.0))
    print('flipped', fig)
    assert not bad, fig


# ---------------------------------------------------------------------------
# 6. LOO wiring
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('family', R.FAMILIES)
def test_loo_wiring(device, family):
    S, K, N = 200, 4, 17
    A, ys, m, off, theta = G.case(family, K, N, S, 41)
    theta = theta * 0.02
    lik = _posterior(family, A, ys, m, off, None).likelihoods['outcomes']
    em = lik.error_model
    x = up(theta, device)
    rec = loo.pointwise_log_likelihood(lik, x)
    assert rec.shape == (S, N)
    assert torch.equal(bits(rec), bits(loo.pointwise_log_likelihood(lik, (x, torch.ones(S, dtype=torch.float64, device=device)))))
    f = G.float_case(family, theta, A, ys, m, off, em.log_norm)
    lc = em.pointwise_constants
    Bp = G.pointwise_bound(f['B'], f['mag'], lc)
    assert np.all(np.abs(rec.cpu().numpy() - (f['ll'] + lc)) <= 2 * Bp)
    # its sums over the observations are the likelihood's log-prob
    lp = lik.log_prob(coefficients=x).cpu().numpy()
    sums = rec.cpu().numpy().sum(axis=1)
    # (log_norm is the correctly rounded sum of the constants: one more u of it)
    allow = 2 * f['lp_bound'] + 2 * G.rowsum_bound(Bp, f['mag'], lc, N) + G.U * abs(em.log_norm)
    assert np.all(np.abs(sums - lp) <= allow)
    r = loo.loo(rec)
    assert math.isfinite(r.elpd) and bool(torch.isfinite(r.khat).all()) and bool(torch.isfinite(r.elpd_i).all())

    class Other(glm._GLMErrorModel):
        kind = 'probit'

        def _constants(self):
            return np.zeros_like(self._ys)

        def native_spec(self):
            return None

    with pytest.raises(TypeError):
        loo.pointwise_log_likelihood(Likelihood('o', LinearForwardModel('c', A), Other(ys)), x)


# ---------------------------------------------------------------------------
# 7. per-step consumers reach the hooks with no change of their own
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('family', R.FAMILIES)
def test_graph_replay_of_the_per_step_tier_equals_eager(device, family):
    """``HMCSampler(graph=True)`` on a posterior with two priors (no fused leapfrog: the
    transition is energies, gradient calls, kicks, drifts and the accept, captured once): the
    same bits as the eager launches, rejections included."""
    K, N, C, L, n = 4, 50, 33, 3, 6
    _, ys, m, off, _ = G.case(family, K, N, C, 17)
    rs = np.random.RandomState(8)
    A = rs.standard_normal((K, N))
    q0 = 0.3 * rs.standard_normal((C, K))
    draws = [(rs.standard_normal((C, K)), rs.uniform(size=C)) for _ in range(n)]

    def run(graph):
        post = Posterior({'outcomes': Likelihood('outcomes', LinearForwardModel('covariates', A), _model(family, ys, m, off))},
                         {'a': IsotropicGaussian(0.5, 0.0, name='a', variable_name='coefficients'),
                          'b': IsotropicGaussian(0.25, 1.0, name='b', variable_name='coefficients')})
        s = HMCSampler(post, up(q0, device), 0.05, L, variable_name='coefficients', graph=graph)
        return s, [s.sample(p0=up(p, device), u=up(u, device)).clone() for p, u in draws]

    se, eager = run(False)
    sg, graph = run('always')
    assert len(sg._graphs) == 1 and not se._graphs
    for a, b in zip(eager, graph):
        assert torch.equal(bits(a), bits(b))
    assert torch.equal(se.n_accepted, sg.n_accepted)
    assert 0 < int(sg.n_accepted.sum()) < n * C
