"""Device tests of the negative-binomial family (csrc/glm_term.hpp, csrc/glm.hip, csrc/negbin.hip)
and of the layers that carry it: derived bounds against exact arithmetic (tests/negbin_bounds.py),
the order contracts bit for bit, the count term, the edges of z and of lam, the refusals, the
dispatch and the stationarity of the coefficients against a closed form.

Largest measured fractions of the bounds, as printed by the bound tests (MI355X): DESIGN
section 4.7."""
import math

import numpy as np
import pytest
import torch
from scipy.special import polygamma, psi

import glm_bounds as G
import glm_ref as R
import negbin_bounds as NB
import negbin_ref as NR
from binf_amd import _native, diagnostics
from binf_amd.model import glm
from binf_amd.model.glm import NegBinomialLogErrorModel
from binf_amd.model.linear import LinearForwardModel
from binf_amd.pdf import IsotropicGaussian
from binf_amd.pdf.likelihoods import Likelihood
from binf_amd.pdf.posteriors import Posterior
from binf_amd.samplers import NUTSSampler
from binf_amd.samplers.hmc import HMCSampler
from binf_amd.samplers.rng import DeviceRNG

pytestmark = pytest.mark.gpu

ONE_K = 5
FORCE_CASES = G.force_cases()
BOUND_CASES = FORCE_CASES + [(K, N, C) for K in G.ROW_KS for N, C in ((35, 19), (48, 19), (17, 4100))
                             if (K, N, C) not in FORCE_CASES] + [(ONE_K, N, 17) for N in (1, 1025, 2049)]
worst = {}


def up(x, device):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(device)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int64)


def _note(key, value):
    worst[key] = max(worst.get(key, 0.0), float(value))


def _count_inputs(em, device):
    return em.tail_device(device), em.values_device(device), em.index_device(device)


def test_bound_cases_reach_every_instantiation():
    reached = set((G.table_row(K), G.chain_tiles(C)) for K, N, C in BOUND_CASES)
    assert reached == set((row, ct) for row in G.TABLE_ROWS for ct in (1, 2)) and len(reached) == 26


# ---------------------------------------------------------------------------
# 1. bounds
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('K,N,C', BOUND_CASES)
def test_fused_and_as_written_within_the_bound(device, K, N, C):
    """binf_linear_negbin_logp_f64, binf_linear_negbin_grad_f64, the record
    (binf_negbin_pointwise_f64 with the prefix and the constants), its row sum and the as-written
    contraction against the exact value within negbin_bounds; lam spread over [-20, 20] across the
    chains, counts with a 0 and a maximum of 300 (N = 1: the single count is 0)."""
    A, ys, off, theta, lam = NB.case(K, N, C, 1000 * K + N + C)
    assert ys.min() == 0.0 and (N == 1 or ys.max() == 300.0)
    assert C == 1 or (lam.min() == -20.0 and lam.max() == 20.0)
    em = NegBinomialLogErrorModel(ys, off)
    ln, lc = em.log_norm, em.pointwise_constants
    dA, dth, dy, do, dl, dlc = (up(v, device) for v in (A, theta, ys, off, lam, lc))
    dtail, dval, didx = _count_inputs(em, device)
    lnc_d, pre_d = _native.negbin_count_term(dl, dtail, ln, values=dval)
    lp = _native.linear_negbin_logp(dth, dA, dy, do, dl, lnc_d).cpu().numpy()
    gr = _native.linear_negbin_grad(dth, dA, dy, do, dl).cpu().numpy()
    mock = _native.linear_forward(dth, dA)
    ll_d, g_d = _native.negbin_pointwise(mock, dy, do, dl, pre_d, didx, dlc, want_ll=True, want_grad=True)
    lp2 = _native.row_sum(ll_d).cpu().numpy()
    gr2 = _native.jacobian_contract(dA, g_d).cpu().numpy()
    ll_h = ll_d.cpu().numpy()
    assert np.all(np.isfinite(lp)) and np.all(np.isfinite(gr))
    # the model's own as-written path is this sequence
    assert torch.equal(bits(em.pointwise_log_prob(mock, dl)), bits(ll_d))

    # every chain: the float form around numpy's values
    f = NB.float_case(theta, A, ys, off, lam, ln)
    values, index = em.count_values, em._index
    pre = NR.prefix(lam, values)
    pb, pm = NB.prefix_bounds(lam, values)                       # [C x J]: bound, |P| limit
    rec = (f['ll'] + pre[:, index]) + lc
    r = [np.max(np.abs(lp - f['lp']) / (2 * f['lp_bound'])),
         np.max(np.abs(gr - f['force']) / (2 * f['force_bound'])),
         np.max(np.abs(gr2 - f['force']) / (2 * f['force_bound']))]
    Bp = NB.record_bound(f['B'], f['mag'], pb[:, index], pm[:, index], lc)
    r.append(np.max(np.abs(ll_h - rec) / (2 * Bp)))
    rb = G.rowsum_bound(Bp, f['mag'] + pm[:, index], lc, N)
    r.append(np.max(np.abs(lp2 - np.sum(rec, axis=1)) / (2 * rb)))
    print('K=%d N=%d C=%d float: logp %.3g grad %.3g contract %.3g pointwise %.3g rowsum %.3g' % (K, N, C, *r))
    assert max(r) <= 1.0, r

    # the sampled chains: exact arithmetic carried through mpmath
    ex = NB.ExactNB(A, ys, off)
    M = R.mp()
    for c in G.exact_chains(C, N):
        e = ex.chain(theta[c], lam[c], ln)
        a = G.err(lp[c], e['lp']) / e['lp_bound']
        b = max(G.err(x, w) / bd for x, w, bd in zip(gr[c], e['force'], e['force_bound']))
        j = max(G.err(x, w) / bd for x, w, bd in zip(gr2[c], e['force'], e['force_bound']))
        pbe = np.array([NB.prefix_bound(lam[c], v) for v in values])
        pe = [NR.exact_prefix(lam[c], v) for v in values]
        Bpe = NB.record_bound(e['B'], e['mag'], pbe[index, 0], pbe[index, 1], lc)
        exact_rec = [w + pe[k] + M.mpf(float(x)) for w, k, x in zip(e['ll'], index, lc)]
        p = max(G.err(x, w) / bd for x, w, bd in zip(ll_h[c], exact_rec, Bpe))
        s = G.err(lp2[c], M.fsum(exact_rec)) / float(G.rowsum_bound(Bpe, e['mag'] + pbe[index, 1], lc, N))
        for key, v in (('logp', a), ('grad', b), ('pointwise', p), ('rowsum', s), ('contract', j)):
            _note(key, v)
        assert max(a, b, p, s, j) <= 1.0, (c, a, b, p, s, j)
    print('largest fraction of the exact bound so far: %s'
          % ', '.join('%s %.3f' % (k, v) for k, v in sorted(worst.items())))


# ---------------------------------------------------------------------------
# 2. order contracts, bit for bit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('K,N', [(5, 2049), (33, 17), (64, 1025)])
def test_logp_of_a_chain_does_not_depend_on_its_batch(device, K, N):
    """Alone, among 17, among 4113, at either end of the batch: the same bits (count term too)."""
    A, ys, off, theta, lam = NB.case(K, N, 4113, 77 + K)
    em = NegBinomialLogErrorModel(ys, off)
    dA, dy, do = up(A, device), up(ys, device), up(off, device)
    dtail = em.tail_device(device)

    def f(th, lm):
        dl = up(lm, device)
        lnc = _native.negbin_count_term(dl, dtail, em.log_norm)[0]
        return _native.linear_negbin_logp(up(th, device), dA, dy, do, dl, lnc)
    whole = f(theta, lam)
    for c in (0, 16, 4096, 4112):
        alone = f(theta[c:c + 1], lam[c:c + 1])
        assert torch.equal(bits(alone), bits(whole[c:c + 1])), c
        for place in (0, 5, 16):
            batch, bl = np.roll(theta[:17], place, axis=0).copy(), np.roll(lam[:17], place).copy()
            batch[place], bl[place] = theta[c], lam[c]
            assert torch.equal(bits(f(batch, bl)[place:place + 1]), bits(alone)), (c, place)
    shard = f(theta[2000:3000], lam[2000:3000])
    assert torch.equal(bits(shard), bits(whole[2000:3000]))


def _posterior(A, ys, off, prior, lam=None):
    em = NegBinomialLogErrorModel(ys, off)
    if lam is not None:
        em.fix_variables(log_dispersion=lam)
    lik = Likelihood('outcomes', LinearForwardModel('covariates', A), em)
    priors = {'prior': IsotropicGaussian(prior[0], prior[1], name='prior', variable_name='coefficients')} \
        if prior else {}
    return Posterior({'outcomes': lik}, priors)


@pytest.mark.parametrize('K,N,C', [(5, 35, 17), (33, 1025, 19), (18, 272, 4100)])
def test_fused_leapfrog_equals_the_per_step_sequence(device, K, N, C):
    """binf_linear_negbin_leapfrog_f64 against HMCSampler._leapfrog with the fused leapfrog
    disabled: the same bits at nsteps 1, 2, 7, EXACT and FMA, with and without the prior, with a
    per-chain dt and a per-chain lam."""
    _, ys, off, _, lam = NB.case(K, N, C, 31 + K)
    lam = lam / 10.0                       # phi in [e**-2, e**2]: trajectories that stay finite
    rs = np.random.RandomState(K + N)
    A = rs.standard_normal((K, N))
    theta = 0.3 * rs.standard_normal((C, K)) / math.sqrt(K)
    p0 = rs.standard_normal((C, K))
    dts = [1e-3, up(rs.uniform(5e-4, 2e-3, size=C), device)]
    for prior in (None, (0.7, 0.25)):
        post = _posterior(A, ys, off, prior, up(lam, device))
        assert post.native_leapfrog_spec('coefficients')[0] == 'linear_glm'
        for mode in ('exact', 'fma'):
            for nsteps in (1, 2, 7):
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


# ---------------------------------------------------------------------------
# 3. the count term
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('ymax', [0, 1, 63, 64, 65, 4097])
def test_count_term_within_the_bound(device, ymax):
    """The device against the restatement's order within twice the float bound and against the
    exact sum within the bound, for lam in {-30, 0, 30}; both outputs."""
    rs = np.random.RandomState(ymax)
    ys = np.concatenate([rs.randint(0, ymax + 1, size=37), [0, ymax]]).astype(np.float64)
    em = NegBinomialLogErrorModel(ys)
    assert em.tail_counts.shape[0] == ymax
    lam = np.array([-30.0, 0.0, 30.0])
    dl = up(lam, device)
    chain, pre = _native.negbin_count_term(dl, em.tail_device(device), em.log_norm,
                                           values=em.values_device(device))
    chain, pre = chain.cpu().numpy(), pre.cpu().numpy()
    want = NR.count_term(lam, em.tail_counts, em.log_norm)
    wpre = NR.prefix(lam, em.count_values)
    M = R.mp()
    for c, l in enumerate(lam):
        cb = NB.count_bound(l, em.tail_counts, em.log_norm)
        a = abs(chain[c] - want[c])
        b = G.err(chain[c], NR.exact_count(l, em.tail_counts) + M.mpf(em.log_norm))
        assert a <= 2 * cb and b <= cb, (ymax, l, a, b, cb)         # ymax = 0: exactly log_norm = 0
        if cb > 0.0:
            _note('count', b / cb)
        for k in sorted(set([0, len(em.count_values) // 2, len(em.count_values) - 1])):
            v = em.count_values[k]
            bound = NB.prefix_bound(l, v)[0]
            if v == 0:
                assert pre[c, k] == 0.0
                continue
            p = G.err(pre[c, k], NR.exact_prefix(l, v)) / bound
            assert p <= 1.0 and abs(pre[c, k] - wpre[c, k]) <= 2 * bound, (ymax, l, v, p)
            _note('prefix', p)
    print('count term ymax=%d: %s' % (ymax, ', '.join('%s %.3f' % kv for kv in sorted(worst.items()))))


def test_count_term_of_all_zero_counts_is_log_norm(device):
    em = NegBinomialLogErrorModel(np.zeros(9))
    assert em.tail_counts.shape == (0,) and em.log_norm == 0.0
    lam = up(np.array([-30.0, 0.0, 30.0, 709.0]), device)
    for ln in (0.0, -12.625):
        out = _native.negbin_count_term(lam, None, ln)[0]
        assert torch.equal(bits(out), bits(torch.full((4,), ln, dtype=torch.float64)))


# ---------------------------------------------------------------------------
# 4. edges
# ---------------------------------------------------------------------------
def test_edge_ladder_on_z(device):
    """glm_bounds.edge_ladder() put exactly into z: lam = 0 (phi = 1, z = eta - 0 exactly), K = 1,
    design entries 1, 2, 4, 8, counts 0, 1, 20.  Every datum of the element-wise kernel within the
    term's bound at delta = 0, finite; every chain of the fused kernels within the exact bound."""
    A, _, _, _, theta = G.edge_case(R.BINOMIAL_LOGIT, 1)
    n = np.arange(G.EDGE_N)
    ys = np.array([0.0, 1.0, 20.0])[n % 3]
    C = theta.shape[0]
    lam = np.zeros(C)
    eta = G.edge_eta((A, ys, None, None, theta))
    dl, dy = up(lam, device), up(ys, device)
    mock = up(eta, device)
    assert G._same_bits(mock.cpu().numpy(), eta)
    ll, g = _native.negbin_pointwise(mock, dy, None, dl, want_ll=True, want_grad=True)
    ll, g = ll.cpu().numpy(), g.cpu().numpy()
    assert np.all(np.isfinite(ll)) and np.all(np.isfinite(g))
    with np.errstate(over='ignore', invalid='ignore'):
        Bp, rho, _, _ = NB.term_bounds(eta, 0.0, ys[None, :], 0.0)
    assert np.all(np.isfinite(Bp)) and np.all(np.isfinite(rho))
    for c in range(C):
        for k in range(G.EDGE_N):
            a = G.err(ll[c, k], NR.exact_ll(float(eta[c, k]), ys[k], 0.0)) / Bp[c, k]
            b = G.err(g[c, k], NR.exact_g(float(eta[c, k]), ys[k], 0.0)) / rho[c, k]
            assert a <= 1.0 and b <= 1.0, (c, k, float(eta[c, k]), a, b)
            _note('edge ll', a), _note('edge g', b)
            if eta[c, k] == 0.0:                  # z = +-0: g = m / 2 - y exactly
                assert g[c, k] == (ys[k] + 1.0) / 2.0 - ys[k]
    em = NegBinomialLogErrorModel(ys)
    lnc = _native.negbin_count_term(dl, em.tail_device(device), em.log_norm)[0]
    dA, dth = up(A, device), up(theta, device)
    lp = _native.linear_negbin_logp(dth, dA, dy, None, dl, lnc).cpu().numpy()
    gr = _native.linear_negbin_grad(dth, dA, dy, None, dl).cpu().numpy()
    assert np.all(np.isfinite(lp)) and np.all(np.isfinite(gr))
    ex = NB.ExactNB(A, ys, None)
    for c in range(C):
        e = ex.chain(theta[c], 0.0, em.log_norm)
        assert np.isfinite(e['lp_bound']) and np.all(np.isfinite(e['force_bound'])), c
        a = G.err(lp[c], e['lp']) / e['lp_bound']
        b = max(G.err(x, w) / bd for x, w, bd in zip(gr[c], e['force'], e['force_bound']))
        assert a <= 1.0 and b <= 1.0, (c, float(theta[c, 0]), a, b)
    print('edges: %s' % ', '.join('%s %.3f' % kv for kv in sorted(worst.items())))


LAM_INSIDE = (NR.LAM_MIN, NR.LAM_MAX)
LAM_OUTSIDE = (float(np.nextafter(NR.LAM_MIN, -np.inf)), float(np.nextafter(NR.LAM_MAX, np.inf)),
               -745.2, 709.8, -1e300, 1e300, -np.inf, np.inf, np.nan)


def test_lam_at_the_ends_of_the_regular_range_and_outside(device):
    """-708 <= lam <= 709 is regular: finite log-prob at both ends, inside the exact bound.  Just
    outside (the neighbouring doubles), where exp gives 0 or inf, at +-inf and NaN: the log-prob,
    the count term and the record are -inf, the gradient and the leapfrog hold no NaN, and the
    other chains of the launch keep their bits."""
    K, N = 5, 35
    A, ys, off, theta, _ = NB.case(K, N, 19, 9)
    theta = theta * 0.05
    em = NegBinomialLogErrorModel(ys, off)
    lam = np.linspace(-3.0, 3.0, 19)
    clean = lam.copy()
    lam[1], lam[17] = LAM_INSIDE
    for k, v in enumerate(LAM_OUTSIDE):
        lam[3 + k] = v
    out_idx = list(range(3, 3 + len(LAM_OUTSIDE)))
    keep = [c for c in range(19) if c not in out_idx and c not in (1, 17)]
    dA, dy, do, dth = up(A, device), up(ys, device), up(off, device), up(theta, device)
    dtail, dval, didx = _count_inputs(em, device)

    def run(lm):
        dl = up(lm, device)
        lnc, pre = _native.negbin_count_term(dl, dtail, em.log_norm, values=dval)
        lp = _native.linear_negbin_logp(dth, dA, dy, do, dl, lnc)
        gr = _native.linear_negbin_grad(dth, dA, dy, do, dl)
        rec, g = _native.negbin_pointwise(_native.linear_forward(dth, dA), dy, do, dl, pre, didx,
                                          em.lconst_device(device), want_ll=True, want_grad=True)
        q, p = dth.clone(), torch.ones_like(dth)
        _native.linear_negbin_leapfrog(q, p, dA, dy, do, dl, None, 1e-4, None, 2)
        return lnc, lp, gr, rec, g, q, p
    got, ref = run(lam), run(clean)
    lnc, lp, gr, rec, g, q, p = got
    for t in (gr, g, q, p):
        assert not bool(torch.isnan(t).any())
    for c in out_idx:
        assert float(lnc[c]) == -np.inf and float(lp[c]) == -np.inf and bool((rec[c] == -np.inf).all()), (c, lam[c])
    for a, b in zip(got, ref):
        assert torch.equal(bits(a[keep]), bits(b[keep]))
    # both ends: finite, and within the exact bound
    ex = NB.ExactNB(A, ys, off)
    for c in (1, 17):
        assert math.isfinite(float(lp[c])) and bool(torch.isfinite(gr[c]).all()) and bool(torch.isfinite(rec[c]).all())
        e = ex.chain(theta[c], lam[c], em.log_norm)
        a = G.err(float(lp[c]), e['lp']) / e['lp_bound']
        b = max(G.err(x, w) / bd for x, w, bd in zip(gr[c].cpu().numpy(), e['force'], e['force_bound']))
        print('lam = %g: logp %.3g grad %.3g of the bound' % (lam[c], a, b))
        assert a <= 1.0 and b <= 1.0, (c, a, b)
    # the model refuses a non-finite float
    for bad in (float('nan'), float('inf')):
        with pytest.raises(ValueError):
            em.lam_device(bad, 3, device)


def test_workspace_and_alias_refusals_leave_out_untouched(device):
    L = _native.lib()
    K, N, C = 5, 2049, 17
    A, ys, off, theta, lam = NB.case(K, N, C, 5)
    dA, dy, do, dth, dl = (up(v, device) for v in (A, ys, off, theta, lam))
    lnc = torch.zeros(C, dtype=torch.float64, device=device)
    st = _native.stream_handle(device)
    p = lambda t: t.data_ptr()
    out = torch.full((C,), -7.25, dtype=torch.float64, device=device)
    need = L.binf_linear_glm_logp_workspace_bytes(C, K, N)
    ws = torch.zeros(need // 8, dtype=torch.float64, device=device)
    for w, wb in ((None, need), (p(ws), need - 8), (None, 0)):
        assert L.binf_linear_negbin_logp_f64(p(dth), p(dA), p(dy), p(do), p(dl), p(lnc), p(out), w, wb,
                                             C, K, N, st) == _native.E_ARG
    assert L.binf_linear_negbin_logp_f64(p(dth), p(dA), p(dy), p(do), p(dl), p(out) + 8, p(out), p(ws), need,
                                         C, K, N, st) == _native.E_ALIAS
    assert L.binf_linear_negbin_logp_f64(p(dth), p(dA), p(dy), p(do), p(out), p(lnc), p(out), p(ws), need,
                                         C, K, N, st) == _native.E_ALIAS
    gout = torch.full((C, K), -7.25, dtype=torch.float64, device=device)
    gneed = L.binf_linear_glm_grad_workspace_bytes(C, K, N)
    gws = torch.zeros(gneed // 8, dtype=torch.float64, device=device)
    for w, wb in ((None, gneed), (p(gws), gneed - 8)):
        assert L.binf_linear_negbin_grad_f64(p(dth), p(dA), p(dy), p(do), p(dl), p(gout), w, wb,
                                             C, K, N, st) == _native.E_ARG
    assert L.binf_linear_negbin_grad_f64(p(dth), p(dA), p(dy), p(do), p(gout) + 16, p(gout), p(gws), gneed,
                                         C, K, N, st) == _native.E_ALIAS
    q, mom = dth.clone(), torch.ones_like(dth)
    lneed = L.binf_linear_glm_leapfrog_workspace_bytes(C, K, N)
    assert L.binf_linear_negbin_leapfrog_f64(p(q), p(mom), p(dA), p(dy), p(do), p(dl), 0, 0.0, 0.0, p(gws),
                                             lneed - 8, C, K, N, 0.01, None, 2, 0, st) == _native.E_ARG
    cout = torch.full((C,), -7.25, dtype=torch.float64, device=device)
    assert L.binf_negbin_count_term_f64(p(dl), p(dy), (1 << 20) + 1, 0.0, p(cout), None, 0, None, C,
                                        st) == _native.E_UNSUPPORTED
    assert L.binf_negbin_count_term_f64(p(cout) + 8, p(dy), 3, 0.0, p(cout), None, 0, None, C, st) == _native.E_ALIAS
    torch.cuda.synchronize()
    assert bool((out == -7.25).all()) and bool((gout == -7.25).all()) and bool((cout == -7.25).all())
    assert torch.equal(q, dth) and bool((mom == 1.0).all())
    assert L.binf_linear_negbin_logp_f64(p(dth), p(dA), p(dy), p(do), p(dl), p(lnc), p(out), p(ws), need,
                                         C, K, N, st) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())


# ---------------------------------------------------------------------------
# 5. dispatch
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


SPIED = ('linear_negbin_logp', 'linear_negbin_grad', 'linear_negbin_leapfrog', 'negbin_pointwise',
         'negbin_count_term', 'linear_forward', 'jacobian_contract', 'linear_glm_logp', 'linear_glm_grad',
         'linear_glm_leapfrog', 'glm_pointwise')


def test_dispatch(device, monkeypatch):
    A, ys, off, theta, lam = NB.case(5, 40, 9, 3)
    theta, lam = theta * 0.05, lam / 10.0
    x, dl = up(theta, device), up(lam, device)
    spy = _Spy(monkeypatch, SPIED)
    post = _posterior(A, ys, off, None)
    lik = post.likelihoods['outcomes']
    assert set(lik.variables) == {'coefficients', 'log_dispersion'}
    assert not glm.logp_covers('negbin_log', 9, 40)
    lp = lik.log_prob(coefficients=x, log_dispersion=dl)
    assert spy.calls == ['linear_forward', 'negbin_count_term', 'negbin_pointwise'] and lp.shape == (9,)
    del spy.calls[:]
    g = lik.gradient(coefficients=x, log_dispersion=dl)
    assert spy.calls == ['linear_negbin_grad'] and g.shape == x.shape
    # [C x 1] and a float shared by all chains
    assert torch.equal(bits(lik.gradient(coefficients=x, log_dispersion=dl.reshape(-1, 1))), bits(g))
    g7 = lik.gradient(coefficients=x, log_dispersion=0.75)
    assert torch.equal(bits(g7), bits(lik.gradient(coefficients=x, log_dispersion=torch.full_like(dl, 0.75))))
    # not fixed: no fused leapfrog; fixed (as inside a Gibbs conditional): the fused one
    assert post.native_leapfrog_spec('coefficients') is None
    for prior in (None, (0.5, 0.0)):
        del spy.calls[:]
        fixed = _posterior(A, ys, off, prior, dl)
        s = HMCSampler(fixed, x.clone(), 1e-3, 3, variable_name='coefficients')
        s._leapfrog(x.clone(), torch.ones_like(x), 1e-3, 3)
        assert spy.calls == ['linear_negbin_leapfrog'], (prior, spy.calls)
    cond = post.conditional_factory(log_dispersion=dl)
    assert cond.native_leapfrog_spec('coefficients')[0] == 'linear_glm'
    # a shape that fills the chip: the fused log-prob, the count term before it
    Cb, Nb = 4096, 8192
    assert glm.logp_covers('negbin_log', Cb, Nb) and not glm.logp_covers('negbin_log', Cb, 1024)
    Ab, yb, ob, tb, lb = NB.case(5, Nb, Cb, 4)
    xb, dlb = up(tb * 0.05, device), up(lb / 10.0, device)
    big = Likelihood('outcomes', LinearForwardModel('covariates', Ab), NegBinomialLogErrorModel(yb, ob))
    del spy.calls[:]
    lp_b = big.log_prob(coefficients=xb, log_dispersion=dlb)
    assert spy.calls == ['negbin_count_term', 'linear_negbin_logp'] and lp_b.shape == (Cb,)
    f = NB.float_case(tb[:8] * 0.05, Ab, yb, ob, lb[:8] / 10.0, big.error_model.log_norm)
    assert np.all(np.abs(lp_b[:8].cpu().numpy() - f['lp']) <= 2 * f['lp_bound'])
    # a lam rewritten in place is the one the next call reads
    dlb.add_(0.25)
    lp_c = big.log_prob(coefficients=xb, log_dispersion=dlb)
    f2 = NB.float_case(tb[:8] * 0.05, Ab, yb, ob, lb[:8] / 10.0 + 0.25, big.error_model.log_norm)
    assert np.all(np.abs(lp_c[:8].cpu().numpy() - f2['lp']) <= 2 * f2['lp_bound'])
    assert not torch.equal(bits(lp_c), bits(lp_b))


def test_samplers_take_the_hooks(device, monkeypatch):
    """HMC (the fused leapfrog) and NUTS (the fused gradient) on a posterior with lam fixed; under
    ``graph`` the replay equals eager, and a replay after lam was rewritten in place sees the new
    lam."""
    K, N, C, L, n = 4, 50, 33, 3, 5
    _, ys, off, _, lam = NB.case(K, N, C, 17)
    rs = np.random.RandomState(8)
    A = rs.standard_normal((K, N))
    q0 = 0.3 * rs.standard_normal((C, K))
    lam = lam / 10.0
    draws = [(rs.standard_normal((C, K)), rs.uniform(size=C)) for _ in range(2 * n)]
    spy = _Spy(monkeypatch, SPIED)

    def run(graph):
        dl = up(lam, device)
        s = HMCSampler(_posterior(A, ys, off, (0.5, 0.0), dl), up(q0, device), 0.05, L,
                       variable_name='coefficients', graph=graph)
        out = [s.sample(p0=up(p, device), u=up(u, device)).clone() for p, u in draws[:n]]
        dl.add_(0.5)                                   # in place: the same buffer, a new lam
        out += [s.sample(p0=up(p, device), u=up(u, device)).clone() for p, u in draws[n:]]
        return s, out
    se, eager = run(False)
    assert 'linear_negbin_leapfrog' in spy.calls and 'linear_glm_leapfrog' not in spy.calls
    sg, graph = run('always')
    assert len(sg._graphs) == 1 and not se._graphs
    for a, b in zip(eager, graph):
        assert torch.equal(bits(a), bits(b))
    assert torch.equal(se.n_accepted, sg.n_accepted) and int(sg.n_accepted.sum()) > 0
    # the second half did see the new lam: an unchanged lam gives other draws
    dl = up(lam, device)
    s0 = HMCSampler(_posterior(A, ys, off, (0.5, 0.0), dl), up(q0, device), 0.05, L, variable_name='coefficients')
    same = [s0.sample(p0=up(p, device), u=up(u, device)).clone() for p, u in draws]
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(same[:n], eager[:n]))
    assert not torch.equal(bits(same[-1]), bits(eager[-1]))
    del spy.calls[:]
    s = NUTSSampler(_posterior(A, ys, off, None, up(lam, device)), up(q0, device), 0.05, max_tree_depth=4,
                    variable_name='coefficients', rng=DeviceRNG(3, device))
    s.sample_n(3)
    assert 'linear_negbin_grad' in spy.calls and 'linear_glm_grad' not in spy.calls


# ---------------------------------------------------------------------------
# 6. stationarity of the coefficients against a closed form
# ---------------------------------------------------------------------------
N_OBS, CHAINS, N_WARM, N_KEEP, SEED, LAM0 = 24, 512, 150, 200, 20250, math.log(2.0)


def _closed_form():
    """Intercept-only, no prior, phi fixed: with z = theta - lam the likelihood is
    prod_n sigma(z)**y_n (1 - sigma(z))**phi, so logistic(theta - lam) ~ Beta(sum y, N phi):
    E theta = lam + psi(sum y) - psi(N phi), Var theta = psi_1(sum y) + psi_1(N phi)."""
    rs = np.random.RandomState(SEED)
    phi = math.exp(LAM0)
    ys = rs.negative_binomial(phi, phi / (phi + 3.0), size=N_OBS).astype(np.float64)
    s, b = float(ys.sum()), N_OBS * phi
    assert s >= 1
    return ys, LAM0 + float(psi(s) - psi(b)), float(polygamma(1, s) + polygamma(1, b))


class _HostPDF(object):
    """The same model as a user's torch PDF, the term's gradient multiplied by ``sign``."""

    def __init__(self, ys, sign):
        self.ys, self.sign, self.phi = ys, sign, math.exp(LAM0)

    def _z(self, coefficients):
        return coefficients.reshape(-1, 1).expand(-1, self.ys.shape[0]) - LAM0

    def log_prob(self, coefficients):
        z = self._z(coefficients)
        return (self.ys * z - (self.ys + self.phi) * torch.nn.functional.softplus(z)).sum(dim=1)

    def gradient(self, coefficients):
        z = self._z(coefficients)
        return self.sign * ((self.ys + self.phi) * torch.sigmoid(z) - self.ys).sum(dim=1, keepdim=True)


def _stationarity(device, sampler, pdf=None):
    ys, mean, var = _closed_form()
    sd = math.sqrt(var)
    rs = np.random.RandomState(SEED + 1)
    q0 = up(mean + sd * (1.0 + rs.standard_normal((CHAINS, 1))), device)      # started one sd off
    if pdf is None:
        pdf = _posterior(np.ones((1, N_OBS)), ys, None, None, LAM0)
    rng = DeviceRNG(SEED, device)
    if sampler == 'hmc':
        s = HMCSampler(pdf, q0, 0.375 * sd, 4, variable_name='coefficients', rng=rng)
    else:
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
    return ok, fig


@pytest.mark.parametrize('sampler', ['hmc', 'nuts'])
def test_stationarity_of_the_coefficients(device, monkeypatch, sampler):
    """512 chains, 150 + 200 transitions, one seed: the mean within 5 MCSE, the pooled variance
    within 5 of its standard errors, split-R^ < 1.01."""
    spy = _Spy(monkeypatch, ('linear_negbin_leapfrog', 'linear_negbin_grad'))
    ok, fig = _stationarity(device, sampler)
    print(sampler, fig)
    assert ok, fig
    assert ('linear_negbin_leapfrog' if sampler == 'hmc' else 'linear_negbin_grad') in spy.calls


def test_the_margin_sees_a_flipped_sign(device):
    """The same check on a host-side torch PDF: passes as written, fails with the gradient's sign
    flipped.  No kernel is mutated."""
    ys, _, _ = _closed_form()
    y = up(ys, device)
    ok, fig = _stationarity(device, 'hmc', _HostPDF(y, 1.0))
    assert ok, fig
    bad, fig = _stationarity(device, 'hmc', _HostPDF(y, -1.0))
    print('flipped', fig)
    assert not bad, fig
