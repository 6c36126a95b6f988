"""CPU tests of the negative-binomial family: the host restatement (tests/negbin_ref.py) against
50-digit arithmetic within the derived bounds (tests/negbin_bounds.py), the identity the kernels
rest on against the textbook density, the tail-count sum against the per-datum sum, the model's
plumbing, ``RWMCSampler(variable=...)``'s signature, and the host-side refusals of the C entry
points (decided before any launch)."""
import inspect
import math

import numpy as np
import pytest
import torch

import glm_bounds as G
import glm_ref as R
import negbin_bounds as NB
import negbin_ref as NR
from binf_amd import _native, native
from binf_amd.example.samplers import RWMCSampler
from binf_amd.model import glm, linear
from binf_amd.model.glm import NegBinomialLogErrorModel
from binf_amd.model.linear import LinearForwardModel
from binf_amd.pdf.likelihoods import Likelihood
from binf_amd.pdf.posteriors import Posterior

ETAS = [0.0, 2.0 ** -60, -2.0 ** -60, 1.0, -1.0, 36.7, -36.7, 40.0, -40.0, 708.0, -708.0, 745.0, -745.0, 800.0]
LAMS = [-708.0, -30.0, -20.0, -1.0, 0.0, math.log(2.0), 3.0, 20.0, 30.0, 709.0]
COUNTS = [0.0, 1.0, 5.0, 40.0, 300.0]


def test_restatement_against_truth_on_a_grid():
    """negbin_ref.term (numpy, the kernel's expressions in its order) against mpmath at 50 digits
    within negbin_bounds' per-datum bounds for an exact eta (delta = 0), over eta x lam x y."""
    worst = [0.0, 0.0]
    for eta in ETAS:
        for lam in LAMS:
            for y in COUNTS:
                ll, g = NR.term(np.float64(eta), y, lam)
                with np.errstate(over='ignore', invalid='ignore'):
                    B, rho, _, _ = NB.term_bounds(np.float64(eta), 0.0, y, lam)
                assert not np.isnan(ll) and np.isfinite(g) and np.isfinite(rho)
                if abs(NR.exact_ll(eta, y, lam)) > 1.7e308:
                    # (y + phi) softplus(z) is no double (phi near e**709 and z > 0): -inf, as the
                    # Poisson term beyond exp's range; never NaN
                    assert ll == -np.inf and lam > 700.0 and eta > lam
                    continue
                assert np.isfinite(ll) and np.isfinite(B)
                a = G.err(ll, NR.exact_ll(eta, y, lam)) / float(B)
                b = G.err(g, NR.exact_g(eta, y, lam)) / float(rho)
                assert a <= 1.0 and b <= 1.0, (eta, lam, y, a, b)
                worst = [max(worst[0], a), max(worst[1], b)]
    print('largest fractions of the bound: ll %.3f g %.3f' % tuple(worst))
    assert min(worst) > 0.0


def test_host_exp_of_lam_within_its_allowance():
    """phi = exp(lam) is held on its own: 8u phi over the regular range (the host library here;
    the device's enters every device bound through the same allowance)."""
    M = R.mp()
    for lam in LAMS + [-707.5, 708.5, 1e-300, -1e-9]:
        phi = float(NR.phi_of(lam))
        assert 0.0 < phi < np.inf and phi >= 2.0 ** -1022
        assert G.err(phi, M.exp(M.mpf(lam))) <= float(NB.phi_bound(phi))


def test_identity_against_the_textbook_density():
    """y z - (y + phi) softplus(z) + sum_{j<y} log(phi + j) - lgamma(y + 1) is lgamma(y + phi) -
    lgamma(phi) - lgamma(y + 1) + phi log phi + y eta - (y + phi) log(phi + mu), at 50 digits."""
    for eta in (-40.0, -1.0, 0.0, 0.3, 5.0, 40.0):
        for lam in (-30.0, -1.0, 0.0, math.log(2.0), 20.0, 30.0):
            for y in (0, 1, 5, 40, 300):
                a, b = NR.exact_log_density(eta, y, lam), NR.textbook_log_density(eta, y, lam)
                assert abs(a - b) <= R.mp().mpf(10) ** -38 * max(1, abs(b)), (eta, lam, y, a, b)


def test_tail_count_sum_is_the_per_datum_sum():
    M = R.mp()
    rs = np.random.RandomState(4)
    ys = np.floor(rs.gamma(0.7, 12.0, size=60))
    ys[:2] = (0.0, 300.0)
    tail = NR.tail_counts(ys)
    em = NegBinomialLogErrorModel(ys)
    assert np.array_equal(em.tail_counts, tail) and tail.dtype == np.int64
    assert tail[0] == np.sum(ys > 0) and tail[-1] == 1 and tail.shape == (300,)
    assert np.all(np.diff(tail) <= 0) and int(tail.sum()) == int(ys.sum())
    for lam in (-30.0, 0.0, 30.0):
        per_datum = M.fsum(NR.exact_prefix(lam, y) for y in ys)
        assert abs(NR.exact_count(lam, tail) - per_datum) <= M.mpf(10) ** -40 * abs(per_datum)
        # and the restatement's two orders against it, inside their bounds
        got = float(NR.count_term(lam, tail, em.log_norm)[0])
        assert G.err(got, per_datum + M.mpf(em.log_norm)) <= NB.count_bound(lam, tail, em.log_norm)
        pre = NR.prefix([lam], em.count_values)[0]
        for k in (0, 1, len(pre) // 2, len(pre) - 1):
            v = em.count_values[k]
            assert G.err(pre[k], NR.exact_prefix(lam, v)) <= NB.prefix_bound(lam, v)[0], (lam, v)
        pb, pm = NB.prefix_bounds([lam], em.count_values)
        one = np.array([NB.prefix_bound(lam, v) for v in em.count_values])
        assert np.all(one[:, 0] <= pb[0]) and np.all(pb[0] <= one[:, 0] * (1 + 1e-6) + 1e-300)
    assert NR.count_term([0.0], np.zeros(0), -2.5)[0] == -2.5


def test_bounds_self_test():
    figs = NB.self_test()
    assert len(figs) == 6
    for f in figs:
        assert 0.0 < f['lp'] <= 1.0 and 0.0 < f['force'] <= 1.0


def test_lam_range_on_the_host():
    lo, hi = float(np.nextafter(-708.0, -np.inf)), float(np.nextafter(709.0, np.inf))
    lam = np.array([-708.0, 709.0, lo, hi, -np.inf, np.inf, np.nan, 0.0])
    assert list(NR.regular(lam)) == [True, True, False, False, False, False, False, True]
    assert list(NR.clamp(lam)) == [-708.0, 709.0, -708.0, 709.0, -708.0, 709.0, -708.0, 0.0]
    assert (_native.NEGBIN_LAM_MIN, _native.NEGBIN_LAM_MAX) == (NR.LAM_MIN, NR.LAM_MAX)
    out = NR.count_term(lam, [2, 1], 0.5)
    assert np.all(np.isfinite(out[[0, 1, 7]])) and np.all(out[2:7] == -np.inf)
    ll, g = NR.term(np.zeros((8, 3)), np.array([0.0, 1.0, 7.0]), lam)
    assert not np.isnan(ll).any() and not np.isnan(g).any()


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
def test_constructor_refusals():
    for bad in ([1.0, -1.0], [0.5, 2.0], [float('nan')], [[1.0, 2.0]]):
        with pytest.raises(ValueError):
            NegBinomialLogErrorModel(bad)
    with pytest.raises(ValueError, match='2\\*\\*20'):
        NegBinomialLogErrorModel([0.0, float((1 << 20) + 1)])
    NegBinomialLogErrorModel([0.0, float(1 << 20)])
    with pytest.raises(ValueError):
        NegBinomialLogErrorModel([1.0, 2.0], offset=[0.0])


def test_variables_fixing_and_clone():
    ys = np.array([0.0, 3.0, 1.0, 3.0, 7.0])
    em = NegBinomialLogErrorModel(ys, offset=np.full(5, 0.25))
    assert em.variables == {'mock_data', 'log_dispersion'} and em.kind == 'negbin_log'
    assert em.family == _native.GLM_NEGBIN_LOG == 2
    assert em.native_spec() == ('negbin_log', em)
    assert list(em.tail_counts) == [4, 3, 3, 1, 1, 1, 1]
    assert list(em.count_values) == [0.0, 1.0, 3.0, 7.0] and list(em._index) == [0, 2, 1, 2, 3]
    want = [-math.lgamma(y + 1.0) for y in ys]
    assert list(em.pointwise_constants) == want and em.log_norm == math.fsum(want)
    fixed = em.conditional_factory(log_dispersion=0.5)
    assert fixed.variables == {'mock_data'} and fixed['log_dispersion'].value == 0.5
    assert em.variables == {'mock_data', 'log_dispersion'}
    copy = fixed.clone()
    assert copy.variables == {'mock_data'} and copy['log_dispersion'].value == 0.5
    assert copy._dev is fixed._dev and np.array_equal(copy.ys, ys) and np.array_equal(copy.offset, em.offset)
    t = torch.zeros(3, dtype=torch.float64)
    em2 = NegBinomialLogErrorModel(ys)
    em2.fix_variables(log_dispersion=t)
    assert em2['log_dispersion'].value is t

    class Mine(NegBinomialLogErrorModel):
        def _evaluate_gradient(self, mock_data, log_dispersion):
            return None
    assert Mine(ys).native_spec() is None


def test_accepted_shapes_of_log_dispersion():
    em = NegBinomialLogErrorModel([0.0, 2.0])
    for bad in (float('nan'), float('inf'), -float('inf')):
        with pytest.raises(ValueError, match='finite'):
            em.lam_device(bad, 3, torch.device('cpu'))
    # tensors must live on the device (checked before their shape; the shapes themselves --
    # [C], [C x 1], a float -- are compared bit for bit in the GPU tests)
    with pytest.raises(TypeError):
        em.lam_device(torch.zeros(3, dtype=torch.float64), 3, torch.device('cpu'))


def test_registry_and_leapfrog_matching_on_the_host():
    hooks = native.likelihood_hooks(linear.KIND, 'negbin_log')
    A =np.random.RandomState(0).standard_normal((3, 12))
    ys = np.arange(12.0)
    em = NegBinomialLogErrorModel(ys)
    lik = Likelihood('outcomes', LinearForwardModel('covariates', A), em)
    pair = native.model_pair(lik)
    assert pair is not None and pair[0][0] == linear.KIND and pair[1][0] == 'negbin_log'
    assert pair[2][:2] == (glm.negbin_log_prob, glm.negbin_gradient)
    assert tuple(hooks[:2]) == (glm.negbin_log_prob, glm.negbin_gradient)
    post = Posterior({'outcomes': lik}, {})
    assert post.variables == {'coefficients', 'log_dispersion'}
    assert post.native_leapfrog_spec('coefficients') is None          # the dispersion is free
    cond = post.conditional_factory(log_dispersion=0.5)
    spec = cond.native_leapfrog_spec('coefficients')
    assert spec[0] == 'linear_glm' and spec[2].kind == 'negbin_log' and spec[3] is None
    assert 'log_dispersion' in spec[2].parameters
    assert glm.LOGP_MIN_WORKGROUPS['negbin_log'] == glm.LOGP_MIN_WORKGROUPS['binomial_logit'] == 256
    assert glm.logp_covers('negbin_log', 4096, 8192) and not glm.logp_covers('negbin_log', 4096, 1024)


def test_rwmc_variable_keyword_keeps_the_default():
    """The keyword defaults to 'coefficients' and is last: every existing call binds as before.
    (The unchanged draw streams of the default are held by the existing RWMC tests, which pass
    unchanged; on a device they are compared with the explicit keyword in the GPU tests.)"""
    sig = inspect.signature(RWMCSampler.__init__)
    assert list(sig.parameters) == ['self', 'pdf', 'state', 'stepsize', 'rng', 'variable']
    assert sig.parameters['variable'].default == 'coefficients'
    s = RWMCSampler(None, None, 0.1)
    assert s.variable == 'coefficients' and list(s.last_draw_stats) == ['coefficients']
    with pytest.raises(TypeError, match='DeviceRNG'):
        RWMCSampler(None, torch.zeros(4, 1, dtype=torch.float64), 0.1, variable='log_dispersion')


# ---------------------------------------------------------------------------
# host-side refusals of the C entry points
# ---------------------------------------------------------------------------
def test_refusals_without_gpu():
    L = _native.lib()
    base = 1 << 40
    th, A, ys, off, lam, lnc, out, ws, q, p = (base + (i << 34) for i in range(10))
    C, K, N = 5, 3, 2049
    need = L.binf_linear_glm_logp_workspace_bytes(C, K, N)

    def logp(th_=th, ys_=ys, lam_=lam, lnc_=lnc, out_=out, ws_=ws, wb=need, K_=K, C_=C, N_=N):
        return L.binf_linear_negbin_logp_f64(th_, A, ys_, off, lam_, lnc_, out_, ws_, wb, C_, K_, N_, None)
    assert logp(th_=None) == _native.E_ARG and logp(ys_=None) == _native.E_ARG and logp(out_=None) == _native.E_ARG
    assert logp(lam_=None) == _native.E_ARG and logp(lnc_=None) == _native.E_ARG
    assert logp(ws_=None) == _native.E_ARG and 'workspace' in _native.last_error()
    assert logp(wb=need - 8) == _native.E_ARG
    assert logp(K_=65) == _native.E_UNSUPPORTED and logp(N_=0) == _native.E_UNSUPPORTED
    assert logp(C_=65535 * 64 + 1, wb=1 << 60) == _native.E_UNSUPPORTED
    assert logp(out_=lam + 8) == _native.E_ALIAS and logp(out_=lnc) == _native.E_ALIAS and logp(out_=th) == _native.E_ALIAS
    assert logp(ws_=lam - 8) == _native.E_ALIAS and logp(ws_=out) == _native.E_ALIAS
    assert logp(C_=0) == 0

    C = 17
    gneed = L.binf_linear_glm_grad_workspace_bytes(C, K, N)

    def grad(th_=th, lam_=lam, out_=out, ws_=ws, wb=gneed, K_=K):
        return L.binf_linear_negbin_grad_f64(th_, A, ys, off, lam_, out_, ws_, wb, C, K_, N, None)
    assert grad(th_=None) == _native.E_ARG and grad(lam_=None) == _native.E_ARG and grad(out_=None) == _native.E_ARG
    assert grad(ws_=None) == _native.E_ARG and grad(wb=gneed - 8) == _native.E_ARG
    assert grad(K_=65) == _native.E_UNSUPPORTED
    assert grad(out_=lam) == _native.E_ALIAS and grad(ws_=lam + 8) == _native.E_ALIAS

    lneed = L.binf_linear_glm_leapfrog_workspace_bytes(C, K, N)

    def leap(q_=q, p_=p, lam_=lam, hp=1, ws_=ws, wb=lneed, nsteps=3, mode=0, K_=K):
        return L.binf_linear_negbin_leapfrog_f64(q_, p_, A, ys, off, lam_, hp, 1.0, 0.0, ws_, wb, C, K_, N,
                                                 0.01, None, nsteps, mode, None)
    assert leap(lam_=None) == _native.E_ARG and leap(q_=None) == _native.E_ARG
    assert leap(nsteps=0) == _native.E_ARG and leap(mode=5) == _native.E_ARG and leap(hp=2) == _native.E_ARG
    assert leap(ws_=None) == _native.E_ARG and leap(wb=lneed - 8) == _native.E_ARG
    assert leap(K_=65) == _native.E_UNSUPPORTED
    assert leap(q_=lam) == _native.E_ALIAS and leap(p_=lam + 8) == _native.E_ALIAS and leap(ws_=lam) == _native.E_ALIAS

    tail, vals, pre = (base + (i << 34) for i in range(10, 13))

    def count(lam_=lam, tail_=tail, ymax=7, out_=out, vals_=None, J=0, pre_=None, C_=C):
        return L.binf_negbin_count_term_f64(lam_, tail_, ymax, 0.5, out_, vals_, J, pre_, C_, None)
    assert count(out_=None) == _native.E_ARG and count(lam_=None) == _native.E_ARG and count(tail_=None) == _native.E_ARG
    assert count(ymax=-1) == _native.E_ARG and count(pre_=pre, J=0) == _native.E_ARG
    assert count(pre_=pre, J=3, vals_=None) == _native.E_ARG
    assert count(ymax=(1 << 20) + 1) == _native.E_UNSUPPORTED and '2^20' in _native.last_error()
    with pytest.raises(NotImplementedError):
        _native.check(count(ymax=(1 << 20) + 1), 'x')
    assert count(out_=lam + 8) == _native.E_ALIAS and count(out_=tail + 16) == _native.E_ALIAS
    assert count(out_=None, pre_=vals + 8, vals_=vals, J=3) == _native.E_ALIAS
    assert count(pre_=out + 8, vals_=vals, J=3) == _native.E_ALIAS
    assert count(C_=0) == 0

    S, mock, idx, lc, g = 4, base + (13 << 34), base + (14 << 34), base + (15 << 34), base + (16 << 34)

    def point(mock_=mock, lam_=lam, pre_=None, idx_=None, J=0, ll_=out, g_=None, S_=S, N_=N):
        return L.binf_negbin_pointwise_f64(mock_, ys, off, lam_, pre_, idx_, lc, ll_, g_, S_, N_, J, None)
    assert point(ll_=None) == _native.E_ARG and point(mock_=None) == _native.E_ARG and point(lam_=None) == _native.E_ARG
    assert point(pre_=pre) == _native.E_ARG and point(idx_=idx) == _native.E_ARG
    assert point(pre_=pre, idx_=idx, J=0) == _native.E_ARG
    assert point(J=(1 << 20) + 2, pre_=pre, idx_=idx) == _native.E_UNSUPPORTED
    assert point(N_=(1 << 31) - 1) == _native.E_UNSUPPORTED
    assert point(ll_=mock + 8) == _native.E_ALIAS and point(ll_=lam) == _native.E_ALIAS
    assert point(ll_=pre + 8, pre_=pre, idx_=idx, J=2) == _native.E_ALIAS
    assert point(g_=out + 8) == _native.E_ALIAS
    assert point(S_=0) == 0 and point(N_=0) == 0
