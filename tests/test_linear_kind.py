"""CPU tests of the linear forward model and its registered kind ``'linear'``
(``binf_amd/model/linear.py``): registration, recognition, the model's bookkeeping, the
C ABI's host-side refusals, and the self-test of the error bounds the GPU tests
(tests/test_gpu_linear.py) hold the kernels to.  No kernel is launched here."""
import ctypes

import numpy as np
import pytest
import torch

import linear_bounds
from binf_amd import _native, native
from binf_amd.example.likelihood import POLYVAL, ForwardModel, GaussianErrorModel
from binf_amd.example.priors import GammaPrior, GaussianPrior
from binf_amd.model import linear
from binf_amd.model.linear import LinearForwardModel
from binf_amd.pdf.likelihoods import Likelihood
from binf_amd.pdf.posteriors import Posterior


def _design(K=4, N=20, seed=0):
    return np.random.RandomState(seed).standard_normal((K, N))


def _likelihood(K=4, N=20, cls=LinearForwardModel):
    A = _design(K, N)
    ys = np.random.RandomState(1).standard_normal(N)
    return Likelihood('points', cls('basis', A), GaussianErrorModel(ys))


class _Overridden(LinearForwardModel):
    def _evaluate(self, coefficients):
        return coefficients @ self.design_matrix(coefficients.shape[-1], coefficients.device)


class _OverriddenJacobian(LinearForwardModel):
    def _evaluate_jacobi_matrix(self, coefficients):
        return self.design_matrix(coefficients.shape[-1], coefficients.device)


class Fourier(LinearForwardModel):
    """A user's model: its own constructor signature, its own attributes."""

    def __init__(self, xs, n_modes):
        self.xs, self.n_modes = np.asarray(xs), n_modes
        rows = [np.ones_like(self.xs)]
        for m in range(1, n_modes + 1):
            rows += [np.cos(m * self.xs), np.sin(m * self.xs)]
        super(Fourier, self).__init__('fourier', np.vstack(rows))


def test_importing_the_module_registers_the_kind():
    k = native.get('linear')
    assert k is not None and k.name == linear.KIND == 'linear'
    assert k.likelihood[('linear', 'gaussian')] == (linear.log_prob, linear.gradient)
    assert k.match_leapfrog is linear.posterior_leapfrog_spec and k.leapfrog is linear.leapfrog
    assert k.hmc is None and k.hmc_n is None and k.gibbs is None       # out of scope


def test_model_pair_returns_the_kinds_hooks():
    lik = _likelihood()
    fs, es, hooks = native.model_pair(lik)
    assert fs == ('linear', lik.forward_model) and es[0] == 'gaussian'
    assert hooks == (linear.log_prob, linear.gradient)
    # the polynomial pair keeps its own
    poly = Likelihood('points', ForwardModel(np.linspace(-1, 1, 20), POLYVAL),
                      GaussianErrorModel(np.zeros(20)))
    assert native.model_pair(poly)[2] != hooks


def test_an_overridden_model_is_evaluated_as_written():
    for cls in (_Overridden, _OverriddenJacobian):
        lik = _likelihood(cls=cls)
        assert lik.forward_model.native_spec() is None
        assert native.model_pair(lik) is None
    assert Fourier(np.linspace(0, 6, 30), 3).native_spec()[0] == 'linear'


def test_variables_differentiability_clone_and_conditional_factory():
    A = _design()
    f = LinearForwardModel('basis', A)
    g = ForwardModel(np.linspace(-1, 1, 20), POLYVAL)
    assert f.variables == g.variables == {'coefficients'}
    assert f.differentiable_variables == g.differentiable_variables == {'coefficients'}
    assert f.var_param_types == g.var_param_types
    assert f.design.shape == (4, 20) and f.design.flags['C_CONTIGUOUS']
    c = f.clone()
    assert type(c) is LinearForwardModel and c is not f and c._dev is f._dev
    assert np.array_equal(c.design, A) and c.variables == {'coefficients'}
    # a model with another variable name and a tensor design
    h = LinearForwardModel('weights_model', torch.from_numpy(A), variable='weights')
    assert h.variables == {'weights'} and h.clone().variable == 'weights'
    with pytest.raises(ValueError):
        LinearForwardModel('bad', np.zeros(5))
    # a subclass with its own constructor clones, keeps its attributes and its kind
    u = Fourier(np.linspace(0, 6, 30), 3)
    uc = u.clone()
    assert type(uc) is Fourier and uc.n_modes == 3 and uc.design.shape == (7, 30)
    assert uc._dev is u._dev and uc.native_spec() == ('linear', uc)
    # the likelihood and its conditionals, as for the example's pair
    lik = _likelihood()
    ref = Likelihood('points', g, GaussianErrorModel(np.zeros(20)))
    assert lik.variables == ref.variables == {'coefficients', 'precision'}
    assert lik.differentiable_variables == ref.differentiable_variables
    cond = lik.conditional_factory(precision=2.0)
    assert cond.variables == {'coefficients'} and 'precision' in cond.error_model.parameters
    assert cond.forward_model._dev is lik.forward_model._dev
    assert native.model_pair(cond)[2] == (linear.log_prob, linear.gradient)
    cond = lik.conditional_factory(coefficients=np.zeros(4))
    assert cond.variables == {'precision'} and 'coefficients' in cond.forward_model.parameters


def _posterior(lik, K):
    return Posterior({lik.name: lik},
                     {'precision_prior': GammaPrior(1.0, 0.2),
                      'coefficients_prior': GaussianPrior(np.zeros(K), np.full(K, 5.0))})


def test_leapfrog_recognition():
    lik = _likelihood()
    post = _posterior(lik, 4)
    cond = post.conditional_factory(precision=2.5)
    spec = cond.native_leapfrog_spec('coefficients')
    assert spec is not None and spec[0] == 'linear' and spec[3] == 2.5
    assert spec[1].native_spec()[0] == 'linear' and spec[2].native_spec()[0] == 'gaussian'
    assert cond.native_leapfrog_spec('precision') is None
    assert cond.native_hmc_spec('coefficients') is None            # no whole-transition kernel
    # the precision still free: not a fixed-precision force
    assert post.native_leapfrog_spec('coefficients') is None
    # an overridden model, or too many rows, fall back to the per-step path
    over = _posterior(_likelihood(cls=_Overridden), 4).conditional_factory(precision=2.5)
    assert over.native_leapfrog_spec('coefficients') is None
    big = _posterior(_likelihood(K=65, N=70), 65).conditional_factory(precision=2.5)
    assert big.native_leapfrog_spec('coefficients') is None
    # the polynomial posterior is still the polynomial kind's
    poly = Likelihood('points', ForwardModel(np.linspace(-1, 1, 20), POLYVAL),
                      GaussianErrorModel(np.zeros(20)))
    assert _posterior(poly, 4).conditional_factory(precision=2.5).native_leapfrog_spec(
        'coefficients')[0] == 'poly'


def test_hooks_decline_what_the_kernels_do_not_cover():
    lik = _likelihood()
    fwm, em = lik.forward_model, lik.error_model
    host = torch.zeros((3, 4), dtype=torch.float64)
    for hook in (linear.log_prob, linear.gradient):
        assert hook(lik, fwm, em, {'coefficients': host}, {'precision': 1.0}) is None     # host tensor
        assert hook(lik, fwm, em, {'coefficients': host.float()}, {'precision': 1.0}) is None
        assert hook(lik, fwm, em, {'coefficients': np.zeros((3, 4))}, {'precision': 1.0}) is None
        assert hook(lik, fwm, em, {'coefficients': host}, {}) is None                     # no precision
    big = _likelihood(K=65, N=70)
    assert linear.log_prob(big, big.forward_model, big.error_model,
                           {'coefficients': torch.zeros((3, 65), dtype=torch.float64)},
                           {'precision': 1.0}) is None
    # ... and the leapfrog hook
    q = torch.zeros((3, 4), dtype=torch.float64)
    assert linear.leapfrog(None, ('linear', fwm, em, 1.0), q, q.clone(), 0.1, None, 2, 0, None) is False


def test_the_new_symbols_are_exported_and_bound():
    raw = ctypes.CDLL(_native.LIB_PATH)
    for name in ('binf_linear_forward_f64', 'binf_linear_gauss_logp_f64',
                 'binf_linear_gauss_logp_workspace_bytes'):
        assert hasattr(raw, name) and name in _native.SIGNATURES
    assert _native.ABI_VERSION == 7 and _native.lib().binf_abi_version() == 7
    assert callable(_native.linear_forward) and callable(_native.linear_gauss_logp)


def test_refusals_without_gpu():
    """Every refusal is made on the host before any launch: fake pointers are never
    dereferenced."""
    L = _native.lib()
    base = 1 << 40
    coeffs, design, ys, out, ws, tauc = (base + (i << 32) for i in range(6))
    C, K, N = 4, 5, 2000

    def logp(coeffs_=coeffs, out_=out, ws_=ws, ws_bytes=None, K_=K, N_=N, tauc_=None):
        need = L.binf_linear_gauss_logp_workspace_bytes(C, K_, N_)
        return L.binf_linear_gauss_logp_f64(coeffs_, design, ys, 1.0, tauc_, out_, ws_,
                                            need if ws_bytes is None else ws_bytes, C, K_, N_, None)
    # K = 65
    assert logp(K_=65) == _native.E_UNSUPPORTED and '65' in _native.last_error()
    assert L.binf_linear_forward_f64(coeffs, design, out, C, 65, N, None) == _native.E_UNSUPPORTED
    with pytest.raises(NotImplementedError):
        _native.check(_native.E_UNSUPPORTED, 'x')
    # the workspace: what it is, and a missing or short one
    assert L.binf_linear_gauss_logp_workspace_bytes(C, K, 1024) == 0       # one piece
    need = L.binf_linear_gauss_logp_workspace_bytes(C, K, N)
    assert need == 2 * C * 8                                               # two pieces of 1024 points
    # the pieces follow from N alone: the bytes are proportional to C
    assert L.binf_linear_gauss_logp_workspace_bytes(10 * C, K, N) == 10 * need
    assert L.binf_linear_gauss_logp_workspace_bytes(C, 64, N) == need
    assert logp(ws_=None) == _native.E_ARG and 'workspace' in _native.last_error()
    assert logp(ws_bytes=need - 8) == _native.E_ARG
    assert logp(coeffs_=None) == _native.E_ARG
    assert L.binf_linear_forward_f64(coeffs, None, out, C, K, N, None) == _native.E_ARG
    assert L.binf_linear_forward_f64(coeffs, design, out, -1, K, N, None) == _native.E_ARG
    # overlaps
    assert logp(out_=coeffs + 8) == _native.E_ALIAS                        # out inside coeffs
    assert logp(out_=coeffs) == _native.E_ALIAS
    assert logp(out_=ys + 8 * (N - 1)) == _native.E_ALIAS                  # ... the last datum
    assert logp(out_=tauc + 16, tauc_=tauc) == _native.E_ALIAS
    assert logp(ws_=out + 8) == _native.E_ALIAS                            # workspace against out
    assert logp(ws_=design - 8) == _native.E_ALIAS                         # its tail inside design
    assert L.binf_linear_forward_f64(coeffs, design, coeffs + 8, C, K, N, None) == _native.E_ALIAS
    assert L.binf_linear_forward_f64(coeffs, design, design - 8, C, K, N, None) == _native.E_ALIAS
    # nothing to do is not an error, with no buffer at all
    assert L.binf_linear_gauss_logp_f64(None, None, None, 1.0, None, None, None, 0, 0, K, N, None) == 0
    assert L.binf_linear_forward_f64(None, None, None, 0, K, N, None) == 0


def test_bounds_self_test():
    """numpy's own results lie inside the derived bounds; an error of 1e-9 S_n in ONE mock
    datum is outside every one of them."""
    figures = linear_bounds.self_test()
    assert len(figures) == 3
    for f in figures:
        assert f['mock'] <= 1.0 and f['chi2'] <= 1.0 and f['chi2_injected'] > 1.0


def test_reference_fixtures_lie_inside_the_bounds():
    """The reference's own Horner mock data, BLAS ``theta.dot(A)`` and ``error_logp`` of the
    fixtures whose Jacobian is stored whole, against exact arithmetic."""
    from conftest import GOLDEN_DIR, load_golden
    import os
    for name in ('k4_n20', 'k7_n37', 'k33_n1000'):
        z = load_golden(os.path.join(GOLDEN_DIR, 'ref_example_models_%s.npz' % name))
        A, ys = z['jacobi'], z['ys']
        assert A.shape[1] == len(ys)
        ex = linear_bounds.Exact(A, ys)
        for c in range(z['theta'].shape[0]):
            th, tau = z['theta'][c], float(z['precision'][c])
            info = ex.chain(th)
            assert np.all(ex.mock_error(th, z['mock'][c]) <= info['delta'])
            assert np.all(ex.mock_error(th, th.dot(A)) <= info['delta'])
            lp, bound = linear_bounds.logp_exact_and_bound(info['chi2'], info['chi2_bound'], tau, len(ys))
            assert linear_bounds.logp_error(z['error_logp'][c], lp) <= bound
