"""
Linear forward models: ``mock = coefficients . A`` with a constant design matrix
``A [n_params x n_data]`` shared by all chains -- Fourier or spline bases,
regression on measured covariates, any fixed dictionary.

A user's model is a subclass that builds its design matrix in ``__init__``::

    class Fourier(LinearForwardModel):
        def __init__(self, xs, n_modes):
            rows = [np.ones_like(xs)]
            for m in range(1, n_modes + 1):
                rows += [np.cos(m * xs), np.sin(m * xs)]
            super(Fourier, self).__init__('fourier', np.vstack(rows))

Nothing else is needed for the fast path: importing this module registers the kind
``'linear'`` with ``binf_amd.native``.  Paired with an error model that advertises the
kind ``'gaussian'``, the likelihood's log-prob runs in ``binf_linear_gauss_logp_f64``
(f64 MFMA product, residual and chi^2 in registers; reference path
``binf/pdf/likelihoods.py:141-146`` calling ``binf/model/forwardmodels.py:23-28``), its
gradient in ``binf_poly_gauss_grad_f64`` and ``HMCSampler._leapfrog`` in
``binf_poly_leapfrog_f64`` -- the ``[C x n_data]`` mock data is never written to HBM.
Paired with ``BinomialLogitErrorModel`` or ``PoissonLogErrorModel``
(``binf_amd/model/glm.py``: logistic and Poisson regression) the same three run in
``binf_linear_glm_logp_f64`` / ``_grad_f64`` / ``_leapfrog_f64``.
With any other error model ``_evaluate`` is ``binf_linear_forward_f64`` and the
likelihood is evaluated as written.  A subclass that overrides ``_evaluate`` or
``_evaluate_jacobi_matrix`` is evaluated as written, too.

Small models (up to 16 coefficients, up to 1024 data points) are launch-bound on that
per-step path.  ``LinearForwardModel(name, design, resident=True)`` opts such a model
into the chain-resident kernels (``binf_amd/model/linear_resident.py``,
``csrc/linear_chain_kernel.hpp``): a whole ``HMCSampler.sample()``, or n Gibbs sweeps of
``sample_n``, in one launch with the chain's state on chip.  It is an opt-in of the
model because the resident kernel's arithmetic is its own (its energies do not carry
the MFMA product's bits), and ``sample()`` and ``sample_n()`` of one model must agree
bit for bit.  Without the flag nothing changes.
"""
import numpy as np
import torch

from binf_amd import ArrayParameter, _native, native
from binf_amd.model.forwardmodels import AbstractForwardModel

KIND = 'linear'              # the name this module's hooks are registered under
MAX_PARAMS = 64              # rows of the design matrix the kernels cover


def _as2d(x):
    return x if x.dim() == 2 else x.reshape(1, -1)


def _unchanged(obj, base, names):
    """True if ``obj``'s class still uses ``base``'s implementation of every method in
    ``names`` -- a subclass that overrides one of them must be evaluated as written,
    not through the fused kernels of the base model."""
    return all(getattr(type(obj), n, None) is getattr(base, n) for n in names)


class LinearForwardModel(AbstractForwardModel):
    """``mock[c, :] = variable[c, :] . design``; the Jacobian is ``design`` itself.

    ``design``: ``[n_params x n_data]`` numpy array or tensor, constant, shared by all
    chains.  The device copy is made when first needed and shared with clones; model
    data are immutable once evaluated.

    ``resident=True``: posteriors of this model may run in the chain-resident kernels
    (kind ``'linear_resident'``) where they cover the shape and are the faster launch;
    everywhere else, and for every hook of the kind ``'linear'``, the model behaves as
    without the flag."""

    def __init__(self, name, design, variable='coefficients', resident=False):
        super(LinearForwardModel, self).__init__(name)
        self._dev = {}
        self._variable = variable
        self._resident = bool(resident)
        d = design.detach().cpu().numpy() if isinstance(design, torch.Tensor) \
            else np.asarray(design, dtype=np.float64)
        if d.ndim != 2:
            raise ValueError('design matrix must be [n_params x n_data], got shape %s'
                             % (tuple(d.shape),))
        self._design = np.ascontiguousarray(d, dtype=np.float64)
        self._register_variable(variable, differentiable=True)
        self.update_var_param_types(**{variable: ArrayParameter})
        self._set_original_variables()

    @property
    def design(self):
        return self._design

    @property
    def variable(self):
        return self._variable

    @property
    def resident(self):
        return self._resident

    def design_matrix(self, n_params, device):
        """The device copy of the design matrix (built once, shared with clones)."""
        if int(n_params) != self._design.shape[0]:
            raise ValueError('%d parameters for a design matrix of %d rows'
                             % (int(n_params), self._design.shape[0]))
        key = ('A', device)
        if key not in self._dev:
            self._dev[key] = torch.from_numpy(self._design).to(device)
        return self._dev[key]

    # -- model interface --------------------------------------------------------
    # (the variable's name is chosen per instance: the methods take it by keyword)
    def _evaluate(self, **variables):
        x = variables[self._variable]
        _native.require_device(x, self._variable)
        x2 = _as2d(x).contiguous()
        out = _native.linear_forward(x2, self.design_matrix(x2.shape[1], x.device))
        return out if x.dim() == 2 else out.reshape(-1)

    def _evaluate_jacobi_matrix(self, **variables):
        x = variables[self._variable]
        _native.require_device(x, self._variable)
        return self.design_matrix(x.shape[-1], x.device)

    def clone(self):
        copy = LinearForwardModel.__new__(self.__class__)
        LinearForwardModel.__init__(copy, self.name, self._design, self._variable,
                                    self._resident)
        # whatever a subclass keeps beside the design matrix (its grid, its mode count)
        for k, v in self.__dict__.items():
            if k not in copy.__dict__:
                copy.__dict__[k] = v
        copy._dev = self._dev            # immutable model data: share it
        self._set_parameters(copy)
        return copy

    def native_spec(self):
        if _unchanged(self, LinearForwardModel, ('_evaluate', '_evaluate_jacobi_matrix')):
            return (KIND, self)
        return None


# ---------------------------------------------------------------------------
# the kind: Likelihood hooks for (linear, gaussian) and the fused leapfrog
# ---------------------------------------------------------------------------
def _usable(x):
    return isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float64 and \
        x.dim() in (1, 2) and x.shape[-1] <= MAX_PARAMS


def _inputs(fwm, em, fwm_vars, em_vars):
    """``(x, x2, A, ys, precision)`` or None (evaluate the models as written)."""
    fwm_vars = dict(fwm_vars)
    em_vars = dict(em_vars)
    fwm._complete_variables(fwm_vars)
    em._complete_variables(em_vars)
    x = fwm_vars.get(fwm.variable)
    if not _usable(x) or 'precision' not in em_vars or \
            x.shape[-1] != fwm.design.shape[0] or not hasattr(em, 'ys_device'):
        return None
    x2 = _as2d(x).contiguous()
    dev = x.device
    return x, x2, fwm.design_matrix(x2.shape[1], dev), em.ys_device(dev), em_vars['precision']


def log_prob(likelihood, fwm, em, fwm_vars, em_vars):
    args = _inputs(fwm, em, fwm_vars, em_vars)
    if args is None:
        return None
    _, x2, A, ys, precision = args
    return _native.linear_gauss_logp(x2, A, ys, precision)


def gradient(likelihood, fwm, em, fwm_vars, em_vars):
    args = _inputs(fwm, em, fwm_vars, em_vars)
    if args is None:
        return None
    x, x2, A, ys, precision = args
    out = _native.poly_gauss_grad(x2, A, ys, precision)
    return out if x.dim() == 2 else out.reshape(-1)


def _is_linear_pair(likelihood):
    """Linear forward model + Gaussian error model, neither overridden?  The error
    model is recognised by the kind it advertises, not by its class."""
    fs = getattr(likelihood.forward_model, 'native_spec', lambda: None)()
    es = getattr(likelihood.error_model, 'native_spec', lambda: None)()
    return fs is not None and es is not None and fs[0] == KIND and es[0] == 'gaussian'


def posterior_leapfrog_spec(posterior, variable_name):
    """``(forward_model, error_model, precision)`` if the force on ``variable_name`` is
    exactly ONE linear + Gaussian-error likelihood with its precision fixed (every
    other component has no differentiable variable), else None."""
    from binf_amd.pdf.likelihoods import Likelihood
    components = getattr(posterior, '_ordered_components', None)
    if components is None:
        return None
    lik = None
    for f in components():
        if not (len(f.variables) > 0 and len(f.differentiable_variables) > 0):
            continue
        if lik is not None or not isinstance(f, Likelihood) or not _is_linear_pair(f) or \
                f.forward_model.variable != variable_name or \
                set(f.variables) != {variable_name} or \
                'precision' not in f.error_model.parameters or \
                not hasattr(f.error_model, 'ys_device'):
            return None
        lik = f
    if lik is None or lik.forward_model.design.shape[0] > MAX_PARAMS:
        return None
    return (lik.forward_model, lik.error_model, lik.error_model['precision'].value)


def leapfrog(sampler, spec, q2, p2, dt, dtc, nsteps, mode, q_from):
    _, fwm, em, precision = spec
    if not (q2.is_cuda and q2.dtype == torch.float64 and q2.shape[1] <= MAX_PARAMS and
            q2.shape[1] == fwm.design.shape[0]):
        return False
    if q_from is not None:
        q2.copy_(q_from)
    _native.poly_leapfrog(q2, p2, fwm.design_matrix(q2.shape[1], q2.device),
                          em.ys_device(q2.device), precision, dt, dtc, nsteps, mode)
    return True


native.register(
    KIND, replace=True,
    match_leapfrog=posterior_leapfrog_spec, leapfrog=leapfrog,
    likelihood={(KIND, 'gaussian'): (log_prob, gradient)})

# the opt-in chain-resident kernels register their own kind beside this one
from binf_amd.model import linear_resident  # noqa: E402,F401
# the generalised-linear error models register theirs ('linear_glm') after both: this
# kind's recognition is consulted first, unchanged
from binf_amd.model import glm  # noqa: E402,F401
