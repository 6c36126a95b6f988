"""
Generalised linear models: error models for binary / binomial outcomes (logistic
regression) and for counts (Poisson regression), and their fusion with the ``'linear'``
forward model.

    fwm = LinearForwardModel('covariates', design)            # [K x N]
    em = BinomialLogitErrorModel(ys, trials=None, offset=None)
    lik = Likelihood('outcomes', fwm, em)

The linear predictor is ``eta = mock + offset``; the term of one datum is that of
``csrc/glm_term.hpp`` (restated in ``tests/glm_ref.py``).  ``gradient`` follows
``GaussianErrorModel._evaluate_gradient``: that of MINUS the log density with respect to
the mock data.  The data-only constants -- ``sum log C(m_n, y_n)``, ``-sum lgamma(y_n + 1)``
-- are computed once here (``math.lgamma``, ``math.fsum``) and make the density the
normalised one: evidences (tempered SMC) and elpd (PSIS-LOO) are those of the model, not
of its kernel.

As written, the error models run ``binf_glm_pointwise_f64`` behind ANY forward model (the
polynomial, a user's own, a ``LinearForwardModel`` subclass that overrides ``_evaluate``).
Paired with an unchanged ``LinearForwardModel`` the likelihood's log-prob runs in
``binf_linear_glm_logp_f64``, its gradient in ``binf_linear_glm_grad_f64`` and
``HMCSampler._leapfrog`` in ``binf_linear_glm_leapfrog_f64`` -- the ``[C x n_data]`` mock
data never reaches HBM.  The log-prob hook declines shapes whose grid would leave most of the
chip idle (``logp_covers``: the as-written path is the faster launch there), so the choice --
and with it the last bits of a log-prob -- depends on the batch; callers that need a shard
to reproduce a batch bit for bit call ``_native.linear_glm_logp`` themselves.  Importing this module registers the kind ``'linear_glm'`` AFTER
``'linear'``, whose own recognition is consulted first and unchanged.  The
whole-transition and chain-resident tiers do not cover these models:
``LinearForwardModel(resident=True)`` behaves as without the flag.

Overdispersed counts: ``NegBinomialLogErrorModel(ys, offset=None)`` (NB2) has a second variable,
the per-chain ``log_dispersion``; its term is the binomial one at ``eta - log_dispersion`` with
``y + phi`` trials and runs in the same fused kernels (``binf_linear_negbin_*``), the rest of its
density is the count term of ``csrc/negbin.hip``.  The fused leapfrog is matched when
``log_dispersion`` is a fixed parameter of the likelihood, as inside a Gibbs conditional.
"""
import math

import numpy as np
import torch

from binf_amd import ArrayParameter, _native, native
from binf_amd.params import Parameter as _ScalarParameter
from binf_amd.model import linear as _linear
from binf_amd.model.errormodels import AbstractErrorModel

KIND = 'linear_glm'
BINOMIAL_LOGIT, POISSON_LOG, NEGBIN_LOG = 'binomial_logit', 'poisson_log', 'negbin_log'
FAMILIES = {BINOMIAL_LOGIT: _native.GLM_BINOMIAL_LOGIT, POISSON_LOG: _native.GLM_POISSON_LOG,
            NEGBIN_LOG: _native.GLM_NEGBIN_LOG}


def _as2d(x):
    return x if x.dim() == 2 else x.reshape(1, -1)


def _host(x, what, like=None):
    if x is None:
        return None
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    a = np.array(a, dtype=np.float64, order='C')        # the model's own copy
    if a.ndim == 0:
        a = a.reshape(1)
    if a.ndim != 1:
        raise ValueError('%s must be one-dimensional, got shape %s' % (what, a.shape))
    if like is not None and a.shape != like.shape:
        raise ValueError('%s has %d entries for %d observations' % (what, a.shape[0], like.shape[0]))
    if not np.all(np.isfinite(a)):
        raise ValueError('%s must be finite' % what)
    return a


class _GLMErrorModel(AbstractErrorModel):
    """What the families share: the variable ``mock_data`` (the negative binomial adds its
    dispersion); the data live on the host, their device copies are made when first needed
    and shared with clones."""

    kind = None                       # the name the model advertises (native_spec)

    def __init__(self, ys, trials=None, offset=None):
        super(_GLMErrorModel, self).__init__('error_model')
        self._dev = {}
        self._ys = _host(ys, 'ys')
        if np.any(self._ys < 0) or np.any(self._ys != np.floor(self._ys)):
            raise ValueError('ys must be non-negative integers (counts)')
        self._trials = _host(trials, 'trials', self._ys)
        self._offset = _host(offset, 'offset', self._ys)
        self._lconst = self._constants()
        self._log_norm = math.fsum(self._lconst)
        self._register_variable('mock_data')
        self.update_var_param_types(mock_data=ArrayParameter)
        self._register_family_variables()
        self._set_original_variables()

    def _register_family_variables(self):
        """Variables beside ``mock_data`` (the negative binomial's dispersion)."""

    # -- data -----------------------------------------------------------------
    @property
    def ys(self):
        return self._ys

    @property
    def trials(self):
        return self._trials

    @property
    def offset(self):
        return self._offset

    @property
    def family(self):
        return FAMILIES[self.kind]

    @property
    def log_norm(self):
        """The data-only constant of the log density, one host double."""
        return self._log_norm

    @property
    def pointwise_constants(self):
        """Its per-observation parts (host ``[N]``); ``log_norm`` is their ``math.fsum``."""
        return self._lconst

    def _device(self, key, host, device):
        if host is None:
            return None
        k = (key, device)
        if k not in self._dev:
            self._dev[k] = torch.from_numpy(host).to(device)
        return self._dev[k]

    def ys_device(self, device):
        return self._device('ys', self._ys, device)

    def trials_device(self, device):
        return self._device('trials', self._trials, device)

    def offset_device(self, device):
        return self._device('offset', self._offset, device)

    def lconst_device(self, device):
        return self._device('lconst', self._lconst, device)

    # -- model interface --------------------------------------------------------
    def _pointwise(self, mock_data, want_ll, want_grad):
        _native.require_device(mock_data, 'mock_data')
        dev = mock_data.device
        return _native.glm_pointwise(_as2d(mock_data).contiguous(), self.ys_device(dev),
                                     self.trials_device(dev), self.offset_device(dev), self.family,
                                     self.lconst_device(dev) if want_ll else None,
                                     want_ll=want_ll, want_grad=want_grad)

    def _evaluate_log_prob(self, mock_data):
        ll, _ = self._pointwise(mock_data, True, False)
        return _native.row_sum(ll)

    def _evaluate_gradient(self, mock_data):
        _, g = self._pointwise(mock_data, False, True)
        return g if mock_data.dim() == 2 else g.reshape(-1)

    def pointwise_log_prob(self, mock_data):
        """``[S x N]``: the log density of every datum under every row of ``mock_data``,
        its constant included (the record PSIS-LOO works on)."""
        return self._pointwise(mock_data, True, False)[0]

    def _clone_args(self):
        return (self._ys, self._trials, self._offset)

    def clone(self):
        copy = self.__class__(*self._clone_args())
        copy._dev = self._dev            # immutable model data: share it
        copy.set_fixed_variables_from_pdf(self)
        return copy

    def native_spec(self):
        base = _GLM_BASES[self.kind]
        if _linear._unchanged(self, base, ('_evaluate_log_prob', '_evaluate_gradient')):
            return (self.kind, self)
        return None


class BinomialLogitErrorModel(_GLMErrorModel):
    """``y_n`` successes of ``m_n`` trials with success probability ``logistic(eta_n)``:
    ``log p = sum_n [log C(m_n, y_n) + y_n eta_n - m_n softplus(eta_n)]``.  ``trials=None``:
    one trial each (binary outcomes)."""

    kind = BINOMIAL_LOGIT

    def __init__(self, ys, trials=None, offset=None):
        t = _host(trials, 'trials')
        y = _host(ys, 'ys')
        if t is not None:
            if t.shape != y.shape:
                raise ValueError('trials has %d entries for %d observations' % (t.shape[0], y.shape[0]))
            if np.any(t < 1) or np.any(t != np.floor(t)):
                raise ValueError('trials must be integers >= 1')
        if np.any(y > (1.0 if t is None else t)):
            raise ValueError('ys must not exceed trials')
        super(BinomialLogitErrorModel, self).__init__(ys, trials, offset)

    def _constants(self):
        m = np.ones_like(self._ys) if self._trials is None else self._trials
        return np.array([math.lgamma(mi + 1.0) - math.lgamma(yi + 1.0) - math.lgamma(mi - yi + 1.0)
                         for yi, mi in zip(self._ys, m)], dtype=np.float64)


class PoissonLogErrorModel(_GLMErrorModel):
    """Counts ``y_n`` with rate ``exp(eta_n)``: ``log p = sum_n [y_n eta_n - exp(eta_n) -
    lgamma(y_n + 1)]``.  ``offset``: the log exposure."""

    kind = POISSON_LOG

    def __init__(self, ys, offset=None):
        super(PoissonLogErrorModel, self).__init__(ys, None, offset)

    def _constants(self):
        return np.array([-math.lgamma(yi + 1.0) for yi in self._ys], dtype=np.float64)

    def _clone_args(self):
        return (self._ys, self._offset)


class NegBinomialLogErrorModel(_GLMErrorModel):
    """Overdispersed counts ``y_n`` (NB2): mean ``mu = exp(eta_n)``, variance ``mu + mu**2 /
    phi``.  With ``lam = log(phi)`` (the variable ``log_dispersion``) and ``z = eta - lam``,

        log p = sum_n [y_n z_n - (y_n + phi) softplus(z_n) + sum_{j<y_n} log(phi + j)
                       - lgamma(y_n + 1)]

    -- the binomial-logit term at ``z`` with ``y + phi`` trials, and a count term that holds
    no ``eta``: summed over the data it is ``sum_j T_j log(phi + j)`` with the integer tail
    counts ``T_j = #{n: y_n > j}`` (``tail_counts``), evaluated by
    ``binf_negbin_count_term_f64``.  ``offset``: the log exposure.

    ``log_dispersion`` is per chain: a ``[C]`` or ``[C x 1]`` device tensor, or a Python float
    shared by all chains (it must be finite).  The regular range is ``-708 <= lam <= 709``;
    a chain outside it has log-prob ``-inf``.  It is a variable like the Gaussian model's
    ``precision``: fix it (``fix_variables`` / ``conditional_factory``) to sample the
    coefficients given it, sample it by Metropolis given the coefficients
    (``RWMCSampler(variable='log_dispersion')``).  The count term is recomputed from the
    value at hand in every log-prob -- one small launch, no cache: a ``lam`` rewritten in
    place (a Gibbs sweep, a replayed graph) is always the one that is read.  Counts above
    ``2**20`` are refused."""

    kind = NEGBIN_LOG
    MAX_COUNT = _native.NEGBIN_MAX_COUNT

    def __init__(self, ys, offset=None):
        y = _host(ys, 'ys')
        if y.size and np.max(y) > self.MAX_COUNT:
            raise ValueError('counts above 2**20 are not covered by the negative-binomial '
                             'kernels (largest: %g)' % np.max(y))
        super(NegBinomialLogErrorModel, self).__init__(ys, None, offset)
        yi = self._ys.astype(np.int64)
        ymax = int(yi.max()) if yi.size else 0
        # T_j = #{n: y_n > j}, j = 0 .. ymax - 1
        hist = np.bincount(yi, minlength=ymax + 1)
        self._tail = (yi.size - np.cumsum(hist))[:ymax].astype(np.int64)
        self._values = np.unique(self._ys)
        self._index = np.searchsorted(self._values, self._ys).astype(np.int32)

    def _register_family_variables(self):
        self._register_variable('log_dispersion')
        self.update_var_param_types(log_dispersion=_ScalarParameter)

    def _constants(self):
        return np.array([-math.lgamma(yi + 1.0) for yi in self._ys], dtype=np.float64)

    def _clone_args(self):
        return (self._ys, self._offset)

    @property
    def tail_counts(self):
        """``T_j = #{n: y_n > j}`` for ``j = 0 .. max(ys) - 1`` (host int64)."""
        return self._tail

    @property
    def count_values(self):
        """The distinct values of ``ys``, ascending (host float64)."""
        return self._values

    def tail_device(self, device):
        if self._tail.size == 0:
            return None
        return self._device('tail', self._tail.astype(np.float64), device)

    def values_device(self, device):
        return self._device('values', self._values, device)

    def index_device(self, device):
        return self._device('index', self._index, device)

    def lam_device(self, log_dispersion, C, device):
        """``log_dispersion`` as the kernels' ``[C]`` tensor: the tensor's own storage where
        it already is one (a later in-place write is then seen by a replayed graph)."""
        if isinstance(log_dispersion, torch.Tensor):
            _native.require_device(log_dispersion, 'log_dispersion')
            lam = log_dispersion
            if lam.dim() > 2 or (lam.dim() == 2 and lam.shape[1] != 1):
                raise ValueError('log_dispersion must be [C], [C x 1] or a float, got shape %s'
                                 % (tuple(lam.shape),))
            lam = lam.reshape(-1)
            if lam.dtype != torch.float64:
                raise ValueError('log_dispersion must be float64 (got %s)' % lam.dtype)
            if lam.numel() == 1 and C != 1:
                lam = lam.expand(C)
            if lam.numel() != C:
                raise ValueError('log_dispersion has %d entries for %d chains' % (lam.numel(), C))
            return lam.contiguous()
        lam = float(log_dispersion)
        if not math.isfinite(lam):
            raise ValueError('log_dispersion must be finite (got %r)' % lam)
        return torch.full((C,), lam, dtype=torch.float64, device=device)

    def log_norm_chain(self, lam):
        """``[C]``: the count term under ``lam`` ``[C]`` plus ``log_norm``."""
        return _native.negbin_count_term(lam, self.tail_device(lam.device), self.log_norm)[0]

    def _nb_pointwise(self, mock_data, log_dispersion, want_ll, want_grad):
        _native.require_device(mock_data, 'mock_data')
        dev = mock_data.device
        mock = _as2d(mock_data).contiguous()
        lam = self.lam_device(log_dispersion, mock.shape[0], dev)
        prefix = index = lconst = None
        if want_ll and self._values.size:
            prefix = _native.negbin_count_term(lam, None, 0.0, values=self.values_device(dev),
                                               want_chain=False)[1]
            index, lconst = self.index_device(dev), self.lconst_device(dev)
        return _native.negbin_pointwise(mock, self.ys_device(dev), self.offset_device(dev), lam,
                                        prefix, index, lconst, want_ll=want_ll, want_grad=want_grad)

    def _evaluate_log_prob(self, mock_data, log_dispersion):
        ll, _ = self._nb_pointwise(mock_data, log_dispersion, True, False)
        return _native.row_sum(ll)

    def _evaluate_gradient(self, mock_data, log_dispersion):
        _, g = self._nb_pointwise(mock_data, log_dispersion, False, True)
        return g if mock_data.dim() == 2 else g.reshape(-1)

    def pointwise_log_prob(self, mock_data, log_dispersion):
        """``[S x N]``: the log density of every datum under row ``s`` of ``mock_data`` and
        ``log_dispersion[s]``, count term and constant included (PSIS-LOO's record)."""
        return self._nb_pointwise(mock_data, log_dispersion, True, False)[0]


_GLM_BASES = {BINOMIAL_LOGIT: BinomialLogitErrorModel, POISSON_LOG: PoissonLogErrorModel,
              NEGBIN_LOG: NegBinomialLogErrorModel}


# ---------------------------------------------------------------------------
# the kind: Likelihood hooks for (linear, binomial_logit) / (linear, poisson_log) and the
# fused leapfrog
# ---------------------------------------------------------------------------
# negbin_log: the binomial term's threshold carried over, not measured
LOGP_MIN_WORKGROUPS = {BINOMIAL_LOGIT: 256, POISSON_LOG: 128, NEGBIN_LOG: 256}


def logp_covers(kind, C, N):
    """Is the fused log-prob the faster launch for ``C`` chains and ``N`` data points?  Its
    grid is one workgroup per piece of 1024 data points and per 64 chains (128 from 4096
    chains on), and a workgroup walks its piece's 64 tiles one after the other: below one
    workgroup per CU the launch takes as long as a full chip's worth and the as-written
    path, which spreads the element-wise term over the whole chip, wins (DESIGN section 4.7:
    measured slower up to 128 workgroups for the binomial term, up to 64 for the Poisson
    one, faster from 256 / 128).  The hook declines those shapes rather than ship a slower
    default.  The gradient and the leapfrog were the faster launch at every measured shape."""
    pieces = max(1, -(-(-(-int(N) // 16)) // 64))
    per_group = 128 if C >= 4096 else 64
    return pieces * -(-int(C) // per_group) >= LOGP_MIN_WORKGROUPS[kind]


def _inputs(fwm, em, fwm_vars):
    """``(x, x2, A, ys, trials, offset)`` or None (evaluate the models as written)."""
    fwm_vars = dict(fwm_vars)
    fwm._complete_variables(fwm_vars)
    x = fwm_vars.get(fwm.variable)
    if not _linear._usable(x) or x.shape[-1] != fwm.design.shape[0] or \
            not isinstance(em, _GLMErrorModel) or fwm.design.shape[1] != em.ys.shape[0] or \
            em.ys.shape[0] < 1:
        return None
    x2 = _as2d(x).contiguous()
    dev = x.device
    return (x, x2, fwm.design_matrix(x2.shape[1], dev), em.ys_device(dev), em.trials_device(dev),
            em.offset_device(dev))


def log_prob(likelihood, fwm, em, fwm_vars, em_vars):
    args = _inputs(fwm, em, fwm_vars)
    if args is None:
        return None
    _, x2, A, ys, trials, offset = args
    if not logp_covers(em.kind, x2.shape[0], ys.shape[0]):
        return None
    return _native.linear_glm_logp(x2, A, ys, trials, offset, em.family, em.log_norm)


def gradient(likelihood, fwm, em, fwm_vars, em_vars):
    args = _inputs(fwm, em, fwm_vars)
    if args is None:
        return None
    x, x2, A, ys, trials, offset = args
    out = _native.linear_glm_grad(x2, A, ys, trials, offset, em.family)
    return out if x.dim() == 2 else out.reshape(-1)


def _is_glm_pair(likelihood):
    """Linear forward model + one of the two GLM error models, neither overridden?  Both
    are recognised by the kind they advertise."""
    fs = getattr(likelihood.forward_model, 'native_spec', lambda: None)()
    es = getattr(likelihood.error_model, 'native_spec', lambda: None)()
    return fs is not None and es is not None and fs[0] == _linear.KIND and es[0] in FAMILIES and \
        isinstance(es[1], _GLMErrorModel)


def posterior_leapfrog_spec(posterior, variable_name):
    """``(forward_model, error_model, prior)`` if the force on ``variable_name`` is exactly
    ONE linear + GLM likelihood and at most one isotropic Gaussian prior on the same
    variable -- recognised by the spec it advertises (``native_hmc_spec``), not by its
    class; ``prior`` is ``(k, x0)`` or None.  Every other component must have no
    differentiable variable.  Else None."""
    from binf_amd.pdf.likelihoods import Likelihood
    components = getattr(posterior, '_ordered_components', None)
    if components is None:
        return None
    lik, prior = None, None
    for f in components():
        if not (len(f.variables) > 0 and len(f.differentiable_variables) > 0):
            continue
        if set(f.variables) != {variable_name}:
            return None
        if isinstance(f, Likelihood):
            if lik is not None or not _is_glm_pair(f) or f.forward_model.variable != variable_name:
                return None
            lik = f
            continue
        spec = getattr(f, 'native_hmc_spec', lambda name: None)(variable_name)
        if prior is not None or spec is None or len(spec) != 3 or spec[0] != 'gauss':
            return None
        prior = (float(spec[1]), float(spec[2]))
    if lik is None or lik.forward_model.design.shape[0] > _linear.MAX_PARAMS or \
            lik.forward_model.design.shape[1] != lik.error_model.ys.shape[0] or \
            lik.error_model.ys.shape[0] < 1:
        return None
    # the negative binomial's dispersion must be a fixed parameter of the likelihood (as
    # inside a Gibbs conditional): the leapfrog reads its value at every call
    if lik.error_model.kind == NEGBIN_LOG and 'log_dispersion' not in lik.error_model.parameters:
        return None
    return (lik.forward_model, lik.error_model, prior)


def leapfrog(sampler, spec, q2, p2, dt, dtc, nsteps, mode, q_from):
    _, fwm, em, prior = spec
    if not (q2.is_cuda and q2.dtype == torch.float64 and q2.shape[1] <= _linear.MAX_PARAMS and
            q2.shape[1] == fwm.design.shape[0]):
        return False
    if q_from is not None:
        q2.copy_(q_from)
    dev = q2.device
    if em.kind == NEGBIN_LOG:
        lam = em.lam_device(em['log_dispersion'].value, q2.shape[0], dev)
        _native.linear_negbin_leapfrog(q2, p2, fwm.design_matrix(q2.shape[1], dev),
                                       em.ys_device(dev), em.offset_device(dev), lam, prior,
                                       dt, dtc, nsteps, mode)
        return True
    _native.linear_glm_leapfrog(q2, p2, fwm.design_matrix(q2.shape[1], dev), em.ys_device(dev),
                                em.trials_device(dev), em.offset_device(dev), em.family, prior,
                                dt, dtc, nsteps, mode)
    return True


def _negbin_inputs(fwm, em, fwm_vars, em_vars):
    """``_inputs`` and the chains' ``log_dispersion`` ``[C]`` (read from ``em_vars``, as
    model/linear.py reads ``precision``), or None."""
    args = _inputs(fwm, em, fwm_vars)
    em_vars = dict(em_vars)
    em._complete_variables(em_vars)
    if args is None or 'log_dispersion' not in em_vars or not hasattr(em, 'lam_device'):
        return None
    x2 = args[1]
    return args + (em.lam_device(em_vars['log_dispersion'], x2.shape[0], x2.device),)


def negbin_log_prob(likelihood, fwm, em, fwm_vars, em_vars):
    args = _negbin_inputs(fwm, em, fwm_vars, em_vars)
    if args is None:
        return None
    _, x2, A, ys, _, offset, lam = args
    if not logp_covers(em.kind, x2.shape[0], ys.shape[0]):
        return None
    return _native.linear_negbin_logp(x2, A, ys, offset, lam, em.log_norm_chain(lam))


def negbin_gradient(likelihood, fwm, em, fwm_vars, em_vars):
    args = _negbin_inputs(fwm, em, fwm_vars, em_vars)
    if args is None:
        return None
    x, x2, A, ys, _, offset, lam = args
    out = _native.linear_negbin_grad(x2, A, ys, offset, lam)
    return out if x.dim() == 2 else out.reshape(-1)


native.register(
    KIND, replace=True,
    match_leapfrog=posterior_leapfrog_spec, leapfrog=leapfrog,
    likelihood={(_linear.KIND, BINOMIAL_LOGIT): (log_prob, gradient),
                (_linear.KIND, POISSON_LOG): (log_prob, gradient),
                (_linear.KIND, NEGBIN_LOG): (negbin_log_prob, negbin_gradient)})
