"""
Model comparison by predictive fit, on the device: Pareto-smoothed importance-sampling
leave-one-out cross-validation (PSIS-LOO: Vehtari, Gelman & Gabry 2017; Vehtari, Simpson,
Gelman, Yao & Gabry 2024) with the Pareto-k^ diagnostic per observation, and WAIC as its
cross-check.  The companion of the evidence estimates (:mod:`binf_amd.free_energy`, tempered
SMC): which model PREDICTS held-out data best, and for which observations that estimate is
not to be trusted.

``log_lik`` is the pointwise log-likelihood record: any ``[S x N]`` or ``[T x C x N]`` fp64
device tensor with unit inner stride -- draw ``s`` (kept sweep ``t`` of chain ``c``),
observation ``i``.  :func:`pointwise_log_likelihood` builds it for a Gaussian error model;
the record of any other model, computed by the user, goes through :func:`loo` just the same.
Views are read through their strides; nothing is copied.  A sharded run diagnoses the
gathered record, as ``diagnostics.summary(store.gather())`` does: the result is then the
single-GPU result by construction.

The arithmetic is the HIP library's (``csrc/loo.hip``, contract in ``include/binf_hip.h``):
the record is sorted per observation by the rank layer (``binf_rank_normalise_f64``), the
generalised-Pareto fit, the smoothing and the log-sum-exps run in ``binf_psis_loo_f64``, and
the reductions over the observations in ``binf_pointwise_totals_f64``.  Every sum has one
fixed order and only the sorted values enter, so a result is reproducible bit for bit and
does not depend on the order of the draws, on the other observations in the call or on the
record's strides.  Read k^ as the `loo` package does: below 0.5 the estimate is reliable, up
to 0.7 usable, above it (``n_bad``) the observation is too influential for importance
sampling and its ``elpd_i`` should not be trusted.
"""
import math
from collections import namedtuple

from binf_amd import _native

KHAT_BAD = 0.7


def pointwise_log_likelihood(*args):
    """The pointwise log-likelihood record ``[S x N]`` of a Gaussian error model,
    ``-0.5 (mock[s, i] - ys[i])^2 precision[s] + 0.5 log precision[s] - 0.5 log 2 pi``
    (``binf_gauss_pointwise_loglik_f64``).  Two forms:

    ``pointwise_log_likelihood(mock, precision, ys)``: ``mock [S x N]``, ``precision [S]``,
    ``ys [N]`` device tensors.

    ``pointwise_log_likelihood(likelihood, samples)``: ``likelihood`` a
    :class:`binf_amd.pdf.likelihoods.Likelihood` with a Gaussian error model, ``samples`` what
    ``binf_amd.example.misc.predict_grid`` accepts (a sequence of ``BinfState`` or a pair
    ``(parameters [S x K], precision [S])``).  The forward model is evaluated for all samples at
    once -- the polynomial and the ``'linear'`` kind through their forward kernels, any other
    forward model as given.  With a binomial-logit or Poisson-log error model
    (``binf_amd/model/glm.py``) the record is that model's (``binf_glm_pointwise_f64``, the
    per-observation constants included) and ``samples`` may be a bare ``[S x K]`` tensor: there
    is no precision.  With the negative-binomial error model the record is
    ``binf_negbin_pointwise_f64``'s, count term and constants included, and ``samples`` is a pair
    ``(parameters [S x K], log_dispersion [S])`` or a sequence of ``BinfState``.
    An error model that advertises no known kind raises ``TypeError``:
    compute its ``[S x N]`` record yourself and pass it to :func:`loo`."""
    if len(args) == 3:
        mock, precision, ys = args
        _native.require_device(mock, 'mock')
        return _native.gauss_pointwise_loglik(mock, precision, ys, 0.5 * math.log(2.0 * math.pi))
    if len(args) != 2:
        raise TypeError('pointwise_log_likelihood(mock, precision, ys) or '
                        'pointwise_log_likelihood(likelihood, samples)')
    from binf_amd.example.misc import _samples_as_tensors
    likelihood, samples = args
    em = likelihood.error_model
    spec = getattr(em, 'native_spec', lambda: None)()
    if spec is not None and spec[0] in ('binomial_logit', 'poisson_log') and \
            hasattr(em, 'pointwise_log_prob'):
        return _glm_record(likelihood, em, samples)
    if spec is not None and spec[0] == 'negbin_log' and hasattr(em, 'pointwise_log_prob'):
        return _negbin_record(likelihood, em, samples)
    if spec is None or spec[0] != 'gaussian':
        raise TypeError('pointwise_log_likelihood: the error model %r is not the Gaussian one; '
                        'compute the [S x N] record of pointwise log-likelihoods yourself and '
                        'pass it to loo() directly' % type(em).__name__)
    parameters, precision = _samples_as_tensors(samples)
    mock = _forward(likelihood, parameters)
    return _native.gauss_pointwise_loglik(mock, precision, em.ys_device(mock.device).reshape(-1),
                                          0.5 * math.log(2.0 * math.pi))


def _forward(likelihood, parameters):
    fwm = likelihood.forward_model
    names = sorted(fwm.variables)
    if len(names) != 1:
        raise TypeError('pointwise_log_likelihood: the forward model must have exactly one free '
                        'variable (got %s)' % names)
    mock = fwm(**{names[0]: parameters})
    _native.require_device(mock, 'the forward model\'s mock data')
    return mock.reshape(parameters.shape[0], -1).contiguous()


def _glm_record(likelihood, em, samples):
    """The record of a binomial-logit or Poisson-log error model (``binf_amd/model/glm.py``):
    the forward kernel, then ``binf_glm_pointwise_f64`` with the per-observation constants.
    There is no precision: ``samples`` may be a bare ``[S x K]`` tensor."""
    import torch
    if isinstance(samples, torch.Tensor):
        _native.require_device(samples, 'samples')
        parameters = samples.reshape(-1, samples.shape[-1]).contiguous()
    elif isinstance(samples, tuple) and len(samples) == 2 and isinstance(samples[0], torch.Tensor):
        parameters = samples[0].reshape(-1, samples[0].shape[-1]).contiguous()
    else:
        if len(samples) == 0:
            raise ValueError('pointwise_log_likelihood: no samples')
        name = likelihood.forward_model.variable if hasattr(likelihood.forward_model, 'variable') \
            else sorted(likelihood.forward_model.variables)[0]
        cs = [s.variables[name] for s in samples]
        parameters = torch.cat([c.reshape(-1, c.shape[-1]) for c in cs], 0).contiguous()
    return em.pointwise_log_prob(_forward(likelihood, parameters))


def _negbin_record(likelihood, em, samples):
    """The record of the negative-binomial error model: the forward kernel, then
    ``binf_negbin_pointwise_f64`` with each sample's count-term prefix and the
    per-observation constants.  ``samples``: a pair ``(parameters [S x K], log_dispersion
    [S])`` or a sequence of ``BinfState`` with both variables (a dispersion fixed in the
    model serves states that lack it)."""
    import torch
    if isinstance(samples, tuple) and len(samples) == 2 and isinstance(samples[0], torch.Tensor):
        parameters = samples[0].reshape(-1, samples[0].shape[-1]).contiguous()
        lam = samples[1]
    else:
        if isinstance(samples, torch.Tensor) or len(samples) == 0:
            raise TypeError('pointwise_log_likelihood: the negative-binomial record needs '
                            '(parameters [S x K], log_dispersion [S]) or a sequence of states')
        name = likelihood.forward_model.variable if hasattr(likelihood.forward_model, 'variable') \
            else sorted(likelihood.forward_model.variables)[0]
        cs = [s.variables[name] for s in samples]
        parameters = torch.cat([c.reshape(-1, c.shape[-1]) for c in cs], 0).contiguous()
        if all('log_dispersion' in s.variables for s in samples):
            ls = [s.variables['log_dispersion'] for s in samples]
            lam = torch.cat([em.lam_device(l, c.reshape(-1, c.shape[-1]).shape[0], parameters.device)
                             for l, c in zip(ls, cs)], 0).contiguous()
        elif 'log_dispersion' in em.parameters:
            lam = em['log_dispersion'].value
        else:
            raise TypeError('pointwise_log_likelihood: the states hold no log_dispersion')
    return em.pointwise_log_prob(_forward(likelihood, parameters), lam)


def _as_draws(log_lik):
    import torch
    if not isinstance(log_lik, torch.Tensor):
        raise TypeError('log_lik must be a torch.Tensor')
    if log_lik.dim() == 2:
        log_lik = log_lik.unsqueeze(1)
    if log_lik.dim() != 3:
        raise ValueError('log_lik must be [S x N] or [T x C x N] (got %d dimensions)' % log_lik.dim())
    return log_lik


def _pointwise(log_lik):
    """The per-observation outputs of ``binf_psis_loo_f64`` for a record."""
    draws = _as_draws(log_lik)
    sorted_ll = _native.rank_normalise(draws, 1, want_sorted=True)[0]
    return _native.psis_loo(sorted_ll)


def _se(ssq, n):
    """``sqrt(N var)`` with the sample variance (``n - 1``), as the `loo` package's."""
    return math.sqrt(n * ssq / (n - 1)) if n > 1 else float('nan')


def _names(n, names):
    return ['[%d]' % i for i in range(n)] if names is None else list(names)


class LOOResult(namedtuple('LOOResult', 'elpd se p_loo n_bad elpd_i khat n_eff tail_len')):
    """Scalars (host floats, read back once): ``elpd`` = sum of ``elpd_i``, its standard error
    ``se = sqrt(N var_i elpd_i)``, the effective number of parameters ``p_loo = sum lppd_i -
    elpd`` and ``n_bad``, the number of observations with ``khat > 0.7``.  ``[N]`` device
    tensors: ``elpd_i``, ``khat`` (+inf where the tail was too short or flat to fit),
    ``n_eff`` of the smoothed weights and ``tail_len`` (int32)."""
    __slots__ = ()

    def table(self, names=None):
        """The result as text, one row per observation (moves the tensors to the host)."""
        e, k, n = self.elpd_i.cpu(), self.khat.cpu(), self.n_eff.cpu()
        N = int(e.shape[0])
        names = _names(N, names)
        width = max([4] + [len(s) for s in names])
        rows = ['%-*s %12s %8s %12s' % (width, 'obs', 'elpd_loo', 'khat', 'n_eff')]
        for i in range(N):
            rows.append('%-*s %12.5g %8.3f%s %11.1f' % (width, names[i], float(e[i]), float(k[i]),
                                                        '!' if float(k[i]) > KHAT_BAD else ' ', float(n[i])))
        rows.append('elpd_loo %.5g +- %.3g   p_loo %.4g   khat > %.1f: %d of %d'
                    % (self.elpd, self.se, self.p_loo, KHAT_BAD, self.n_bad, N))
        return '\n'.join(rows)

    def __str__(self):
        return self.table()


class WAICResult(namedtuple('WAICResult', 'elpd se p_waic lppd_i p_waic_i')):
    """``elpd = sum_i (lppd_i - p_waic_i)`` with its standard error, ``p_waic = sum_i p_waic_i``
    (host floats), and the ``[N]`` device tensors ``lppd_i`` (log pointwise predictive density)
    and ``p_waic_i`` (posterior variance of the log-likelihood)."""
    __slots__ = ()

    def table(self, names=None):
        """The result as text, one row per observation (moves the tensors to the host)."""
        l, p = self.lppd_i.cpu(), self.p_waic_i.cpu()
        N = int(l.shape[0])
        names = _names(N, names)
        width = max([4] + [len(s) for s in names])
        rows = ['%-*s %12s %12s %12s' % (width, 'obs', 'elpd_waic', 'lppd', 'p_waic')]
        for i in range(N):
            rows.append('%-*s %12.5g %12.5g %12.4g' % (width, names[i], float(l[i]) - float(p[i]),
                                                       float(l[i]), float(p[i])))
        rows.append('elpd_waic %.5g +- %.3g   p_waic %.4g' % (self.elpd, self.se, self.p_waic))
        return '\n'.join(rows)

    def __str__(self):
        return self.table()


def loo(log_lik):
    """:class:`LOOResult` of the record ``log_lik``: a sort per observation, the PSIS kernels
    and one reduction over the observations, all on the device; four numbers are read back."""
    import torch
    r = _pointwise(log_lik)
    N = int(r['elpd_loo'].shape[0])
    tot = _native.pointwise_totals(torch.stack((r['elpd_loo'], r['lppd'])), khat=r['khat'],
                                   threshold=KHAT_BAD).cpu()
    elpd = float(tot[0])
    return LOOResult(elpd, _se(float(tot[1]), N), float(tot[2]) - elpd, int(tot[4]), r['elpd_loo'],
                     r['khat'], r['n_eff'], r['tail_len'])


def waic(log_lik):
    """:class:`WAICResult` of the record ``log_lik``, from the same path as :func:`loo`."""
    import torch
    r = _pointwise(log_lik)
    N = int(r['lppd'].shape[0])
    zero = torch.zeros_like(r['lppd'])
    # rows: lppd_i - p_waic_i (elpd and its spread), p_waic_i - 0
    tot = _native.pointwise_totals(torch.stack((r['lppd'], r['p_waic'])),
                                   torch.stack((r['p_waic'], zero))).cpu()
    return WAICResult(float(tot[0]), _se(float(tot[1]), N), float(tot[2]), r['lppd'], r['p_waic'])


def compare(a, b):
    """``(elpd_diff, se_diff)`` of two results over the SAME observations (:class:`LOOResult` or
    :class:`WAICResult`, or two ``[N]`` device tensors of pointwise elpd): the sum of the
    pointwise differences ``a_i - b_i`` and ``sqrt(N var_i (a_i - b_i))``.  Positive: ``a``
    predicts better.  The differences are paired, so ``se_diff`` is usually far smaller than
    either model's own ``se``."""
    def pointwise(r):
        if isinstance(r, LOOResult):
            return r.elpd_i
        if isinstance(r, WAICResult):
            return r.lppd_i - r.p_waic_i
        return r
    x, y = pointwise(a), pointwise(b)
    _native.require_device(x, 'a')
    _native.require_device(y, 'b')
    if x.dim() != 1 or x.shape != y.shape:
        raise ValueError('compare: two results over the same observations are needed (got %s and %s)'
                         % (tuple(x.shape), tuple(y.shape)))
    tot = _native.pointwise_totals(x.reshape(1, -1).contiguous(), y.reshape(1, -1).contiguous()).cpu()
    return float(tot[0]), _se(float(tot[1]), int(x.shape[0]))
