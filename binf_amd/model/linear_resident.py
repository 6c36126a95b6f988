"""
The kind ``'linear_resident'``: whole HMC transitions and whole Gibbs sweeps of a
:class:`~binf_amd.model.linear.LinearForwardModel` built with ``resident=True`` in ONE
launch (``binf_hmc_sample_linear_f64``, ``binf_gibbs_linear_sample_n_f64``;
``csrc/linear_chain_kernel.hpp``), the chain's state on chip between the sweeps.

Reference path: ``HMCSampler.sample`` (``binf/samplers/hmc.py:136-164``) and the Gibbs
sweep (``binf/samplers/gibbs.py:136-151``) around ``Likelihood.log_prob`` / ``gradient``
(``binf/pdf/likelihoods.py:141-155``) of a linear forward model
(``binf/model/forwardmodels.py:23-33``).

What is recognised is what the polynomial kind recognises for the example's model, with
the resident linear model in its place:

``match_hmc``  one linear + Gaussian-error likelihood with its precision fixed, at most
               one ``GaussianPrior`` on the variable (energy only, quirk Q4), components
               without free variables before and at most one after;
``gibbs``      variables ``coefficients`` and ``precision``, likelihood ``'points'``,
               ``HMCSampler`` or ``RWMCSampler`` plus ``GammaSampler``, draws all from a
               ``DeviceRNG`` or all from the host legacy stream.

The recognition, the draw sources, adaption and the samplers' bookkeeping are not
written twice: the module that defines those priors and samplers registers them with
``binf_amd.native`` under ``'chain_resident'`` (extras, parametrised by a ``ChainModel``),
and this module asks the registry.  The priors, the error model and the samplers such a
posterior is made of come from that module, so wherever a posterior to recognise
exists, the machinery is registered; where it is not, the hooks decline.

The kind ``'linear'`` is untouched: a model without the flag, a shape the kernel does
not cover (the library is asked: ``binf_linear_resident_supported``) and a batch beyond
``RESIDENT_MAX_WORK`` all run the per-step path and give its results.
"""
import torch

from binf_amd import _native, native
from binf_amd.model import linear as _linear

KIND = 'linear_resident'

# chains x data points x coefficients up to which the resident kernel is the launch to
# take (see covers).  Measured crossover against the per-step path, one MI355X
# (scripts/probe_linear_resident.py, profiles/r06_r_probe_linear_resident.json;
# per-step time / resident time per transition, L = 20):
#   K = 8,  N = 512:   3.0 at 1.7e7,  0.89 at 6.7e7,  0.51 at 2.7e8
#   K = 16, N = 1024:  5.5 at 4.2e6,  1.09 at 6.7e7,  0.41 at 2.7e8
#   K = 9,  N = 200:   5.3 at 7.4e6,  0.64 at 1.2e8
#   K = 4,  N = 20:    25 at 3.3e5,   4.7 at 5.2e6,   2.0 at 2.1e7
# The two paths meet between 5e7 and 7e7; the threshold sits on the per-step side of
# that, where the resident path was still at least twice as fast in every row.
RESIDENT_MAX_WORK = 3.0e7


def _is_resident_pair(likelihood):
    """A linear forward model that opted in + a Gaussian error model, neither overridden?"""
    return _linear._is_linear_pair(likelihood) and \
        bool(getattr(likelihood.forward_model, 'resident', False)) and \
        hasattr(likelihood.error_model, 'ys_device')


def _shape_ok(fwm, n_data):
    K, N = fwm.design.shape
    return N == n_data and _native.linear_resident_supported(K, N)


def covers(sampler, spec, D, C=None):
    """Is the resident kernel the right launch for ``D`` coefficients (and, when given,
    ``C`` chains)?  ``sampler.fused_transition``: False = never, ``'always'`` = wherever
    the kernel covers the shape, anything else = up to ``RESIDENT_MAX_WORK``."""
    mode = getattr(sampler, 'fused_transition', True)
    K, N = spec[1].design.shape
    if not mode or D != K or not _native.linear_resident_supported(K, N):
        return False
    if C is not None and mode != 'always' and float(C) * N * K > RESIDENT_MAX_WORK:
        # the resident kernel wins while the batch is launch-bound; a batch this large
        # fills the chip on the per-step tier, whose force runs on the MFMA pipe
        return False
    return True


def _shared():
    """The registered chain-resident machinery (a dict of callables), or None."""
    k = native.get('chain_resident')
    return k.extras if k is not None else None


def _same_model(a, b, K, dev):
    return a.design.shape == b.design.shape and \
        _shared()['same_data'](a.design_matrix(K, dev), b.design_matrix(K, dev))


_MODEL = None


def model():
    """The ``ChainModel`` of this kind, built on first use."""
    global _MODEL
    if _MODEL is None:
        _MODEL = _shared()['ChainModel'](
            KIND, None, _is_resident_pair, shape_ok=_shape_ok,
            data=lambda fwm, K, dev: fwm.design_matrix(K, dev), same_model=_same_model,
            hmc_launch=lambda *a, **k: _native.hmc_sample_linear(*a, **k),
            gibbs_launch=lambda *a, **k: _native.gibbs_linear_sample_n(*a, **k),
            covers=covers, lane_layout=lambda sampler, spec, C: False, rwmc_covers=covers)
    return _MODEL


def match_hmc(posterior, variable_name):
    shared = _shared()
    if shared is None:
        return None
    spec = shared['posterior_hmc_spec'](posterior, variable_name, model())
    return None if spec is None else tuple(spec[1:])


def hmc_sample(sampler, spec, q0, p0, u, accepted, adapt):
    if not (q0.is_cuda and q0.dtype == torch.float64):
        raise ValueError('linear_resident: the state must be an fp64 tensor in GPU memory')
    return _shared()['hmc_sample'](sampler, spec, q0, p0, u, accepted, adapt, model())


def hmc_n(sampler, spec, n, thin, p0, u, record, out, q0, shape):
    return _shared()['hmc_n'](sampler, spec, n, thin, p0, u, record, out, q0, shape, model())


def gibbs_sample_n(gibbs, n, thin, record):
    shared = _shared()
    if shared is None:
        return False, None
    return shared['gibbs_sample_n'](gibbs, n, thin, record, model())


native.register(KIND, replace=True, match_hmc=match_hmc, covers=covers, hmc=hmc_sample,
                hmc_n=hmc_n, gibbs=gibbs_sample_n)
