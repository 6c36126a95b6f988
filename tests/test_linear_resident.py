"""CPU tests of the opt-in chain-resident path of a linear forward model
(``LinearForwardModel(..., resident=True)``, kind ``'linear_resident'``,
``binf_amd/model/linear_resident.py``): registration, recognition, the flag's
bookkeeping, the grown C ABI and its host-side refusals (csrc/chain_common.hpp: the checks
it shares with the polynomial kind, which walks the same table here).  No kernel is launched here;
the kernels are tested in tests/test_gpu_linear_resident.py."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from binf_amd import _native, native
from binf_amd.example.likelihood import GaussianErrorModel
from binf_amd.example.priors import GammaPrior, GaussianPrior
from binf_amd.model import linear, linear_resident
from binf_amd.model.linear import LinearForwardModel
from binf_amd.pdf.likelihoods import Likelihood
from binf_amd.pdf.posteriors import Posterior


class Fourier(LinearForwardModel):
    """A user's model with its own constructor: the flag is one more keyword of it."""

    def __init__(self, xs, n_modes, resident=False):
        self.xs, self.n_modes = np.asarray(xs, dtype=np.float64), n_modes
        rows = [np.ones_like(self.xs)]
        for m in range(1, n_modes + 1):
            rows += [np.cos(m * self.xs), np.sin(m * self.xs)]
        super(Fourier, self).__init__('fourier', np.vstack(rows), resident=resident)


class _Overridden(LinearForwardModel):
    def _evaluate(self, coefficients):
        return coefficients @ self.design_matrix(coefficients.shape[-1], coefficients.device)


def _likelihood(K=4, N=20, cls=LinearForwardModel, **kw):
    A = np.random.RandomState(0).standard_normal((K, N))
    ys = np.random.RandomState(1).standard_normal(N)
    return Likelihood('points', cls('basis', A, **kw), GaussianErrorModel(ys))


def _posterior(lik, K, gaussian=True):
    priors = {'precision_prior': GammaPrior(1.0, 0.2)}
    if gaussian:
        priors['coefficients_prior'] = GaussianPrior(np.zeros(K), np.full(K, 5.0))
    return Posterior({lik.name: lik}, priors)


def test_the_kind_is_registered_and_the_linear_kind_is_unchanged():
    k = native.get('linear_resident')
    assert k is not None and k.name == linear_resident.KIND == 'linear_resident'
    for hook in ('match_hmc', 'covers', 'hmc', 'hmc_n', 'gibbs'):
        assert callable(getattr(k, hook)), hook
    assert k.match_leapfrog is None and not k.likelihood        # those stay the kind 'linear''s
    lin = native.get('linear')
    assert lin.hmc is None and lin.hmc_n is None and lin.gibbs is None
    assert lin.match_leapfrog is linear.posterior_leapfrog_spec


def test_recognition_needs_the_flag_and_a_covered_shape():
    plain = _posterior(_likelihood(), 4).conditional_factory(precision=2.5)
    assert plain.native_hmc_spec('coefficients') is None
    flagged = _posterior(_likelihood(resident=True), 4).conditional_factory(precision=2.5)
    spec = flagged.native_hmc_spec('coefficients')
    assert spec is not None and spec[0] == 'linear_resident' and spec[3] == 2.5
    assert spec[1].resident and spec[1].native_spec() == ('linear', spec[1])
    assert spec[4] is not None and spec[5] is True          # 'coefficients_prior' < 'points'
    assert flagged.native_hmc_spec('precision') is None
    # the fused leapfrog of the kind 'linear' is still offered for the same object
    assert flagged.native_leapfrog_spec('coefficients')[0] == 'linear'
    # no Gaussian prior
    bare = _posterior(_likelihood(resident=True), 4, gaussian=False).conditional_factory(precision=2.5)
    assert bare.native_hmc_spec('coefficients')[4] is None
    # shapes at the limits are covered ...
    for K, N in ((16, 128), (16, 1024), (1, 1), (9, 200), (5, 920)):
        post = _posterior(_likelihood(K, N, resident=True), K).conditional_factory(precision=1.5)
        assert post.native_hmc_spec('coefficients') is not None, (K, N)
    # ... and beyond them, with an overridden model or a free precision, declined
    for K, N in ((17, 20), (4, 2000)):
        post = _posterior(_likelihood(K, N, resident=True), K).conditional_factory(precision=1.5)
        assert post.native_hmc_spec('coefficients') is None, (K, N)
        assert post.native_leapfrog_spec('coefficients')[0] == 'linear'
    over = _posterior(_likelihood(cls=_Overridden, resident=True), 4).conditional_factory(precision=2.5)
    assert over.native_hmc_spec('coefficients') is None
    assert _posterior(_likelihood(resident=True), 4).native_hmc_spec('coefficients') is None
    # another variable name is the model's own
    A = np.random.RandomState(0).standard_normal((4, 20))
    lik = Likelihood('points', LinearForwardModel('w', A, variable='weights', resident=True),
                     GaussianErrorModel(np.zeros(20)))
    post = Posterior({'points': lik}, {'precision_prior': GammaPrior(1.0, 0.2)})
    cond = post.conditional_factory(precision=2.0)
    assert cond.native_hmc_spec('weights')[0] == 'linear_resident'
    assert cond.native_hmc_spec('coefficients') is None


def test_covers_asks_the_library_and_the_threshold():
    class S(object):
        fused_transition = True
    cond = _posterior(_likelihood(9, 200, resident=True), 9).conditional_factory(precision=2.5)
    spec = cond.native_hmc_spec('coefficients')
    s = S()
    assert linear_resident.covers(s, spec, 9) and linear_resident.covers(s, spec, 9, 4096)
    assert not linear_resident.covers(s, spec, 8, 4096)               # not this model's state
    big = int(linear_resident.RESIDENT_MAX_WORK / (9 * 200)) + 1
    assert not linear_resident.covers(s, spec, 9, big)
    s.fused_transition = 'always'
    assert linear_resident.covers(s, spec, 9, big)
    s.fused_transition = False
    assert not linear_resident.covers(s, spec, 9, 4)
    # the limits are the library's
    L = _native.lib()
    for K, N, want in ((1, 0, 1), (16, 1024, 1), (17, 8, 0), (0, 8, 0), (4, 1025, 0), (4, 2000, 0),
                       (4, 920, 1), (4, -1, 0)):
        assert L.binf_linear_resident_supported(K, N) == want, (K, N)
        assert _native.linear_resident_supported(K, N) == bool(want)
    for N in range(0, 1025, 7):
        assert _native.linear_resident_supported(3, N) == (_native.pairwise_tree_height(N) <= 3)


def test_the_flag_survives_clone_and_conditional_factory():
    f = LinearForwardModel('basis', np.ones((3, 5)), resident=True)
    assert f.resident and f.clone().resident and type(f.clone()) is LinearForwardModel
    assert not LinearForwardModel('basis', np.ones((3, 5))).resident
    assert not LinearForwardModel('basis', np.ones((3, 5))).clone().resident
    u = Fourier(np.linspace(0, 6, 30), 3, resident=True)
    uc = u.clone()
    assert type(uc) is Fourier and uc.resident and uc.n_modes == 3 and uc._dev is u._dev
    assert not Fourier(np.linspace(0, 6, 30), 3).clone().resident
    lik = Likelihood('points', u, GaussianErrorModel(np.zeros(30)))
    for cond in (lik.conditional_factory(precision=2.0), lik.conditional_factory(coefficients=np.zeros(7)),
                 lik.clone()):
        assert type(cond.forward_model) is Fourier and cond.forward_model.resident
    post = _posterior(lik, 7).conditional_factory(precision=2.0)
    assert post.likelihoods['points'].forward_model.resident
    assert post.native_hmc_spec('coefficients')[0] == 'linear_resident'


def test_the_new_symbols_are_exported_and_bound():
    raw = ctypes.CDLL(_native.LIB_PATH)
    for name in ('binf_linear_resident_supported', 'binf_hmc_sample_linear_f64',
                 'binf_gibbs_linear_sample_n_f64'):
        assert hasattr(raw, name) and name in _native.SIGNATURES
    assert _native.ABI_VERSION == 7 and _native.lib().binf_abi_version() == 7
    assert callable(_native.hmc_sample_linear) and callable(_native.gibbs_linear_sample_n)
    assert _native.SIGNATURES['binf_hmc_sample_linear_f64'] == _native.SIGNATURES['binf_hmc_sample_poly_f64']
    # the argument block is the polynomial one with `design` where `xs` was
    a = [n for n, _ in _native.GibbsLinearArgs._fields_]
    b = [n for n, _ in _native.GibbsPolyArgs._fields_]
    assert [n if n != 'design' else 'xs' for n in a] == b and 'design' in a
    assert ctypes.sizeof(_native.GibbsLinearArgs) == ctypes.sizeof(_native.GibbsPolyArgs)


def test_the_ctypes_mirror_matches_the_header():
    """binf_gibbs_linear_args is passed by pointer: size and every offset against the
    header, through the host compiler."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = [n for n, _ in _native.GibbsLinearArgs._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "binf_hip.h"\nint main(void) {\n'
           '  printf("%zu\\n", sizeof(binf_gibbs_linear_args));\n' +
           ''.join('  printf("%%zu\\n", offsetof(binf_gibbs_linear_args, %s));\n' % f for f in fields) +
           '  return 0;\n}\n')
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, 'm.c'), os.path.join(d, 'm')
        with open(c, 'w') as fh:
            fh.write(src)
        cc = os.environ.get('CC', 'cc')
        subprocess.check_call([cc, '-I', os.path.join(root, 'include'), c, '-o', exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got[0] == ctypes.sizeof(_native.GibbsLinearArgs)
    assert got[1:] == [getattr(_native.GibbsLinearArgs, f).offset for f in fields]


# the two kinds behind the one host path: Gibbs block and entry, HMC entry, name of the model's buffer
_KINDS = {'linear': (_native.GibbsLinearArgs, 'binf_gibbs_linear_sample_n_f64', 'binf_hmc_sample_linear_f64',
                     'design'),
          'poly': (_native.GibbsPolyArgs, 'binf_gibbs_poly_sample_n_f64', 'binf_hmc_sample_poly_f64', 'xs')}


def _gibbs_args(kind='linear', **over):
    base = 1 << 40
    block, _, _, model = _KINDS[kind]
    a = block()
    a.struct_size = ctypes.sizeof(a)
    for i, n in enumerate(('coefficients', 'precision', 'coefficients_out', 'precision_out', model, 'ys')):
        setattr(a, n, base + (i << 32))
    a.C, a.K, a.N, a.n, a.thin, a.nsteps = 4, 5, 200, 3, 1, 10
    a.gp_shape, a.gamma_shape, a.timestep = 1.0, 100.0, 0.1
    a.move, a.mode = _native.MOVE_HMC, _native.MODE_EXACT
    for k, v in over.items():
        setattr(a, model if k == 'design' else k, v)
    return a


@pytest.mark.parametrize('kind', ['linear', 'poly'])
def test_refusals_without_gpu(kind):
    """Every refusal is made on the host before any launch: the fake pointers are never
    dereferenced (there is no GPU to launch on here).  One validator stands behind the
    linear and the polynomial entry points, so both walk the same table (`design` is the
    polynomial's `xs`)."""
    L = _native.lib()
    block, gibbs_entry, hmc_entry, _ = _KINDS[kind]
    gibbs = getattr(L, gibbs_entry)
    call = lambda a: gibbs(ctypes.byref(a), None)
    args = lambda **over: _gibbs_args(kind, **over)
    base = 1 << 40
    assert call(args(K=17)) == _native.E_UNSUPPORTED and '17' in _native.last_error()
    assert call(args(N=2000)) == _native.E_UNSUPPORTED and '2000' in _native.last_error()
    assert call(args(N=1023)) == _native.E_UNSUPPORTED        # a tree of height 4
    assert call(args(struct_size=8)) == _native.E_ARG and 'struct_size' in _native.last_error()
    assert call(args(struct_size=ctypes.sizeof(block) + 8)) == _native.E_ARG
    assert gibbs(None, None) == _native.E_ARG
    # overlapping buffers: an output may be exactly its input, nothing else
    assert call(args(coefficients_out=base + 8)) == _native.E_ALIAS
    assert call(args(precision_out=base + (1 << 32) + 8)) == _native.E_ALIAS
    assert call(args(precision_out=base + 16)) == _native.E_ALIAS
    # generated gamma variates need shape >= 1; supplied ones do not
    assert call(args(gamma_shape=0.5)) == _native.E_UNSUPPORTED
    assert call(args(gamma_shape=0.0)) == _native.E_ARG
    for bad in (dict(n=0), dict(thin=0), dict(move=2), dict(mode=16), dict(nsteps=0), dict(gp_where=3),
                dict(chain_offset=-1), dict(design=None), dict(prior_means=base + (9 << 32)),
                dict(n_adapt=1)):
        assert call(args(**bad)) == _native.E_ARG, bad
    # every message names its own entry point
    assert _native.last_error().startswith('gibbs_%s: ' % kind)
    # nothing to do is not an error
    assert call(args(C=0, coefficients=None, precision=None, coefficients_out=None,
                     precision_out=None, design=None, ys=None)) == 0

    q0, p0, u, qo, acc, A, ys = (base + (i << 32) for i in range(7))

    def hmc(q_out=qo, K=5, N=200, C=4, mode=_native.MODE_EXACT, nsteps=10, dt_chain=None, adapt=0,
            design=A):
        return getattr(L, hmc_entry)(q0, p0, u, q_out, acc, None, None, None, design, ys, 1.0, None,
                                     None, None, 0, None, None, 0.1, dt_chain, C, K, N, nsteps, adapt,
                                     1.05, 0.95, mode, None)
    assert hmc(K=17) == _native.E_UNSUPPORTED and '17' in _native.last_error()
    assert hmc(N=2000) == _native.E_UNSUPPORTED
    assert hmc(q_out=q0 + 8) == _native.E_ALIAS and hmc(q_out=p0) == _native.E_ALIAS
    if kind == 'linear':
        assert hmc(mode=_native.MODE_LANE_PER_CHAIN) == _native.E_ARG       # no such layout here
        assert hmc(mode=_native.MODE_LANE_PER_CHAIN, C=0) == _native.E_ARG
    else:
        # the polynomial entry knows the layout: it is a flag beside the mode, for n_data <= 128
        assert hmc(mode=_native.MODE_LANE_PER_CHAIN) == _native.E_UNSUPPORTED
        assert '128' in _native.last_error()
        assert hmc(mode=_native.MODE_LANE_PER_CHAIN | _native.MODE_FMA, N=128, C=0) == 0
        assert hmc(mode=_native.MODE_LANE_PER_CHAIN | 2, N=128) == _native.E_ARG
    assert hmc(mode=2) == _native.E_ARG
    assert hmc(nsteps=0) == _native.E_ARG and hmc(adapt=1) == _native.E_ARG
    assert hmc(design=None) == _native.E_ARG and hmc(C=-1) == _native.E_ARG
    assert _native.last_error().startswith('hmc_sample_%s: ' % kind)
    assert hmc(C=0) == 0
