"""Every device draw stream against its LAW (tests/draw_laws.py): statistics with known null
laws at a total level of 1e-9 per test function, fixed seeds, every setting read from
``draw_laws.CASES`` -- the table whose power tests/test_draw_laws.py shows on the CPU.

Every check reads the device array.  The host supplies the intervals and, for the ziggurat's
slow paths, each element's first candidate (layer, sign, slow or not) from the generator's words
alone -- never from the slow-path code under test.  No interval comes from device output.

tests/test_gpu_draw_streams.py pins the same streams to the restatement bit for bit; this file is
about whether both draw from the right distribution.  The law checks of tests/test_gpu_rng.py
(``test_moments``, ``test_ziggurat_normals``, ``test_fused_generator_stream_properties``: moments
at hand-set thresholds, KS at 1 %, correlation coefficients) are superseded by these and stay.

Each test prints every statistic with its interval; the figures of a run on an MI355X are in
HISTORY.md.
"""
import numpy as np
import pytest
import torch

import draw_laws as L
import draw_streams as ds
from binf_amd import _native

pytestmark = pytest.mark.gpu


def fill(kind, n, seed, offset, device, e0=0, shape=None):
    out = torch.empty(n, dtype=torch.float64, device=device)
    _native.rng_fill(kind, out, seed, offset, shape=shape, elem_offset=e0)
    return out


def hold(name, checks):
    print('case %s, level per statistic %.3g' % (name, L.alpha_of(name)))
    for c in checks:
        print('    ' + L.describe(c) + '   margin %.2f' % L.margin_of(c))
    bad = [L.describe(c) for c in checks if not L.inside(c)]
    assert not bad, bad


def test_ziggurat_slow_paths(device):
    """rng_fill('normal_zig'): the elements whose first candidate failed the fast test against
    their conditional law (wedge mixture per layer and sign; the tail), how many of them stayed
    inside their candidate's wedge, their number, and the tail values' signs."""
    c = L.CASES['zig_slow']
    z = fill('normal_zig', c['n'], c['seed'], c['offset'], device, c['e0']).cpu().numpy()
    d = ds.zig_stream(c['seed'], c['offset'], c['e0'], c['n'])
    hold('zig_slow', L.evaluate('zig_slow', (z,), d))


def test_ziggurat_whole_stream(device):
    """2^26 elements, sorted and transformed on the device: DKW of Phi(z) (threshold below 4.3e-4),
    the counts of z > R, z < -R, |z| > 5, z > 0 in exact binomial intervals, independence of the
    elements 2g / 2g+1 and e / e+2, of the offsets o / o+1 and of the seeds s / s+1."""
    c = L.CASES['zig_whole']
    z, z_off, z_seed = (fill('normal_zig', c['n'], c['seed'] + ks, c['offset'] + ko, device, c['e0'])
                        for ks, ko in ((0, 0), (0, 1), (1, 0)))
    hold('zig_whole', L.evaluate('zig_whole', (z, z_off, z_seed)))


@pytest.mark.parametrize('name', L.cases_of('lanes'))
def test_lane_generators(device, name):
    """hmc_gauss_rng_draws (two transitions of one launch) and hmc_gauss_big_rng_draws (two calls,
    offset and offset + 1): the slow paths against their conditional law with the classification
    from the lane streams, DKW of the whole, independence of neighbouring lanes, of a lane's
    successive draws, of neighbouring chains and transitions and of each chain's acceptance uniform
    against its first momentum element; the uniforms' own DKW and range."""
    c = L.CASES[name]
    if c['stream'] == 'fused':
        p, u = _native.hmc_gauss_rng_draws(c['n'], c['C'], c['D'], c['seed'], c['offset'], device,
                                           chain_offset=c['chain_offset'])
    else:
        calls = [_native.hmc_gauss_big_rng_draws(c['C'], c['D'], c['seed'], c['offset'] + k, device,
                                                 chain_offset=c['chain_offset']) for k in range(c['n'])]
        p, u = torch.stack([a for a, _ in calls]), torch.stack([b for _, b in calls])
    d = L.host_arrays(name)[1]
    hold(name, L.evaluate(name, (p.cpu().numpy(), u.cpu().numpy()), d))


def test_box_muller(device):
    """rng_fill('normal'): DKW of Phi(z); per pair exp(-r^2 / 2) and the angle, each uniform, and
    their independence."""
    c = L.CASES['box_muller']
    z = fill('normal', c['n'], c['seed'], c['offset'], device, c['e0']).cpu().numpy()
    hold('box_muller', L.evaluate('box_muller', (z,)))


def test_uniform(device):
    c = L.CASES['uniform']
    args = tuple(fill('uniform', c['n'], c['seed'] + ks, c['offset'] + ko, device, c['e0']).cpu().numpy()
                 for ks, ko in ((0, 0), (0, 1), (1, 0)))
    hold('uniform', L.evaluate('uniform', args))


@pytest.mark.parametrize('name', L.cases_of('gamma'))
def test_gamma(device, name):
    """rng_fill('gamma'): the PIT (computed on the host) against U(0, 1), positivity, independence
    of the elements e / e+1 and of the streams o / o+128 (DeviceRNG.gamma advances by 128); the
    shapes below 1 take the U^(1/shape) boost."""
    c = L.CASES[name]
    g, g_off = (fill('gamma', c['n'], c['seed'], c['offset'] + ko, device, c['e0'], shape=c['shape']).cpu().numpy()
                for ko in (0, 128))
    hold(name, L.evaluate(name, (g, g_off)))


def test_ziggurat_with_the_uniforms_in_one_launch(device):
    """rng_fill_normal_zig_uniform at odd element offsets and odd sizes (8-byte aligned windows:
    the kernel's one-double stores): both outputs against their laws."""
    c = L.CASES['zig_uniform']
    p = torch.empty(c['n'], dtype=torch.float64, device=device)
    u = torch.empty(c['n_u'], dtype=torch.float64, device=device)
    _native.rng_fill_normal_zig_uniform(p, u, c['seed'], c['offset'], c['offset_u'], c['e0'], c['e0_u'])
    d = ds.zig_stream(c['seed'], c['offset'], c['e0'], c['n'])
    hold('zig_uniform', L.evaluate('zig_uniform', (p.cpu().numpy(), u.cpu().numpy()), d))
