"""Every device draw stream against its host restatement (tests/draw_streams.py),
element by element: in bits wherever no device log / sincospi / pow enters the value,
within the bound derived there where one does.  A decision that differs from the
restatement on a non-marginal element shows as a mismatch and fails the test.

Each test states how many elements of each path it must have compared, so that none
can pass by comparing nothing; the minimum counts follow from the path probabilities
(slow path 0.43 %, of which wedge-accepted about half; tail 5.1e-5) at half their
expectation.  Marginal elements: at most 1 per 10^6 compared (the chosen seeds meet
none, tests/test_draw_streams.py).

The accuracy hypothesis behind the bounds (1 ulp log / exp, 2 ulp sincospi, 2 ulp pow)
is stated in tests/draw_streams.py; the largest errors observed on an MI355X are in the
docstring of each test (ulp = 2**-52 relative).  They are records, not tolerances.
"""
import numpy as np
import pytest
import torch

import draw_streams as ds
from binf_amd import _native

pytestmark = pytest.mark.gpu


def fill(kind, n, seed, offset, device, elem_offset=0, shifted=False, shape=None):
    """`shifted`: the output is a view one double into its buffer (8-byte aligned)."""
    buf = torch.full((n + 3,), float('nan'), dtype=torch.float64, device=device)
    out = buf[1:n + 1] if shifted else buf[:n]
    assert out.data_ptr() % 16 == (8 if shifted else 0)
    _native.rng_fill(kind, out, seed, offset, shape=shape, elem_offset=elem_offset)
    host = buf.cpu().numpy()
    rest = np.concatenate([host[:1], host[n + 1:]]) if shifted else host[n:]
    assert np.isnan(rest).all(), 'the kernel wrote outside its window'
    return host[1:n + 1] if shifted else host[:n]


def hold(got, d, label, minimum=None, exact=False):
    rep = ds.compare(got, d)
    print('%s: %s' % (label, ds.describe(rep, got, d)))
    assert len(rep['mismatches']) == 0, ds.describe(rep, got, d)
    assert rep['marginal'] * 10 ** 6 <= rep['n'], rep
    if exact:
        assert not d.bound.any()
    for name, least in (minimum or {}).items():
        assert rep['compared'][name] >= least, (label, name, rep['compared'])
    return rep


def slow_minimum(n):
    """Half the expected counts of n ziggurat candidates (none asked for below 10^4)."""
    if n < 10 ** 4:
        return {'fast': min(n, 1)}
    return {'fast': int(0.99 * n), 'wedge': int(0.5 * 0.0021 * n), 'redrawn': int(0.5 * 0.0018 * n),
            'tail': int(0.5 * 5.1e-5 * n)}


@pytest.mark.parametrize('seed,offset,e0,n,shifted', ds.FLAT_CASES)
def test_uniform_stream_in_bits(device, seed, offset, e0, n, shifted):
    d = ds.uniform_stream(seed, offset, e0, n)
    hold(fill('uniform', n, seed, offset, device, e0, shifted), d, 'uniform', {'fast': n}, exact=True)


@pytest.mark.parametrize('seed,offset,e0,n,shifted', ds.FLAT_CASES)
def test_box_muller_stream_within_4_ulp(device, seed, offset, e0, n, shifted):
    """log, sqrt, sincospi and one product.  Observed on an MI355X: largest error 1.98 ulp
    over 2^20 elements (bound 4 + 1/2 for the reference's rounding)."""
    d = ds.box_muller_stream(seed, offset, e0, n)
    hold(fill('normal', n, seed, offset, device, e0, shifted), d, 'box-muller', {'fast': n})


@pytest.mark.parametrize('seed,offset,e0,n,shifted', ds.ZIG_CASES)
def test_ziggurat_stream(device, seed, offset, e0, n, shifted):
    """Fast, wedge-accepted and redrawn elements in bits; tail elements (log, a division,
    a subtraction) within the bound.  Observed: largest tail error 0.95 ulp over 190
    tail elements -- one spacing of a value just above 4."""
    d = ds.zig_stream(seed, offset, e0, n)
    rep = hold(fill('normal_zig', n, seed, offset, device, e0, shifted), d, 'ziggurat', slow_minimum(n))
    assert not d.bound[d.path != ds.TAIL].any()
    if n == 1 << 22:
        c = rep['compared']
        assert c['wedge'] + c['redrawn'] + c['tail'] >= 17000 and c['tail'] >= 180, c


@pytest.mark.parametrize('C,D,coff', [(4099, 64, 0), (7, 33, 11), (1, 1, (1 << 33) + 1)])
def test_ziggurat_with_the_uniform_tail_in_one_launch(device, C, D, coff):
    seed, on, ou = ds.SEED + 9, ds.ZIG_OFF - 9, ds.ZIG_OFF - 8
    p = torch.empty(C * D, dtype=torch.float64, device=device)
    u = torch.empty(C, dtype=torch.float64, device=device)
    _native.rng_fill_normal_zig_uniform(p, u, seed, on, ou, coff * D, coff)
    hold(p.cpu().numpy(), ds.zig_stream(seed, on, coff * D, C * D), 'zig+uniform: normals', slow_minimum(C * D))
    hold(u.cpu().numpy(), ds.uniform_stream(seed, ou, coff, C), 'zig+uniform: uniforms', {'fast': C}, exact=True)


@pytest.mark.parametrize('shape,seed,offset,e0,n', ds.GAMMA_CASES)
def test_gamma_stream(device, shape, seed, offset, e0, n):
    """Every element, retried ones included, within the propagated bound (a few ulp;
    it grows as t = 1 + c x nears 0).  Observed, largest error per shape: 0.5 (with pow)
    23.9 ulp, 1: 86.2, 2.5: 7.5, 11: 3.3, 8193: 3.0, 1e8: 2.7 -- the large figures belong
    to elements with t near 0, whose bound is larger still; no element used more than
    0.86 of its bound."""
    d = ds.gamma_stream(shape, seed, offset, e0, n)
    assert d.info['exhausted'] == 0
    retried = int(np.sum(d.info['attempts'] >= 1))
    # Marsaglia & Tsang's acceptance rate is above 95 % for every alpha >= 1 and tends to 1
    # with alpha: retried elements are certain at 2 10^5 draws only for the small shapes
    assert (shape > 11.0 or retried > 100) and retried < 0.06 * n
    hold(fill('gamma', n, seed, offset, device, e0, shape=shape), d, 'gamma %g' % shape,
         {'fast': int(0.94 * n), 'redrawn': retried})


@pytest.mark.parametrize('n,C,D,seed,offset,coff', ds.FUSED_CASES)
def test_fused_generator_stream(device, n, C, D, seed, offset, coff):
    """hmc_gauss_rng_draws: all paths of every lane stream, the candidates-then-
    rejections order (D >= 64: several elements per lane), ragged trees (D = 33, 200:
    undrawn slots consume nothing, redundant groups share the stream of their leaf),
    chains of several waves (D = 2048), two transitions per launch, a chain offset;
    and the acceptance uniform that follows the last group, in bits.  Observed:
    largest tail error 0.95 ulp (D = 2048), everything else 0."""
    p0, u = _native.hmc_gauss_rng_draws(n, C, D, seed, offset, device, chain_offset=coff)
    dp, du = ds.fused_streams(n, C, D, seed, offset, coff)
    hold(p0.cpu().numpy(), dp, 'fused D=%d: momenta' % D, slow_minimum(n * C * D))
    hold(u.cpu().numpy(), du, 'fused D=%d: uniforms' % D, {'fast': n * C}, exact=True)


@pytest.mark.parametrize('C,D,seed,offset,coff', ds.BIG_CASES)
def test_long_chain_stream(device, C, D, seed, offset, coff):
    """hmc_gauss_big_rng_draws: a full and a ragged chunk; momenta and the chain's
    uniform from BIG_U_STREAM.  Observed: every element in bits (the 21 tail elements
    included)."""
    p0, u = _native.hmc_gauss_big_rng_draws(C, D, seed, offset, device, chain_offset=coff)
    dp, du = ds.big_streams(C, D, seed, offset, coff)
    hold(p0.cpu().numpy(), dp, 'long chains: momenta', slow_minimum(C * D))
    hold(u.cpu().numpy(), du, 'long chains: uniforms', {'fast': C}, exact=True)
