"""The Gaussian HMC kernel with 16-byte lane ownership (WIDE, hmc_gauss_kernel.hpp): lane l of a
chain's wave owns elements 128 r + 2 l + b and moves them 16 bytes at a time; its fused sums
run in that order, and only the rare exact decision keeps numpy's ownership for its own reads.
It is the kernel launched for the unit Gaussian with one step size for the batch when no
energy is recorded and every stream is 16-byte aligned, and it must return the bits of the
kernel that keeps numpy's sums, which is the one launched when energies are recorded:
`samples`, `state`, `accepted` and `n_accepted` of `binf_hmc_sample_n_gauss_f64` without energy
buffers against the same call with them.

D = 1024 with 2049 and 2051 chains (a last workgroup of one and of three waves; up to 2048
chains run the split kernel).  n = 1 / 2 / 5 / 9, L = 1 / 2 / 5 / 20, both modes, and thin =
1 / 2 / 3: a rejected chain's old state comes back from q0 (the first transition with thin = 1,
and n = 1), from the record (thin = 1) or from the LDS stash (every other launch).  Further: u
within an ulp of exp(-dE) on every chain and transition, so that every decision is the exact
path's, reading each of those three sources by numpy's ownership; a step near the domain's edge
(dt = 0.9, L = 5), where many transitions reject and the 16-byte restore runs; chains that hold
an inf, a NaN and a momentum of 1e160; and q0, p0, the record and the state each one double off
a 16-byte boundary in turn, which take the kernel with numpy's ownership and give the same
bits."""
from decimal import Decimal, getcontext

import numpy as np
import pytest
import torch

from binf_amd import _native

pytestmark = pytest.mark.gpu

D = 1024
CHAINS = [2049, 2051]
NMAX = 9
MODES = [_native.MODE_EXACT, _native.MODE_FMA]
_draws = {}
_placed = {}


def draws(device, C):
    """(q0, p0 [NMAX, C, D], u [NMAX, C]) on the device, made once per shape and never changed."""
    key = (str(device), C)
    if key not in _draws:
        rs = np.random.RandomState(13 * C + D)
        _draws[key] = tuple(torch.from_numpy(a).to(device) for a in (
            rs.standard_normal((C, D)), rs.standard_normal((NMAX, C, D)), rs.uniform(size=(NMAX, C))))
    return _draws[key]


def bits(t):
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


def buffer(shape, device, off, fill=None):
    """A contiguous float64 tensor whose first element lies `off` doubles past a 16-byte boundary."""
    numel = int(np.prod(shape))
    flat = torch.empty(numel + 2, dtype=torch.float64, device=device)
    assert flat.data_ptr() % 16 == 0
    t = flat[off:off + numel].view(shape)
    if fill is not None:
        t.fill_(fill)
    assert t.data_ptr() % 16 == 8 * off and t.is_contiguous()
    return t


def run(q0, p0, u, n, thin, L, energies, mode=_native.MODE_EXACT, dt=0.3, off=()):
    """One launch.  `off`: the streams ('q0', 'p0', 'samples', 'state') to place one double
    past a 16-byte boundary; every other stream starts on one."""
    C = q0.shape[0]
    dev = q0.device
    nrec = n // thin
    o = lambda name: 1 if name in off else 0
    qin = buffer((C, D), dev, o('q0'))
    qin.copy_(q0)
    pin = buffer((n, C, D), dev, o('p0'))
    pin.copy_(p0[:n])
    res = {'state': buffer((C, D), dev, o('state'), -3.0),
           'samples': buffer((nrec, C, D), dev, o('samples'), -7.0) if nrec else None,
           'accepted': torch.full((n, C), 9, dtype=torch.uint8, device=dev),
           'n_accepted': torch.zeros(C, dtype=torch.int64, device=dev)}
    eb = torch.empty((n, C), dtype=torch.float64, device=dev) if energies else None
    ea = torch.empty((n, C), dtype=torch.float64, device=dev) if energies else None
    _native.hmc_sample_n_gauss(qin, pin, u[:n].contiguous(), res['state'], res['samples'],
                               res['accepted'], res['n_accepted'], eb, ea, dt, None, L, n, thin, 1.0, 0.0,
                               0, 1.05, 0.95, mode)
    torch.cuda.synchronize()
    if res['samples'] is None:
        del res['samples']
    return res, eb, ea


def assert_same_bits(wide, exact):
    assert sorted(wide) == sorted(exact)
    for name in wide:
        assert torch.equal(bits(wide[name]), bits(exact[name])), name


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('L', [1, 2, 5, 20])
@pytest.mark.parametrize('thin', [1, 2, 3])
@pytest.mark.parametrize('C', CHAINS)
def test_wide_ownership_equals_exact_path(device, C, thin, L, mode):
    assert _native.gauss_waves_per_chain(C, D) == 1
    q0, p0, u = draws(device, C)
    rates = []
    for n in (1, 2, 5, 9):
        wide, _, _ = run(q0, p0, u, n, thin, L, False, mode=mode)
        exact, eb, ea = run(q0, p0, u, n, thin, L, True, mode=mode)
        assert_same_bits(wide, exact)
        assert torch.isfinite(eb).all() and torch.isfinite(ea).all()
        rates.append(exact['accepted'].double().mean().item())
    print('C=%d thin=%d L=%d: acceptance %s' % (C, thin, L, ' '.join('%.3f' % r for r in rates)))
    assert 0.05 < rates[-1] < 0.999                           # both branches of the tail ran


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('thin', [1, 2, 3])
@pytest.mark.parametrize('C', CHAINS)
def test_many_rejections_restore_16_bytes_at_a_time(device, C, thin, mode):
    """dt = 0.9 with L = 5, close to the edge k dt^2 <= 1 of the kernel's domain: dH = (dt^2 / 8)
    (sum q'^2 - sum q^2) is tens of units at D = 1024 (numpy on the host: acceptance below one
    in a thousand), so nearly every transition rejects and the restore runs in every wave, from
    each of its three sources."""
    q0, p0, u = draws(device, C)
    for n in (1, 2, 5, 9):
        wide, _, _ = run(q0, p0, u, n, thin, 5, False, mode=mode, dt=0.9)
        exact, _, _ = run(q0, p0, u, n, thin, 5, True, mode=mode, dt=0.9)
        assert_same_bits(wide, exact)
        rate = exact['accepted'].double().mean().item()
        print('C=%d thin=%d n=%d: acceptance %.4f' % (C, thin, n, rate))
        assert rate < 0.5                                      # many rejections
        kept = ~exact['accepted'].bool().any(dim=0)            # chains that never moved keep q0
        assert kept.any() and torch.equal(bits(wide['state'][kept]), bits(q0[kept]))


def special_start(q0, p0):
    """Chains 0 / 1 / 2: an inf, a NaN in the state, a momentum whose square overflows."""
    q0, p0 = q0.clone(), p0.clone()
    q0[0, 5] = float('inf')
    q0[1, D - 1] = float('nan')
    p0[:, 2, 77] = 1e160
    return q0, p0


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('L', [1, 5, 20])
@pytest.mark.parametrize('thin', [1, 2, 3])
@pytest.mark.parametrize('C', CHAINS)
def test_inf_nan_and_overflowing_momentum(device, C, thin, L, mode):
    q0, p0, u = draws(device, C)
    q0, p0 = special_start(q0, p0)
    n = 5
    wide, _, _ = run(q0, p0, u, n, thin, L, False, mode=mode)
    exact, eb, ea = run(q0, p0, u, n, thin, L, True, mode=mode)
    assert_same_bits(wide, exact)
    assert not exact['accepted'][:, :3].any()                 # rejected, state kept
    assert torch.equal(bits(wide['state'][:3]), bits(q0[:3]))
    assert torch.isinf(eb[:, 2]).all()


def nearest_exp(x):
    """The double nearest e^x."""
    return float(Decimal(float(x)).exp())


def placed_draws(device, C, L, mode, n):
    """u [n, C] within an ulp of exp(-dE) of the exact path on every chain and transition (chain
    c: on the threshold, one ulp below, one ulp above, by c % 3).  It depends on the trajectory
    alone, not on thin: made once per (C, L, mode)."""
    key = (str(device), C, L, mode, n)
    if key not in _placed:
        getcontext().prec = 40
        q0, p0, u = draws(device, C)
        q0, p0 = special_start(q0, p0)
        u = u[:n].clone()
        for i in range(n):
            # the exact path up to and including transition i, its draws up to i - 1 already placed
            _, eb, ea = run(q0, p0, u, i + 1, 1, L, True, mode=mode)
            x = (-(ea[i] - eb[i])).cpu().numpy()
            ui = u[i].cpu().numpy()
            for c in range(C):
                if np.isfinite(x[c]) and x[c] < 700.0:
                    ui[c] = np.nextafter(nearest_exp(x[c]), [0.0, 0.0, 2.0][c % 3]) if c % 3 else nearest_exp(x[c])
            u[i] = torch.from_numpy(ui).to(device)
        _placed[key] = (q0, p0, u)
    return _placed[key]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('L', [1, 20])
@pytest.mark.parametrize('thin', [1, 2, 3])
@pytest.mark.parametrize('C', CHAINS)
def test_forced_fallback_reads_by_numpy_ownership(device, C, thin, L, mode):
    """Every transition of every chain is decided by gauss_exact_accept: from q0 and from the
    record (thin = 1), from q0 alone (n = 1) and from the LDS stash (thin = 2, 3)."""
    nmax = 3
    q0, p0, u = placed_draws(device, C, L, mode, nmax)
    for n in (1, nmax):
        wide, _, _ = run(q0, p0, u, n, thin, L, False, mode=mode)
        exact, eb, ea = run(q0, p0, u, n, thin, L, True, mode=mode)
        assert_same_bits(wide, exact)
    acc = exact['accepted'].cpu().numpy()
    assert not acc[:, :3].any()
    assert torch.equal(bits(wide['state'][:3]), bits(q0[:3]))
    placed = acc[:, 3:]                                       # u one ulp either side of the threshold
    assert 0.1 < placed.mean() < 0.9


@pytest.mark.parametrize('off', ['q0', 'p0', 'samples', 'state'])
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('thin', [1, 2])
@pytest.mark.parametrize('C', CHAINS)
def test_misaligned_streams_take_the_fallback(device, C, thin, mode, off):
    """One stream at a time starts 8 bytes past a 16-byte boundary: the launch must not move
    16 bytes per lane (an unaligned dwordx4 access), and gives the same bits."""
    q0, p0, u = draws(device, C)
    for n, L in ((1, 5), (5, 5), (9, 20)):
        if off == 'samples' and n // thin == 0:
            continue
        moved, _, _ = run(q0, p0, u, n, thin, L, False, mode=mode, off=(off,))
        exact, _, _ = run(q0, p0, u, n, thin, L, True, mode=mode)
        assert_same_bits(moved, exact)
