"""The cache policy of the WIDE Gaussian HMC kernel's HBM streams (STREAM, hmc_gauss_kernel.hpp):
its record stores and its momentum loads carry the non-temporal hint.  A hint changes no value,
but one read depends on what a hinted store left behind: a rejected chain's old state is read
back from the record that the same lane stored one transition earlier (thin = 1), and the rare
exact decision reads that record by numpy's ownership, i.e. through other lanes of the wave.
Whatever the policy, those reads must see the stored bytes.

Every case holds the launch without energy buffers (the touched kernel where D = 1024, the
step is uniform, the mode is EXACT, every stream is 16-byte aligned and the batch is past the
split kernel's range) to the same launch with them (the untouched kernel that keeps numpy's
sums): `samples`, `state`, `accepted` and `n_accepted` bit for bit.

D = 1024; C = 1 / 5 / 70 and 2051 (a ragged last workgroup, and no multiple of 8); n = 1 / 3 / 9,
thin = 1 / 2, L = 1 / 20, both modes; dt = 0.9 with L = 5, where nearly every transition rejects
and the read-back restore of a hinted store runs in every wave (thin = 1; thin = 2 restores
from the LDS stash); q0, p0, the record and the state each one double off a 16-byte boundary
in turn (the kernel without WIDE); and one record buffer written by two consecutive launches,
so that the second launch's restores read lines that an earlier launch's hinted stores and its
own both touched."""
import numpy as np
import pytest
import torch

from binf_amd import _native

pytestmark = pytest.mark.gpu

D = 1024
CHAINS = [1, 5, 70, 2051]
NMAX = 9
MODES = [_native.MODE_EXACT, _native.MODE_FMA]
_draws = {}


def draws(device, C):
    """(q0 [C, D], p0 [2 NMAX, C, D], u [2 NMAX, C]) on the device, made once per shape and never changed."""
    key = (str(device), C)
    if key not in _draws:
        rs = np.random.RandomState(29 * C + D)
        _draws[key] = tuple(torch.from_numpy(a).to(device) for a in (
            rs.standard_normal((C, D)), rs.standard_normal((2 * NMAX, C, D)), rs.uniform(size=(2 * NMAX, C))))
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


def run(q0, p0, u, n, thin, L, energies, mode, dt=0.3, off=(), samples=None):
    """One launch of n transitions from q0 with the draws p0[:n], u[:n].  `off`: the streams
    ('q0', 'p0', 'samples', 'state') placed one double past a 16-byte boundary.  `samples`: a
    record buffer to write into (one of an earlier launch) instead of a fresh one."""
    C = q0.shape[0]
    dev = q0.device
    nrec = n // thin
    o = lambda name: 1 if name in off else 0
    qin = buffer((C, D), dev, o('q0'))
    qin.copy_(q0)
    pin = buffer((n, C, D), dev, o('p0'))
    pin.copy_(p0[:n])
    if samples is None and nrec:
        samples = buffer((nrec, C, D), dev, o('samples'), -7.0)
    res = {'state': buffer((C, D), dev, o('state'), -3.0),
           'accepted': torch.full((n, C), 9, dtype=torch.uint8, device=dev),
           'n_accepted': torch.zeros(C, dtype=torch.int64, device=dev)}
    if nrec:
        assert samples.shape == (nrec, C, D)
        res['samples'] = samples
    eb = torch.empty((n, C), dtype=torch.float64, device=dev) if energies else None
    ea = torch.empty((n, C), dtype=torch.float64, device=dev) if energies else None
    _native.hmc_sample_n_gauss(qin, pin, u[:n].contiguous(), res['state'], samples if nrec else None,
                               res['accepted'], res['n_accepted'], eb, ea, dt, None, L, n, thin, 1.0, 0.0,
                               0, 1.05, 0.95, mode)
    torch.cuda.synchronize()
    return res


def assert_same_bits(hinted, exact, what):
    assert sorted(hinted) == sorted(exact)
    for name in hinted:
        assert torch.equal(bits(hinted[name]), bits(exact[name])), (name, what)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('C', CHAINS)
def test_hinted_streams_equal_exact_path(device, C, mode):
    q0, p0, u = draws(device, C)
    for L in (1, 20):
        for thin in (1, 2):
            for n in (1, 3, 9):
                hinted = run(q0, p0, u, n, thin, L, False, mode)
                exact = run(q0, p0, u, n, thin, L, True, mode)
                assert_same_bits(hinted, exact, (L, thin, n))
            rate = exact['accepted'].double().mean().item()
            print('C=%d L=%d thin=%d: acceptance %.3f over n = 9' % (C, L, thin, rate))
    assert (exact['state'] != q0).any()                        # L = 20, n = 9: the chains moved


@pytest.mark.parametrize('thin', [1, 2])
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('C', CHAINS)
def test_rejections_read_back_hinted_stores(device, C, mode, thin):
    """dt = 0.9, L = 5: dH = (dt^2 / 8) (sum q'^2 - sum q^2) is tens of units at D = 1024, so
    acceptance is below 1e-3 and the restore runs in every wave on nearly every transition:
    from q0 (the first transition, and n = 1), then from the record that this launch's hinted
    stores wrote (thin = 1) or from the LDS stash (thin = 2)."""
    q0, p0, u = draws(device, C)
    accepted = total = 0
    for n in (1, 3, 9):
        hinted = run(q0, p0, u, n, thin, 5, False, mode, dt=0.9)
        exact = run(q0, p0, u, n, thin, 5, True, mode, dt=0.9)
        assert_same_bits(hinted, exact, n)
        accepted += int(exact['accepted'].sum().item())
        total += n * C
        kept = ~exact['accepted'].bool().any(dim=0)            # chains that never moved keep q0
        assert kept.any() and torch.equal(bits(hinted['state'][kept]), bits(q0[kept]))
        if 'samples' in hinted:                                # ... in every record as well
            assert torch.equal(bits(hinted['samples'][:, kept]),
                               bits(q0[kept].expand(n // thin, -1, -1)))
    print('C=%d thin=%d: %d of %d transitions accepted' % (C, thin, accepted, total))
    assert accepted < 1e-3 * total


@pytest.mark.parametrize('off', ['q0', 'p0', 'samples', 'state'])
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('C', CHAINS)
def test_misaligned_streams_take_the_kernel_without_hints(device, C, mode, off):
    """One stream at a time starts 8 bytes past a 16-byte boundary: the launch takes the kernel
    that moves 8 bytes per lane, and gives the same bits."""
    q0, p0, u = draws(device, C)
    for thin in (1, 2):
        for n, L, dt in ((1, 20, 0.3), (3, 1, 0.3), (9, 20, 0.3), (9, 5, 0.9)):
            if off == 'samples' and n // thin == 0:
                continue
            moved = run(q0, p0, u, n, thin, L, False, mode, dt=dt, off=(off,))
            exact = run(q0, p0, u, n, thin, L, True, mode, dt=dt)
            assert_same_bits(moved, exact, (thin, n, L, dt))


@pytest.mark.parametrize('dt,L', [(0.3, 20), (0.9, 5)])
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('C', CHAINS)
def test_record_buffer_reused_by_the_next_launch(device, C, mode, dt, L):
    """Two consecutive launches write the same record buffer, the second starting from the first's
    state with fresh draws: its restores read records whose lines the first launch stored too."""
    q0, p0, u = draws(device, C)
    n = NMAX
    out = {}
    for energies in (False, True):
        first = run(q0, p0, u, n, 1, L, energies, mode, dt=dt)
        kept = {k: v.clone() for k, v in first.items()}
        second = run(first['state'], p0[n:], u[n:], n, 1, L, energies, mode, dt=dt, samples=first['samples'])
        assert second['samples'].data_ptr() == first['samples'].data_ptr()
        out[energies] = (kept, second)
    assert_same_bits(out[False][0], out[True][0], 'first launch')
    assert_same_bits(out[False][1], out[True][1], 'second launch')
    if dt == 0.9:
        assert not out[True][1]['accepted'].bool().all()       # the second launch restored
    else:
        assert (bits(out[True][1]['samples']) != bits(out[True][0]['samples'])).any()
