"""The persistent Gaussian HMC kernel's leapfrog step loop, unrolled by U steps per
back-edge with the remaining steps after it (hmc_gauss_kernel.hpp: GAUSS_STEP_UNROLL):
every trip count class -- no full step at all, remainder only, the unrolled body
alone, both -- against the C oracle run one transition at a time, bit for bit:
every recorded state, the accept flags, both energies, the final state and the
counters.  Shapes: one chain per wave with two element groups (D = 1024) and with
three groups of four (D = 768), several chains per wave (D = 64, 8); the per-lane
step size with adaption; the draws generated in the kernel."""
import functools

import numpy as np
import pytest
import torch

from binf_amd import _native
from oracle import c_oracle

pytestmark = pytest.mark.gpu

# GAUSS_STEP_UNROLL of hmc_gauss_kernel.hpp, restated: the trip counts below sit on the
# boundaries of the main loop and the remainder only while the two agree, so a change of
# the constant there is a change here.  Not every shape takes the unrolled loop:
# gauss_step_unroll() returns 1 for D = 768 in EXACT mode (TMAX 12), whose cases run the
# bare loop; D = 768 in FMA mode and D = 1024, 64, 8 in both modes run the unrolled one.
U = 4
N = 3
NSTEPS = [1, 2, 3, U, U + 1, U + 2, 2 * U + 1, 20, 21]
SHAPES = [1024, 768, 64, 8]


def dev_t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def chains_for(D):
    # the smallest batch at which D = 768 / 1024 run one wave per chain
    return 2049 if D in (768, 1024) else 67


@functools.lru_cache(maxsize=None)
def draws(D):
    C = chains_for(D)
    rs = np.random.RandomState(9100 + D)
    return (rs.standard_normal((C, D)), rs.standard_normal((N, C, D)), rs.uniform(size=(N, C)),
            1.0 + 0.01 * rs.uniform(size=C))


def step_size(D):
    # the energy error of a trajectory scales with dt^4 D: acceptance inside (0, 1), so
    # both the accepted path and the restore of a rejected chain run
    return 1.3 / D ** 0.25


def same_energy(got, want):
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan], want[~nan])


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def check(device, D, L, fma, adapt=False):
    C = chains_for(D)
    assert _native.gauss_waves_per_chain(C, D) == 1
    q, p0, u, jitter = draws(D)
    dt = step_size(D)
    dts = dt * jitter if adapt else None
    tq, tp, tu = dev_t(q, device), dev_t(p0, device), dev_t(u, device)
    out = torch.empty_like(tq)
    rec = torch.empty((N, C, D), dtype=torch.float64, device=device)
    acc = torch.empty((N, C), dtype=torch.uint8, device=device)
    nacc = torch.zeros(C, dtype=torch.int64, device=device)
    eb = torch.empty((N, C), dtype=torch.float64, device=device)
    ea = torch.empty((N, C), dtype=torch.float64, device=device)
    tdt = dev_t(dts, device) if adapt else None
    _native.hmc_sample_n_gauss(tq, tp, tu, out, rec, acc, nacc, eb, ea, dt, tdt, L, N, 1, 1.0, 0.0,
                               N if adapt else 0, 1.05, 0.95,
                               mode=_native.MODE_FMA if fma else _native.MODE_EXACT)
    torch.cuda.synchronize()
    acc_h, eb_h, ea_h, rec_h = acc.cpu().numpy(), eb.cpu().numpy(), ea.cpu().numpy(), rec.cpu().numpy()
    flags = []
    for i in range(N):
        w = c_oracle.hmc_sample_gauss(q, p0[i], u[i], dts if adapt else dt, L, nthreads=8, fma=fma,
                                      adapt=adapt)
        q = w['q_out']
        if adapt:
            dts = w['timestep_out']
        flags.append(w['accepted'])
        assert np.array_equal(acc_h[i], w['accepted']), i
        assert same_energy(eb_h[i], w['e_before']), i
        assert same_energy(ea_h[i], w['e_after']), i
        assert np.array_equal(bits(rec_h[i]), bits(q)), i
    assert np.array_equal(bits(out.cpu().numpy()), bits(q))
    assert np.array_equal(nacc.cpu().numpy(), np.sum(flags, axis=0))
    if adapt:
        assert np.array_equal(bits(tdt.cpu().numpy()), bits(dts))
    return np.array(flags)


@pytest.mark.parametrize('fma', [False, True], ids=['exact', 'fma'])
@pytest.mark.parametrize('L', NSTEPS)
@pytest.mark.parametrize('D', SHAPES)
def test_every_trip_count_bitwise(device, D, L, fma):
    flags = check(device, D, L, fma)
    assert 0 < flags.mean() < 1


@pytest.mark.parametrize('fma', [False, True], ids=['exact', 'fma'])
@pytest.mark.parametrize('L', [U + 1, 20])
def test_per_chain_step_with_adaption(device, L, fma):
    check(device, 1024, L, fma, adapt=True)


@pytest.mark.parametrize('mode', [_native.MODE_EXACT, _native.MODE_FMA], ids=['exact', 'fma'])
def test_draws_generated_in_the_kernel(device, mode):
    """sample_n with the generator in the kernel against the same call fed with the
    dump of its stream."""
    C, D, L, seed, offset = 2049, 1024, U + 1, 31, 4
    dt = step_size(D)
    tq = dev_t(draws(D)[0], device)

    def buffers():
        return (torch.empty_like(tq), torch.empty((N, C, D), dtype=torch.float64, device=device),
                torch.empty((N, C), dtype=torch.uint8, device=device),
                torch.zeros(C, dtype=torch.int64, device=device),
                torch.empty((N, C), dtype=torch.float64, device=device),
                torch.empty((N, C), dtype=torch.float64, device=device))
    a, b = buffers(), buffers()
    _native.hmc_sample_n_gauss_rng(tq, *a, dt, None, L, N, 1, 1.0, 0.0, 0, 1.05, 0.95, mode, seed, offset)
    p0, u = _native.hmc_gauss_rng_draws(N, C, D, seed, offset, device)
    _native.hmc_sample_n_gauss(tq, p0, u, *b, dt, None, L, N, 1, 1.0, 0.0, 0, 1.05, 0.95, mode=mode)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert 0 < float(a[2].double().mean()) < 1
