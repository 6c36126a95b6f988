"""The persistent Gaussian HMC kernel sets its wave priority from the transitions it has
left (hmc_gauss_kernel.hpp: GAUSS_PRIO_WINDOW).  Priority cannot change a value, so this
file guards the code around it: sample_n(n) against the C oracle run one transition at a
time and against n calls of sample(), bit for bit -- every recorded state, the final
state, the accept flags and the counters -- at transition counts with no priority change
in the launch, inside one window, exactly one window and past the last threshold, with
every state recorded and every second one, in both arithmetic modes.  Shapes: several
chains per wave (D = 8, 64), one chain per wave or a chain over several waves (D = 768,
1024, by the batch size), a ragged tree (D = 1032); batches that end inside a wave; one
batch with more waves than the chip holds at once, so that a wave buffer slot is reused."""
import functools

import numpy as np
import pytest
import torch

from binf_amd import _native
from binf_amd.pdf import IsotropicGaussian
from binf_amd.samplers.hmc import HMCSampler
from oracle import c_oracle

pytestmark = pytest.mark.gpu

L = 5
NMAX = 9
DIMS = [8, 64, 768, 1024, 1032]
CHAINS = [1, 5, 70]
COUNTS = [1, 3, 4, 9]
MODES = [False, True]


def dev_t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device)


def step_size(D):
    # the energy error of a trajectory scales with dt^4 D: acceptance inside (0, 1), so
    # both the accepted path and the restore of a rejected chain run
    return 1.3 / D ** 0.25


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@functools.lru_cache(maxsize=None)
def draws(D, C, n):
    rs = np.random.RandomState(7300 + 13 * D + C)
    return rs.standard_normal((C, D)), rs.standard_normal((n, C, D)), rs.uniform(size=(n, C))


@functools.lru_cache(maxsize=None)
def reference(D, C, n, fma):
    """The oracle's chain, one transition at a time: states [n, C, D] and flags [n, C].
    Shared by every test of the shape and never written to."""
    q, p0, u = draws(D, C, n)
    states, flags = [], []
    for i in range(n):
        w = c_oracle.hmc_sample_gauss(q, p0[i], u[i], step_size(D), L, nthreads=8, fma=fma)
        q = w['q_out']
        states.append(q)
        flags.append(w['accepted'].astype(bool))
    states, flags = np.array(states), np.array(flags)
    states.setflags(write=False)
    flags.setflags(write=False)
    return states, flags


def sampler(device, D, C, fma):
    q0 = draws(D, C, NMAX)[0]
    return HMCSampler(IsotropicGaussian(), dev_t(q0, device), step_size(D), L, variable_name='x',
                      mode='fma' if fma else 'exact')


def check_sample_n(device, D, C, n, thin, fma, nmax=NMAX):
    _, p0, u = draws(D, C, nmax)
    states, flags = reference(D, C, nmax, fma)
    s = sampler(device, D, C, fma) if nmax == NMAX else \
        HMCSampler(IsotropicGaussian(), dev_t(draws(D, C, nmax)[0], device), step_size(D), L,
                   variable_name='x', mode='fma' if fma else 'exact')
    rec = s.sample_n(n, thin=thin, p0=dev_t(p0[:n], device), u=dev_t(u[:n], device))
    torch.cuda.synchronize()
    kept = [i for i in range(n) if (i + 1) % thin == 0]
    assert rec.shape == (len(kept), C, D)
    if kept:
        assert np.array_equal(bits(rec.cpu().numpy()), bits(states[kept]))
    assert np.array_equal(bits(s.state.cpu().numpy()), bits(states[n - 1]))
    assert np.array_equal(s.accepted_history.cpu().numpy(), flags[:n])
    assert np.array_equal(s.last_move_accepted.cpu().numpy(), flags[n - 1])
    assert np.array_equal(s.n_accepted.cpu().numpy(), flags[:n].sum(axis=0))
    return s


@pytest.mark.parametrize('fma', MODES, ids=['exact', 'fma'])
@pytest.mark.parametrize('thin', [1, 2])
@pytest.mark.parametrize('n', COUNTS)
@pytest.mark.parametrize('C', CHAINS)
@pytest.mark.parametrize('D', DIMS)
def test_sample_n_against_the_oracle_bitwise(device, D, C, n, thin, fma):
    check_sample_n(device, D, C, n, thin, fma)


@pytest.mark.parametrize('fma', MODES, ids=['exact', 'fma'])
@pytest.mark.parametrize('n', COUNTS)
@pytest.mark.parametrize('C', CHAINS)
@pytest.mark.parametrize('D', DIMS)
def test_sample_n_equals_n_calls_of_sample(device, D, C, n, fma):
    _, p0, u = draws(D, C, NMAX)
    a = check_sample_n(device, D, C, n, 1, fma)
    b = sampler(device, D, C, fma)
    flags = []
    for i in range(n):
        out = b.sample(p0=dev_t(p0[i], device), u=dev_t(u[i], device))
        flags.append(b.last_move_accepted.cpu().numpy())
    torch.cuda.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(a.state.cpu().numpy()))
    assert np.array_equal(np.array(flags), a.accepted_history.cpu().numpy())
    assert np.array_equal(b.n_accepted.cpu().numpy(), a.n_accepted.cpu().numpy())


def test_some_chains_reject():
    """The step size puts the acceptance inside (0, 1) at every dimension, so the restore of
    a rejected chain runs in the cases above (host reference alone, no device work)."""
    for D in DIMS:
        flags = reference(D, 70, NMAX, False)[1]
        assert 0 < flags.mean() < 1, D


@pytest.mark.parametrize('fma', MODES, ids=['exact', 'fma'])
@pytest.mark.parametrize('n', COUNTS)
@pytest.mark.parametrize('D', [768, 1024])
def test_one_wave_per_chain(device, D, n, fma):
    """The smallest batch at which D = 768 / 1024 run one wave per chain: the
    instantiations that change their priority.  The last wave's workgroup is not full."""
    C = 2049
    assert _native.gauss_waves_per_chain(C, D) == 1
    check_sample_n(device, D, C, n, 1, fma)


@pytest.mark.parametrize('fma', MODES, ids=['exact', 'fma'])
def test_more_waves_than_the_chip_holds(device, fma):
    """4100 one-wave chains of 112 VGPRs: 4096 are resident at once, so the last workgroup
    starts in a slot that another has left."""
    D, C, n = 1024, 4100, 2
    assert _native.gauss_waves_per_chain(C, D) == 1
    check_sample_n(device, D, C, n, 1, fma, nmax=n)
