"""The persistent Gaussian HMC kernel where the three energy sums of a transition go
up ONE shared tree (one chain per wave: D = 768 and 1024 past 2048 chains) and where
the accept test decides by bounds on the exponential: every recorded state, the
accept flags, both energies, the final state and the counters, bit for bit against
the C oracle run one transition at a time.  D = 8, 64, 256 run beside them so that
every compiled tree height sees the same cases.  Three step sizes per shape: one at
which the bounds decide every move, a mixed one, and one at which most moves are
rejected and the state comes back from the record."""
import functools

import numpy as np
import pytest
import torch

from binf_amd import _native
from oracle import c_oracle

pytestmark = pytest.mark.gpu

N, L = 6, 3
SHAPES = [1024, 768, 8, 64, 256]


def dev_t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def chains_for(D):
    # the smallest batch at which D = 768 / 1024 run one wave per chain
    return 2049 if D in (768, 1024) else 67


@functools.lru_cache(maxsize=None)
def draws(D):
    C = chains_for(D)
    rs = np.random.RandomState(7000 + D)
    return (rs.standard_normal((C, D)), rs.standard_normal((N, C, D)), rs.uniform(size=(N, C)),
            1.0 + 0.01 * rs.uniform(size=C))


def same_energy(got, want):
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan], want[~nan])


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def check(device, D, dt, fma, n=N, thins=(1, 2), k=1.0, x0=0.0, per_chain_dt=False, q0=None):
    """The oracle's n transitions once; the kernel once per thinning against them."""
    C = chains_for(D)
    assert _native.gauss_waves_per_chain(C, D) == 1
    q_start, p0, u, jitter = draws(D)
    q_start = q_start if q0 is None else q0
    p0, u = p0[:n], u[:n]
    dts = dt * jitter if per_chain_dt else None
    states, flags, ebs, eas = [], [], [], []
    q = q_start
    for i in range(n):
        w = c_oracle.hmc_sample_gauss(q, p0[i], u[i], dts if per_chain_dt else dt, L,
                                      k=k, x0=x0, nthreads=8, fma=fma)
        q = w['q_out']
        states.append(q)
        flags.append(w['accepted'])
        ebs.append(w['e_before'])
        eas.append(w['e_after'])

    tp, tu = dev_t(p0, device), dev_t(u, device)
    for thin in thins:
        tq = dev_t(q_start, device)
        out = torch.empty_like(tq)
        rec = torch.empty((n // thin, C, D), dtype=torch.float64, device=device)
        acc = torch.empty((n, C), dtype=torch.uint8, device=device)
        nacc = torch.zeros(C, dtype=torch.int64, device=device)
        eb = torch.empty((n, C), dtype=torch.float64, device=device)
        ea = torch.empty((n, C), dtype=torch.float64, device=device)
        tdt = dev_t(dts, device) if per_chain_dt else None
        _native.hmc_sample_n_gauss(tq, tp, tu, out, rec, acc, nacc, eb, ea, dt, tdt,
                                   L, n, thin, k, x0, 0, 1.05, 0.95,
                                   mode=_native.MODE_FMA if fma else _native.MODE_EXACT)
        torch.cuda.synchronize()
        acc_h, eb_h, ea_h, rec_h = (acc.cpu().numpy(), eb.cpu().numpy(), ea.cpu().numpy(),
                                    rec.cpu().numpy())
        for i in range(n):
            assert np.array_equal(acc_h[i], flags[i]), (thin, i)
            assert same_energy(eb_h[i], ebs[i]), (thin, i)
            assert same_energy(ea_h[i], eas[i]), (thin, i)
            if (i + 1) % thin == 0:
                assert np.array_equal(bits(rec_h[(i + 1) // thin - 1]), bits(states[i])), (thin, i)
        assert np.array_equal(bits(out.cpu().numpy()), bits(states[-1])), thin
        assert np.array_equal(nacc.cpu().numpy(), np.sum(flags, axis=0)), thin
    return np.array(flags)


@pytest.mark.parametrize('fma', [False, True], ids=['exact', 'fma'])
@pytest.mark.parametrize('dt', [0.05, 0.3, 1.7])
@pytest.mark.parametrize('D', SHAPES)
def test_records_flags_energies_bitwise(device, D, dt, fma):
    flags = check(device, D, dt, fma)
    if dt == 0.05:
        assert flags.mean() > 0.9
    if dt == 1.7 and D >= 256:
        assert flags.mean() < 0.5          # the restore path is the common one


@pytest.mark.parametrize('fma', [False, True], ids=['exact', 'fma'])
@pytest.mark.parametrize('dt', [0.05, 0.3, 1.7])
@pytest.mark.parametrize('D', SHAPES)
def test_per_chain_step(device, D, dt, fma):
    check(device, D, dt, fma, per_chain_dt=True)


@pytest.mark.parametrize('fma', [False, True], ids=['exact', 'fma'])
@pytest.mark.parametrize('dt', [0.05, 0.3, 1.7])
def test_non_unit_gaussian(device, dt, fma):
    check(device, 1024, dt, fma, k=2.5, x0=0.3)


@pytest.mark.parametrize('fma', [False, True], ids=['exact', 'fma'])
@pytest.mark.parametrize('dt', [0.3, 1.7])
@pytest.mark.parametrize('D', SHAPES)
def test_single_transition_launches(device, D, dt, fma):
    check(device, D, dt, fma, n=1, thins=(1,))


@pytest.mark.parametrize('D', [1024, 768])
def test_non_finite_state_is_rejected_and_kept(device, D):
    q0 = draws(D)[0].copy()
    q0[3, 5] = np.inf
    q0[1000, D - 1] = np.nan
    q0[2048, 0] = np.nan
    q0[2048, 700] = np.inf
    flags = check(device, D, 0.3, False, q0=q0)
    assert not flags[:, [3, 1000, 2048]].any()
    assert flags.any()
