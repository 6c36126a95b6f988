"""The persistent Gaussian HMC kernel on the regular one-wave shapes, whose energy
trees have a compile-time height (one kernel per height, dispatched by the host):
every recorded state, the accept flags and both energies of every transition,
bit for bit against the C oracle run one transition at a time.  Covers every
tree height a one-wave chain has (D = 8 ... 1024, and the 12-element leaves of
D = 96 ... 768), single and many transitions, thinned records, the per-chain
step size variant, a non-unit Gaussian, and batches where most moves are
rejected (the restore path)."""
import numpy as np
import pytest
import torch

from binf_amd import _native
from oracle import c_oracle

pytestmark = pytest.mark.gpu


def dev_t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def chains_for(D):
    # D = 768 / 1024 with few chains go to the split kernel; past 2048 chains one
    # wave runs one chain
    return 2049 if D in (768, 1024) else 67


def run_and_check(device, D, n, thin, dt, L=3, k=1.0, x0=0.0, per_chain_dt=False):
    C = chains_for(D)
    assert _native.gauss_waves_per_chain(C, D) == 1
    rs = np.random.RandomState(1000 * D + 10 * n + thin)
    q0 = rs.standard_normal((C, D))
    p0 = rs.standard_normal((n, C, D))
    u = rs.uniform(size=(n, C))
    dts = dt * (1.0 + 0.01 * rs.uniform(size=C)) if per_chain_dt else None

    tq = dev_t(q0, device)
    out = torch.empty_like(tq)
    rec = torch.empty((n // thin, C, D), dtype=torch.float64, device=device)
    acc = torch.empty((n, C), dtype=torch.uint8, device=device)
    nacc = torch.zeros(C, dtype=torch.int64, device=device)
    eb = torch.empty((n, C), dtype=torch.float64, device=device)
    ea = torch.empty((n, C), dtype=torch.float64, device=device)
    tdt = dev_t(dts, device) if per_chain_dt else None
    _native.hmc_sample_n_gauss(tq, dev_t(p0, device), dev_t(u, device), out,
                               rec if n // thin else None, acc, nacc, eb, ea, dt, tdt,
                               L, n, thin, k, x0, 0, 1.05, 0.95)
    torch.cuda.synchronize()

    q = q0
    want_acc = []
    for i in range(n):
        w = c_oracle.hmc_sample_gauss(q, p0[i], u[i], dts if per_chain_dt else dt, L,
                                      k=k, x0=x0, nthreads=8)
        q = w['q_out']
        assert np.array_equal(acc[i].cpu().numpy(), w['accepted']), i
        assert np.array_equal(eb[i].cpu().numpy(), w['e_before']), i
        assert np.array_equal(ea[i].cpu().numpy(), w['e_after']), i
        if (i + 1) % thin == 0:
            assert np.array_equal(rec[(i + 1) // thin - 1].cpu().numpy(), q), i
        want_acc.append(w['accepted'])
    assert np.array_equal(out.cpu().numpy(), q)
    assert np.array_equal(nacc.cpu().numpy(), np.sum(want_acc, axis=0))
    return np.mean(want_acc)


SHAPES = [8, 16, 32, 64, 128, 256, 512, 1024, 96, 192, 384, 768]


@pytest.mark.parametrize('n,thin', [(1, 1), (64, 1), (64, 4)])
@pytest.mark.parametrize('D', SHAPES)
def test_regular_shapes_bitwise_vs_oracle(device, D, n, thin):
    run_and_check(device, D, n, thin, dt=0.3)


@pytest.mark.parametrize('D', [16, 256, 1024, 768])
def test_regular_shapes_non_unit_and_per_chain_step(device, D):
    run_and_check(device, D, 8, 1, dt=0.25, k=2.5, x0=0.3)
    run_and_check(device, D, 8, 2, dt=0.25, per_chain_dt=True)


@pytest.mark.parametrize('D,thin', [(1024, 1), (1024, 4), (64, 1), (384, 1)])
def test_forced_rejections_restore_the_state(device, D, thin):
    # a step this large makes the trajectory diverge for most chains
    rate = run_and_check(device, D, 16, thin, dt=2.5)
    assert rate < 0.5
