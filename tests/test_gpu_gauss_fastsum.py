"""The Gaussian HMC kernel that decides its accepts from fused energy sums (FASTSUM,
hmc_gauss_kernel.hpp): launched when no energy is recorded, it must return the bits of
the kernel that keeps numpy's sums, which is the one launched when energies are recorded.

  * path equality on ordinary draws: records, final state, accept flags, counts and adapted
    step sizes of `binf_hmc_sample_n_gauss_f64` without energy buffers against the same
    call with them -- thin = 1 (a rejection reads the record back) and thin = 2 (it reads
    the LDS stash), both arithmetic modes, with and without per-chain step adaption, a
    non-unit Gaussian;
  * the forced fallback: u of every chain and transition is put on exp(-dE) of the exact
    path to within an ulp, where accept_decide cannot decide (test_gpu_accept_decide.py), so
    every transition of every chain is decided again from numpy's sums; with one chain
    whose start state holds an inf and one that holds a NaN (rejected, state kept).

D = 768 and 1024 are the shapes of the one-chain-per-wave kernel (HC = 3), which serves them
from 2049 chains up: C = 2049 and 2051 end in a workgroup of one and of three waves.  The
fused sums are built for D = 1024 and for the non-unit Gaussian at D = 768; the unit one at
D = 768 and fewer chains (the split kernel) keep numpy's sums on both paths and must agree
all the same."""
from decimal import Decimal, getcontext

import numpy as np
import pytest
import torch

from binf_amd import _native

pytestmark = pytest.mark.gpu

CHAINS = [1, 3, 130, 2049, 2051]
N, L = 4, 3
_draws = {}


def draws(device, C, D):
    """(q0, p0 [N, C, D], u [N, C]) on the device, made once per shape."""
    key = (str(device), C, D)
    if key not in _draws:
        rs = np.random.RandomState(7 * C + D)
        _draws[key] = tuple(torch.from_numpy(a).to(device) for a in (
            rs.standard_normal((C, D)), rs.standard_normal((N, C, D)), rs.uniform(size=(N, C))))
    return _draws[key]


def bits(t):
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


def run(q0, p0, u, n, thin, energies, mode=_native.MODE_EXACT, k=1.0, x0=0.0, dt=0.3, n_adapt=0):
    C, D = q0.shape
    dev = q0.device
    res = {'state': torch.empty_like(q0),
           'samples': torch.full((n // thin, C, D), -7.0, dtype=torch.float64, device=dev),
           'accepted': torch.full((n, C), 9, dtype=torch.uint8, device=dev),
           'n_accepted': torch.zeros(C, dtype=torch.int64, device=dev)}
    eb = torch.empty((n, C), dtype=torch.float64, device=dev) if energies else None
    ea = torch.empty((n, C), dtype=torch.float64, device=dev) if energies else None
    dtc = None
    if n_adapt:
        dtc = dt * (1.0 + 0.01 * torch.arange(C, dtype=torch.float64, device=dev) / C)
        res['dt_chain'] = dtc
    _native.hmc_sample_n_gauss(q0, p0[:n].contiguous(), u[:n].contiguous(), res['state'], res['samples'],
                               res['accepted'], res['n_accepted'], eb, ea, dt, dtc, L, n, thin, k, x0,
                               n_adapt, 1.05, 0.95, mode)
    torch.cuda.synchronize()
    return res, eb, ea


def assert_same_bits(fast, exact):
    assert sorted(fast) == sorted(exact)
    for name in fast:
        assert torch.equal(bits(fast[name]), bits(exact[name])), name


@pytest.mark.parametrize('mode,k,x0,n_adapt', [
    (_native.MODE_EXACT, 1.0, 0.0, 0), (_native.MODE_EXACT, 1.0, 0.0, 3),
    (_native.MODE_FMA, 1.0, 0.0, 0), (_native.MODE_FMA, 1.0, 0.0, 3),
    (_native.MODE_EXACT, 2.5, 0.3, 0), (_native.MODE_FMA, 2.5, 0.3, 3)])
@pytest.mark.parametrize('thin', [1, 2])
@pytest.mark.parametrize('C', CHAINS)
@pytest.mark.parametrize('D', [768, 1024])
def test_fast_path_equals_exact_path(device, D, C, thin, mode, k, x0, n_adapt):
    assert _native.gauss_waves_per_chain(C, D) == (1 if C > 2048 else 4)
    q0, p0, u = draws(device, C, D)
    if k != 1.0:
        q0 = x0 + q0 / np.sqrt(k)
    kw = dict(mode=mode, k=k, x0=x0, n_adapt=n_adapt)
    fast, _, _ = run(q0, p0, u, N, thin, False, **kw)
    exact, eb, ea = run(q0, p0, u, N, thin, True, **kw)
    assert_same_bits(fast, exact)
    rate = exact['accepted'].double().mean().item()
    print('D=%d C=%d: acceptance %.3f' % (D, C, rate))
    if C > 2048:
        assert 0.05 < rate < 0.95                              # both branches of the tail ran
        assert torch.isfinite(eb).all() and torch.isfinite(ea).all()


def nearest_exp(x):
    """The double nearest e^x."""
    return float(Decimal(float(x)).exp())


@pytest.mark.parametrize('k,x0', [(1.0, 0.0), (2.5, 0.3)])
@pytest.mark.parametrize('mode', [_native.MODE_EXACT, _native.MODE_FMA])
@pytest.mark.parametrize('thin', [1, 2])
@pytest.mark.parametrize('C', CHAINS)
@pytest.mark.parametrize('D', [768, 1024])
def test_forced_fallback_returns_the_exact_bits(device, D, C, thin, mode, k, x0):
    getcontext().prec = 40
    n = 3
    q0, p0, u = draws(device, C, D)
    q0, u = x0 + q0 / np.sqrt(k), u[:n].clone()
    special = C >= 3
    if special:
        q0[0, 5] = float('inf')
        q0[1, D - 1] = float('nan')
    for i in range(n):
        # the exact path up to and including transition i, its draws up to i - 1 already placed
        _, eb, ea = run(q0, p0, u, i + 1, 1, True, mode=mode, k=k, x0=x0)
        x = (-(ea[i] - eb[i])).cpu().numpy()
        ui = u[i].cpu().numpy()
        for c in range(C):
            if np.isfinite(x[c]) and x[c] < 700.0:
                ui[c] = np.nextafter(nearest_exp(x[c]), [0.0, 0.0, 2.0][c % 3]) if c % 3 else nearest_exp(x[c])
        u[i] = torch.from_numpy(ui).to(device)
    fast, _, _ = run(q0, p0, u, n, thin, False, mode=mode, k=k, x0=x0)
    exact, eb, ea = run(q0, p0, u, n, thin, True, mode=mode, k=k, x0=x0)
    assert_same_bits(fast, exact)
    acc = exact['accepted'].cpu().numpy()
    if special:
        assert not acc[:, :2].any()
        assert torch.equal(bits(fast['state'][:2]), bits(q0[:2]))
    if C > 2048:
        # u one ulp either side of the threshold: both outcomes occur
        placed = acc[:, 2:]
        assert 0.1 < placed.mean() < 0.9
