"""The Gaussian HMC kernel that decides its accepts from TWO fused sums (ONESUM,
hmc_gauss_kernel.hpp): for the unit Gaussian with one step size for the batch, launched when
no energy is recorded, the trajectory ends with its last drift and the exponent is
-(k^2 dt^2 / 8) (sum q'^2 - sum q^2).  It must return the bits of the kernel that keeps numpy's
sums, which is the one launched when energies are recorded: `samples`, `state`, `accepted`
and `n_accepted` of `binf_hmc_sample_n_gauss_f64` without energy buffers against the same call
with them.

D = 1024 with 2049 and 2051 chains (a last workgroup of one and of three waves; up to 2048
chains run the split kernel).  L = 1 (no full step) .. 20 covers every remainder of the step
loop's unroll by 4, n = 1 .. 9 every priority window, thin = 1 / 2 both sources of a rejected
chain's old state.  Further: u within an ulp of exp(-dE) on every chain and transition (every
decision falls back to numpy's sums), chains that hold an inf, a NaN and a momentum of 1e160
(p^2 overflows), and launches outside the kernel's domain (dt = 1.5, adaption, a non-unit
Gaussian), which take the three-sum kernels as before."""
from decimal import Decimal, getcontext

import numpy as np
import pytest
import torch

from binf_amd import _native

pytestmark = pytest.mark.gpu

D = 1024
CHAINS = [2049, 2051]
NMAX = 9
_draws = {}


def draws(device, C):
    """(q0, p0 [NMAX, C, D], u [NMAX, C]) on the device, made once per shape and never changed."""
    key = (str(device), C)
    if key not in _draws:
        rs = np.random.RandomState(11 * C + D)
        _draws[key] = tuple(torch.from_numpy(a).to(device) for a in (
            rs.standard_normal((C, D)), rs.standard_normal((NMAX, C, D)), rs.uniform(size=(NMAX, C))))
    return _draws[key]


def bits(t):
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


def run(q0, p0, u, n, thin, L, energies, mode=_native.MODE_EXACT, k=1.0, x0=0.0, dt=0.3, n_adapt=0):
    C = q0.shape[0]
    dev = q0.device
    nrec = n // thin
    res = {'state': torch.empty_like(q0),
           'samples': torch.full((nrec, C, D), -7.0, dtype=torch.float64, device=dev) if nrec else None,
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
    if res['samples'] is None:
        del res['samples']
    return res, eb, ea


def assert_same_bits(fast, exact):
    assert sorted(fast) == sorted(exact)
    for name in fast:
        assert torch.equal(bits(fast[name]), bits(exact[name])), name


@pytest.mark.parametrize('mode', [_native.MODE_EXACT, _native.MODE_FMA])
@pytest.mark.parametrize('L', [1, 2, 4, 5, 7, 20])
@pytest.mark.parametrize('thin', [1, 2])
@pytest.mark.parametrize('C', CHAINS)
def test_two_sum_path_equals_exact_path(device, C, thin, L, mode):
    assert _native.gauss_waves_per_chain(C, D) == 1
    q0, p0, u = draws(device, C)
    rates = []
    for n in (1, 2, 5, 9):
        fast, _, _ = run(q0, p0, u, n, thin, L, False, mode=mode)
        exact, eb, ea = run(q0, p0, u, n, thin, L, True, mode=mode)
        assert_same_bits(fast, exact)
        assert torch.isfinite(eb).all() and torch.isfinite(ea).all()
        rates.append(exact['accepted'].double().mean().item())
    print('C=%d L=%d: acceptance %s' % (C, L, ' '.join('%.3f' % r for r in rates)))
    assert 0.05 < rates[-1] < 0.999                           # both branches of the tail ran


def special_start(q0, p0):
    """Chains 0 / 1 / 2: an inf, a NaN in the state, a momentum whose square overflows."""
    q0, p0 = q0.clone(), p0.clone()
    q0[0, 5] = float('inf')
    q0[1, D - 1] = float('nan')
    p0[:, 2, 77] = 1e160
    return q0, p0


@pytest.mark.parametrize('mode', [_native.MODE_EXACT, _native.MODE_FMA])
@pytest.mark.parametrize('L', [1, 5, 20])
@pytest.mark.parametrize('thin', [1, 2])
@pytest.mark.parametrize('C', CHAINS)
def test_inf_nan_and_overflowing_momentum(device, C, thin, L, mode):
    q0, p0, u = draws(device, C)
    q0, p0 = special_start(q0, p0)
    n = 5
    fast, _, _ = run(q0, p0, u, n, thin, L, False, mode=mode)
    exact, eb, ea = run(q0, p0, u, n, thin, L, True, mode=mode)
    assert_same_bits(fast, exact)
    assert not exact['accepted'][:, :3].any()                 # rejected, state kept
    assert torch.equal(bits(fast['state'][:3]), bits(q0[:3]))
    assert torch.isinf(eb[:, 2]).all()


def nearest_exp(x):
    """The double nearest e^x."""
    return float(Decimal(float(x)).exp())


@pytest.mark.parametrize('mode', [_native.MODE_EXACT, _native.MODE_FMA])
@pytest.mark.parametrize('L', [1, 20])
@pytest.mark.parametrize('thin', [1, 2])
@pytest.mark.parametrize('C', CHAINS)
def test_forced_fallback_returns_the_exact_bits(device, C, thin, L, mode):
    getcontext().prec = 40
    n = 3
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
    fast, _, _ = run(q0, p0, u, n, thin, L, False, mode=mode)
    exact, eb, ea = run(q0, p0, u, n, thin, L, True, mode=mode)
    assert_same_bits(fast, exact)
    acc = exact['accepted'].cpu().numpy()
    assert not acc[:, :3].any()
    assert torch.equal(bits(fast['state'][:3]), bits(q0[:3]))
    placed = acc[:, 3:]                                       # u one ulp either side of the threshold
    assert 0.1 < placed.mean() < 0.9


@pytest.mark.parametrize('kw', [dict(dt=1.5), dict(n_adapt=3), dict(k=3.7, x0=2.0)],
                         ids=['dt=1.5', 'adaption', 'non-unit'])
@pytest.mark.parametrize('mode', [_native.MODE_EXACT, _native.MODE_FMA])
@pytest.mark.parametrize('thin', [1, 2])
@pytest.mark.parametrize('C', CHAINS)
def test_outside_the_domain(device, C, thin, mode, kw):
    q0, p0, u = draws(device, C)
    if 'k' in kw:
        q0 = kw['x0'] + q0 / np.sqrt(kw['k'])
    L = 1 if 'dt' in kw else 5                                # dt = 1.5: one step keeps some accepts
    fast, _, _ = run(q0, p0, u, 5, thin, L, False, mode=mode, **kw)
    exact, _, _ = run(q0, p0, u, 5, thin, L, True, mode=mode, **kw)
    assert_same_bits(fast, exact)
