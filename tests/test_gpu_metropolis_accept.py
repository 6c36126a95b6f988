"""`metropolis_accept(u, x)` (gauss_common.hpp), the accept test shared by the HMC
kernels, through `binf_accept_select_f64`: it must return exactly
`u < exp_clipped_range(clip(x, -308, 709))`, although it evaluates the exponential
only where the bounds 1 + x <= e^x <= 1 + x + x^2/2 (less / plus a margin of 2^-40)
do not already decide.  The expected flag is `u < y` with y from the same device's
`clipped_exp`; u is placed on and around y and on and around both bounds, where a
wrong margin or a wrong branch would flip a decision."""
import numpy as np
import pytest
import torch

from binf_amd import _native

pytestmark = pytest.mark.gpu

MARGIN = 2.0 ** -40


def dev_t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def shifted(v, k):
    """v moved by k ulps (k < 0: towards -inf)."""
    out = v.copy()
    for _ in range(abs(k)):
        out = np.nextafter(out, np.inf if k > 0 else -np.inf)
    return out


def exponents():
    rs = np.random.RandomState(151)
    tiny = 10.0 ** rs.uniform(-300.0, -3.0, size=30000)
    half = np.float64(-0.5)
    special = [0.0, -0.0, -308.0, 709.0, -308.5, -400.0, -1e300, 709.5, 800.0, 1e300,
               np.inf, -np.inf, np.nan, 5e-324, -5e-324, 1e-310, -1e-310,
               2.0 ** -40, -2.0 ** -40, 2.0 ** -41, -2.0 ** -41, 1.0, -1.0]
    special += [float(shifted(np.array([half]), k)[0]) for k in range(-4, 5)]
    return np.concatenate([rs.uniform(-1.0, 1.0, size=30000), tiny[:15000], -tiny[15000:],
                           np.array(special)])


def test_same_decision_as_the_clipped_exponential(device):
    x = exponents()
    y = _native.clipped_exp(dev_t(x, device)).cpu().numpy()
    with np.errstate(invalid='ignore', over='ignore'):
        lower = 1.0 + x
        upper = 1.0 + x + x * x * 0.5
    us = []
    for centre in (y, lower, upper):
        for k in range(-4, 5):
            us.append(shifted(centre, k))
    for v in (0.0, 5e-324, 1.0 - 2.0 ** -53, 1.0, 1.5, np.nan):
        us.append(np.full_like(x, v))
    u = np.stack(us, axis=1)                                  # [len(x), 33]
    xx = np.repeat(x[:, None], u.shape[1], axis=1)
    yy = np.repeat(y[:, None], u.shape[1], axis=1)
    u, xx, yy = u.ravel(), xx.ravel(), yy.ravel()
    n = u.size
    assert 1.9e6 < n < 2.6e6

    # which path decides, from the documented bounds
    with np.errstate(invalid='ignore', over='ignore'):
        small = (xx >= -0.5) & (xx < 0.0)
        fast_acc = ((xx >= 0.0) & (u < 1.0)) | (small & (u < (1.0 + xx) - MARGIN))
        fast_rej = ~fast_acc & small & (u >= (1.0 + xx + xx * xx * 0.5) + MARGIN)
        want = u < yy
    slow = ~(fast_acc | fast_rej)
    print('pairs %d: fast accept %.3f, fast reject %.3f, exponential %.3f'
          % (n, fast_acc.mean(), fast_rej.mean(), slow.mean()))
    assert slow.mean() >= 0.25
    assert fast_acc.sum() > 10000 and fast_rej.sum() > 10000

    q_prop = torch.ones((n, 1), dtype=torch.float64, device=device)
    q_old = torch.zeros((n, 1), dtype=torch.float64, device=device)
    q_out = torch.full((n, 1), -1.0, dtype=torch.float64, device=device)
    acc = torch.full((n,), 7, dtype=torch.uint8, device=device)
    e_before = torch.zeros(n, dtype=torch.float64, device=device)
    _native.accept_select(q_prop, q_old, e_before, dev_t(-xx, device), dev_t(u, device),
                          q_out, acc)
    torch.cuda.synchronize()
    got = acc.cpu().numpy()
    bad = np.nonzero(got != want.astype(np.uint8))[0]
    assert bad.size == 0, [(xx[i], u[i], yy[i], int(got[i])) for i in bad[:5]]
    assert np.array_equal(q_out.cpu().numpy()[:, 0], want.astype(np.float64))


def test_clipped_exp_is_at_least_one_from_zero_up(device):
    """What the x >= 0 fast path rests on."""
    rs = np.random.RandomState(152)
    grid = np.arange(2048) * (np.log(2.0) / 2.0)
    edges = np.concatenate([shifted(grid, k) for k in range(-4, 5)])
    edges = edges[edges >= 0.0]
    sub = np.arange(1, 1025) * 5e-324
    fill = 1000000 - edges.size - sub.size - 5
    x = np.concatenate([[0.0, 709.0, 2.2250738585072014e-308, 710.0, 1e300], sub, edges,
                        rs.uniform(0.0, 709.0, size=fill // 2),
                        10.0 ** rs.uniform(-300.0, 2.85, size=fill - fill // 2)])
    assert x.size == 1000000 and np.all(x >= 0.0)
    y = _native.clipped_exp(dev_t(x, device)).cpu().numpy()
    bad = np.nonzero(~(y >= 1.0))[0]
    assert bad.size == 0, [(x[i], y[i]) for i in bad[:5]]
