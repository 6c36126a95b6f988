"""`accept_decide(u, x, delta)` (gauss_common.hpp), the accept test of an exponent that is
only known to within delta, through `binf_accept_decide_f64`, against exact arithmetic
(decimal, 60 digits).  u is placed at the correctly rounded e^x and one and two ulps
either side, at e^(x -+ delta), on and around the bounds 1 + xl - 2^-40 and
1 + xh + xh^2 / 2 + 2^-40 and far from all of them:
  * UNDECIDED whenever |u - e^x| <= e^x delta;
  * never ACCEPT where u >= e^(x + delta), never REJECT where u < e^(x - delta);
  * a decided answer is the flag the exact test (`binf_accept_select_f64`) gives at x;
  * every non-finite input, u outside [0, 1) and delta outside [0, 2^-21]: UNDECIDED."""
from decimal import Decimal, getcontext

import numpy as np
import pytest
import torch

from binf_amd import _native

pytestmark = pytest.mark.gpu

REJECT, ACCEPT, UNDECIDED = 0, 1, 2
MARGIN = 2.0 ** -40


def dev_t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def shifted(v, k):
    out = np.array(v, dtype=np.float64)
    for _ in range(abs(k)):
        out = np.nextafter(out, np.inf if k > 0 else -np.inf)
    return out


def decide(device, u, x, delta):
    out = _native.accept_decide(dev_t(u, device), dev_t(x, device), dev_t(delta, device))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def exact_flags(device, u, x):
    """u < exp_clipped_range(clip(x)): what the kernels that keep numpy's sums decide."""
    n = u.size
    one = torch.ones((n, 1), dtype=torch.float64, device=device)
    zero = torch.zeros((n, 1), dtype=torch.float64, device=device)
    q_out = torch.empty((n, 1), dtype=torch.float64, device=device)
    acc = torch.full((n,), 7, dtype=torch.uint8, device=device)
    _native.accept_select(one, zero, torch.zeros(n, dtype=torch.float64, device=device),
                          dev_t(-x, device), dev_t(u, device), q_out, acc)
    torch.cuda.synchronize()
    return acc.cpu().numpy()


def exponents():
    grid = np.linspace(-2.0, 0.25, 181)
    edges = [float(shifted(c, k)) for c in (-0.5, 0.0) for k in range(-3, 4)]
    small = [s * 10.0 ** -e for e in (1, 2, 3, 5, 8, 11, 12, 14, 16, 20, 40, 300) for s in (1.0, -1.0)]
    far = [-308.0, -309.0, -1e4, -40.0, -27.0, -5.0, 0.7, 3.0, 709.0, 710.0, 1e4, 5e-324, -5e-324]
    return np.array(list(grid) + edges + small + far)


DELTAS = [0.0, 5e-324, 2.0 ** -60, 2.0 ** -46 * 1024.0, 2.0 ** -46 * 2048.0, 2.0 ** -30, 2.0 ** -22,
          float(shifted(2.0 ** -21, -1)), 2.0 ** -21]


def test_three_answers_against_exact_arithmetic(device):
    getcontext().prec = 60
    us, xs, ds = [], [], []
    lo_e, mid_e, hi_e = [], [], []           # e^(x - delta), e^x, e^(x + delta), exact
    for x in exponents():
        for delta in DELTAS:
            dx, dd = Decimal(float(x)), Decimal(delta)
            mid, lo, hi = dx.exp(), (dx - dd).exp(), (dx + dd).exp()
            xl, xh = x - delta, x + delta
            centres = [float(mid), float(lo), float(hi), (1.0 + xl) - MARGIN,
                       (1.0 + xh + xh * xh * 0.5) + MARGIN]
            cand = [shifted(c, k) for c in centres for k in range(-2, 3)]
            cand += [0.5 * float(mid), min(2.0 * float(mid), 0.75), 0.0, 5e-324, 1.0 - 2.0 ** -53]
            for u in cand:
                u = float(u)
                if not (0.0 <= u < 1.0):
                    continue                 # outside [0, 1): the last test
                us.append(u); xs.append(float(x)); ds.append(delta)
                lo_e.append(lo); mid_e.append(mid); hi_e.append(hi)
    u, x, d = np.array(us), np.array(xs), np.array(ds)
    got = decide(device, u, x, d)
    flag = exact_flags(device, u, x)
    assert set(np.unique(got)) <= {REJECT, ACCEPT, UNDECIDED}

    must_be_undecided = 0
    for i in range(u.size):
        du = Decimal(float(u[i]))
        if abs(du - mid_e[i]) <= mid_e[i] * Decimal(float(d[i])):
            must_be_undecided += 1
            assert got[i] == UNDECIDED, (u[i], x[i], d[i], int(got[i]))
        if du >= hi_e[i] and x[i] + d[i] <= 709.0:
            assert got[i] != ACCEPT, (u[i], x[i], d[i])
        if du < lo_e[i] and x[i] - d[i] >= -308.0:
            assert got[i] != REJECT, (u[i], x[i], d[i])
        if got[i] != UNDECIDED:
            assert got[i] == flag[i], (u[i], x[i], d[i], int(got[i]), int(flag[i]))
    frac = [(got == v).mean() for v in (REJECT, ACCEPT, UNDECIDED)]
    print('%d triples: reject %.3f accept %.3f undecided %.3f; %d inside delta of the threshold'
          % (u.size, frac[0], frac[1], frac[2], must_be_undecided))
    assert must_be_undecided > 2000
    assert frac[0] > 0.05 and frac[1] > 0.05
    # u far from the threshold is decided: the window is 2 delta e^x + 2^-40 on either side
    far = (np.abs(u - np.exp(np.clip(x, -308.0, 0.0))) > 1e-5) & (np.abs(x) < 300.0)
    assert far.sum() > 1000 and np.all(got[far] != UNDECIDED)


def test_inputs_outside_the_domain_are_undecided(device):
    bad = [np.nan, np.inf, -np.inf]
    rows = []
    for x in (-0.3, 0.0, 0.2, -40.0):
        for u in (0.0, 0.3, 0.9):
            for v in bad:
                rows += [(v, x, 2.0 ** -35), (u, v, 2.0 ** -35), (u, x, v), (v, v, v)]
            rows += [(1.0, x, 2.0 ** -35), (1.5, x, 2.0 ** -35), (-0.25, x, 2.0 ** -35), (-0.0, x, 0.0),
                     (u, x, -2.0 ** -35), (u, x, float(shifted(2.0 ** -21, 1))), (u, x, 1.0), (u, x, 1e300)]
    a = np.array(rows)
    got = decide(device, a[:, 0], a[:, 1], a[:, 2])
    assert np.all(got == UNDECIDED), a[got != UNDECIDED][:5]
