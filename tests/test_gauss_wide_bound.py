"""The bound behind the two-sum accept decision, for the lane order of the kernel with 16-byte
ownership (WIDE, hmc_gauss_kernel.hpp), on the host.

The WIDE kernel's lane l holds elements 128 r + 2 l + b (r = 0..7, b = 0..1) in slot 2 r + b and
sums acc = fma(x, x, acc) over its 16 slots in slot order; the 64 lane partials then climb the
same tree of six levels (chain_sums_shared2).  The derivation of delta (above accept_decide and
gauss_onesum_factor, gauss_common.hpp) counts roundings by depth alone, 16 in the lane and 6 in
the tree, so it must hold for this order as it does for numpy's ownership: asserted here in
rational arithmetic, |x~ - xe| <= delta / 2, over the grid of L, dt and scales of
test_gauss_onesum_bound.py, against the exponent numpy's sums of the same float64 trajectory
give.  The worst observed ratio is printed and kept in `worst_seen`; it is no threshold.
Observed: 0.0097 at L = 2, 0.0029 at L = 20, 0.0001 at L = 32764, in both modes -- the figures of
numpy's ownership (HISTORY 43), against the derived (66 + 24 L) / (128 + 32 L) = 0.56 ... 0.75."""
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle import c_oracle
from test_gauss_fastsum_bound import fma
from test_gauss_onesum_bound import D, K, L_MAX, factor, np_sumsq, starts, steps, trajectory

worst_seen = {}


def wide_sumsq(d):
    """[..., 1024] -> [...]: lane l owns elements 128 r + 2 l + b, slot 2 r + b, and sums
    acc = fma(x, x, acc) in slot order; the tree above the lanes joins neighbours, level by
    level (xor 1, 2, 4, 8, 16, 32), and ends with np.add.reduce's 0.0 + r."""
    x = d.reshape(d.shape[:-1] + (8, 64, 2))                  # [r, lane, b]
    acc = x[..., 0, :, 0] * x[..., 0, :, 0]
    for t in range(1, 16):
        v = x[..., t // 2, :, t % 2]
        acc = c_oracle.fma(v, v, acc)
    r = acc
    while r.shape[-1] > 1:
        r = r[..., 0::2] + r[..., 1::2]
    return 0.0 + r[..., 0]


def test_wide_sum_restatement():
    """The vectorised restatement against a scalar one written from the mapping."""
    rs = np.random.RandomState(2)
    d = rs.standard_normal((2, D))
    for row, got in zip(d, wide_sumsq(d)):
        lanes = []
        for l in range(64):
            own = [float(row[128 * r + 2 * l + b]) for r in range(8) for b in range(2)]
            s = own[0] * own[0]
            for v in own[1:]:
                s = fma(v, v, s)
            lanes.append(s)
        while len(lanes) > 1:
            lanes = [lanes[i] + lanes[i + 1] for i in range(0, len(lanes), 2)]
        assert got == 0.0 + lanes[0]
        # every element once: the exact sum of squares is the same as in numpy's ownership
        assert abs(Fraction(float(got)) - sum(Fraction(float(v)) ** 2 for v in row)) <= \
            Fraction(22, 2 ** 53) * sum(Fraction(float(v)) ** 2 for v in row) * Fraction(101, 100)


@pytest.mark.parametrize('use_fma', [False, True], ids=['exact', 'fma'])
@pytest.mark.parametrize('L', [1, 2, 3, 4, 5, 20, 63, L_MAX])
def test_wide_order_exponent_within_half_delta_of_numpy_order(L, use_fma):
    names, q0, p0 = starts()
    dts = steps(L)
    dt = np.array(dts).reshape(-1, 1, 1)
    q0 = np.broadcast_to(q0, (len(dts),) + q0.shape).copy()
    p0 = np.broadcast_to(p0, (len(dts),) + p0.shape).copy()
    q1, p1 = trajectory(q0, p0, dt, L, use_fma)
    c_lp = -0.5 * K
    f = factor(L)
    # numpy's side (hmc.py:143-151)
    eb = -(c_lp * np_sumsq(q0)) + 0.5 * np_sumsq(p0)
    ea = -(c_lp * np_sumsq(q1)) + 0.5 * np_sumsq(p1)
    xe = -(ea - eb)
    # the kernel's side, in the WIDE lane order
    sq0, spb, sqa = wide_sumsq(q0), wide_sumsq(p0), wide_sumsq(q1)
    worst = 0.0
    for i, h in enumerate(dts):
        c_dh = ((K * h) * (K * h)) * 0.125
        for j, name in enumerate(names):
            xt = -(c_dh * (sqa[i, j] - sq0[i, j]))
            ebt = -(c_lp * sq0[i, j]) + 0.5 * spb[i, j]
            delta = f * ((ebt + ebt) + abs(xt))
            assert math.isfinite(xe[i, j]) and math.isfinite(xt) and math.isfinite(delta), (name, h)
            err = abs(Fraction(xt) - Fraction(float(xe[i, j])))
            assert err <= Fraction(delta) / 2, (name, h, L, float(xe[i, j]), xt, delta)
            worst = max(worst, float(err / (Fraction(delta) / 2)))
    worst_seen[(L, use_fma)] = worst
    print('L = %d, %s: worst |x~ - xe| / (delta / 2) = %.4f' % (L, 'fma' if use_fma else 'exact', worst))
