"""The bound behind the two-sum accept decision of the Gaussian HMC kernel (ONESUM,
hmc_gauss_kernel.hpp; derivation above gauss_onesum_factor in gauss_common.hpp), on the host.

For the unit Gaussian the kernel forms the exponent of the accept test without any momentum,
x~ = -(c (Sq'~ - Sq~)), c = k^2 dt^2 / 8, from the fused sums of squares of the start and the end
position, and decides u < exp(x~) unless u lies within delta = f(L) (2 Eb~ + |x~|) of the
threshold, f(L) = (128 + 32 L) 2^-53.  That is sound if xe, the exponent numpy's sums of the
same float64 trajectory give (final half kick included), is never further than delta / 2 from
x~: accept_decide's precondition, asserted here in rational arithmetic for every case.  The
trajectory is restated in both arithmetic modes (FMA: C99 fma, oracle/), the fused sums for the
lanes and the tree of D = 1024.  The worst observed ratio is printed; it is no threshold."""
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle import c_oracle
from test_gauss_fastsum_bound import sumsq

D = 1024
L_MAX = 32764            # the dispatch's largest L: f(L) 2^12 <= 2^-21 (gauss_onesum_domain)
K = 1.0


def factor(L):
    return 2.0 ** -46 + L * 2.0 ** -48


def test_largest_L_of_the_dispatch():
    assert factor(L_MAX) * 2.0 ** 12 <= 2.0 ** -21 < factor(L_MAX + 1) * 2.0 ** 12
    assert Fraction(factor(L_MAX)) == Fraction(128 + 32 * L_MAX, 2 ** 53)       # f is exact


def fused_sumsq(d):
    """[..., 1024] -> [...]: lane (leaf g, accumulator j) owns elements 128 g + 8 t + j and sums
    acc = fma(x, x, acc); the tree above the accumulators is np.sum's."""
    x = d.reshape(d.shape[:-1] + (8, 16, 8))
    acc = x[..., 0, :] * x[..., 0, :]
    for t in range(1, 16):
        acc = c_oracle.fma(x[..., t, :], x[..., t, :], acc)
    r = ((acc[..., 0] + acc[..., 1]) + (acc[..., 2] + acc[..., 3])) + \
        ((acc[..., 4] + acc[..., 5]) + (acc[..., 6] + acc[..., 7]))
    while r.shape[-1] > 1:
        r = r[..., 0::2] + r[..., 1::2]
    return 0.0 + r[..., 0]


def np_sumsq(d):
    return np.sum(d * d, axis=-1)        # contiguous rows of 1024: numpy's pairwise order


def trajectory(q, p, dt, L, use_fma):
    """hmc.py:116-123 for the unit Gaussian: (q', p') with the final half kick, and dt of shape
    [ndt, 1, 1] against states [ndt, S, D]."""
    hdt = 0.5 * dt
    if use_fma:
        p = c_oracle.fma(-hdt, q, p)
        for _ in range(L - 1):
            q = c_oracle.fma(p, dt, q)
            p = c_oracle.fma(-dt, q, p)
        q = c_oracle.fma(p, dt, q)
        p = c_oracle.fma(-hdt, q, p)
    else:
        p = p - hdt * q
        for _ in range(L - 1):
            q = q + p * dt
            p = p - dt * q
        q = q + p * dt
        p = p - hdt * q
    return q, p


def starts():
    rs = np.random.RandomState(5300)
    n = lambda: rs.standard_normal(D)
    mixed = lambda: rs.standard_normal(D) * 10.0 ** rs.uniform(-8.0, 8.0, size=D)
    out = [('scale 1e-150', 1e-150 * n(), 1e-150 * n()), ('scale 1', n(), n()),
           ('scale 1e150', 1e150 * n(), 1e150 * n()), ('mixed', mixed(), mixed()),
           ('mixed, scale 1e-140', 1e-140 * mixed(), 1e-140 * mixed()),
           ('mixed, scale 1e140', 1e140 * mixed(), 1e140 * mixed()),
           ('q-dominated', n(), 1e-8 * n()), ('p-dominated', 1e-8 * n(), n())]
    return [o[0] for o in out], np.stack([o[1] for o in out]), np.stack([o[2] for o in out])


def steps(L):
    """0.05, 0.5, the edge of k dt^2 <= 1 and, where it lies inside, the dt of L theta = pi
    (cos theta = 1 - dt^2 / 2): q' = -q up to rounding, dH ~ 0."""
    dts = [0.05, 0.5, 1.0]
    pi_dt = 2.0 * math.sin(math.pi / (2.0 * L))
    if pi_dt <= 1.0:
        dts.append(pi_dt)
    return dts


def test_fused_sum_restatement():
    rs = np.random.RandomState(1)
    d = rs.standard_normal((2, D))
    for row, got, got_np in zip(d, fused_sumsq(d), np_sumsq(d)):
        assert got == sumsq(row, True)
        assert got_np == sumsq(row, False)


@pytest.mark.parametrize('use_fma', [False, True], ids=['exact', 'fma'])
@pytest.mark.parametrize('L', [1, 2, 3, 4, 5, 20, 63, L_MAX])
def test_two_sum_exponent_within_half_delta_of_numpy_order(L, use_fma):
    names, q0, p0 = starts()
    dts = steps(L)
    dt = np.array(dts).reshape(-1, 1, 1)
    q0 = np.broadcast_to(q0, (len(dts),) + q0.shape).copy()
    p0 = np.broadcast_to(p0, (len(dts),) + p0.shape).copy()
    q1, p1 = trajectory(q0, p0, dt, L, use_fma)
    if L * dts[-1] > 3.0:                                       # the L theta = pi row: q' ~ -q
        assert np.all(np.abs(q1[-1, 1] + q0[-1, 1]) < 1e-6 * (1.0 + np.abs(p0[-1, 1])))
    c_lp = -0.5 * K
    f = factor(L)
    # numpy's side (hmc.py:143-151)
    eb = -(c_lp * np_sumsq(q0)) + 0.5 * np_sumsq(p0)
    ea = -(c_lp * np_sumsq(q1)) + 0.5 * np_sumsq(p1)
    xe = -(ea - eb)
    # the kernel's side
    sq0, spb, sqa = fused_sumsq(q0), fused_sumsq(p0), fused_sumsq(q1)
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
    print('L = %d, %s: worst |x~ - xe| / (delta / 2) = %.4f' % (L, 'fma' if use_fma else 'exact', worst))
