"""The bound behind the fused energy sums of the Gaussian HMC kernel (FASTSUM,
hmc_gauss_kernel.hpp; derivation above accept_decide in gauss_common.hpp), on the host.

The kernel that records no energies accumulates its three sums of squares as
acc = fma(x, x, acc) -- one rounding per element -- and decides u < exp(x~) from them,
x~ = -(Ea~ - Eb~), unless u lies within delta = 2^-46 (Eb~ + Ea~) of the threshold.  That
is sound if the exponent of the sums in numpy's order, x, is never further than delta
from x~.  Here both orders are restated for the lanes and the tree of D = 768 / 1024
(the fused multiply-add exactly: math.fma, or rationals where the interpreter has
none) and |x~ - x| <= delta is asserted for every case; the derived bound is
delta / 2.5, the worst observed ratio is printed."""
import math
from fractions import Fraction

import numpy as np
import pytest

DELTA_SCALE = 2.0 ** -46


def fma(a, b, c):
    if hasattr(math, 'fma'):
        return math.fma(a, b, c)
    return float(Fraction(a) * Fraction(b) + Fraction(c))      # correctly rounded


def tree(acc):
    """[8 leaves][8 accumulators] -> np.sum's result: ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7))
    inside a leaf, the leaves joined pairwise, 0.0 + r."""
    leaves = []
    for r in acc:
        leaves.append(((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7])))
    while len(leaves) > 1:
        leaves = [leaves[i] + leaves[i + 1] for i in range(0, len(leaves), 2)]
    return 0.0 + leaves[0]


def sumsq(d, fused):
    """Sum of d**2 over a row of 768 / 1024 elements: lane (leaf g, accumulator j) owns
    elements g * len + 8 t + j, t = 0 .. len / 8 - 1."""
    n = d.size // 8
    acc = []
    for g in range(8):
        row = []
        for j in range(8):
            x = [float(v) for v in d[g * n + j:(g + 1) * n:8]]
            s = x[0] * x[0]
            for v in x[1:]:
                s = fma(v, v, s) if fused else s + v * v
            row.append(s)
        acc.append(row)
    return tree(acc)


def exponent_and_delta(q0, p0, q1, p1, k, x0, fused):
    c_lp = -0.5 * k
    s = [sumsq(v, fused) for v in (q0 - x0, p0, q1 - x0, p1)]
    eb = -(c_lp * s[0]) + 0.5 * s[1]
    ea = -(c_lp * s[2]) + 0.5 * s[3]
    return -(ea - eb), DELTA_SCALE * (eb + ea), s


def leapfrog(q, p, dt, L, k, x0):
    q, p = q.copy(), p.copy()
    p = p - 0.5 * dt * (k * (q - x0))
    for _ in range(L - 1):
        q = q + p * dt
        p = p - dt * (k * (q - x0))
    q = q + p * dt
    p = p - 0.5 * dt * (k * (q - x0))
    return q, p


def cases(D):
    rs = np.random.RandomState(4600 + D)
    out = []
    for scale in (1e-150, 1.0, 1e150):
        for _ in range(3):
            out.append(('scale %g' % scale, [scale * rs.standard_normal(D) for _ in range(4)], 1.0, 0.0))
    for _ in range(3):                                          # magnitudes mixed inside a row
        out.append(('mixed', [rs.standard_normal(D) * 10.0 ** rs.uniform(-8.0, 8.0, size=D)
                              for _ in range(4)], 1.0, 0.0))
    for dt, k, x0 in ((0.2, 1.0, 0.0), (1e-3, 1.0, 0.0), (0.05, 2.5, 0.3), (0.3, 1.0, 0.0)):
        for _ in range(2):                                      # a real trajectory: dH ~ 0
            q0 = x0 + rs.standard_normal(D) / np.sqrt(k)
            p0 = rs.standard_normal(D)
            q1, p1 = leapfrog(q0, p0, dt, 3, k, x0)
            out.append(('trajectory dt=%g' % dt, [q0, p0, q1, p1], k, x0))
    q = rs.standard_normal(D)                                   # dH == 0: the state unchanged
    p = rs.standard_normal(D)
    out.append(('identical', [q, p, q, p], 1.0, 0.0))
    return out


@pytest.mark.parametrize('D', [768, 1024])
def test_fused_exponent_within_delta_of_numpy_order(D):
    worst = 0.0
    for name, (q0, p0, q1, p1), k, x0 in cases(D):
        x, _, s = exponent_and_delta(q0, p0, q1, p1, k, x0, fused=False)
        # the restated lanes and tree are numpy's: bit for bit
        for got, v in zip(s, (q0 - x0, p0, q1 - x0, p1)):
            assert got == np.sum(v * v), name
        xt, delta, _ = exponent_and_delta(q0, p0, q1, p1, k, x0, fused=True)
        assert math.isfinite(x) and math.isfinite(xt) and delta >= 0.0, name
        err = abs(Fraction(xt) - Fraction(x))
        assert err <= Fraction(delta), (name, x, xt, delta)
        if delta > 0.0:
            worst = max(worst, float(err / Fraction(delta)))
    print('D = %d: worst |x~ - x| / delta = %.4f (derived bound: 1 / 2.5 = 0.4)' % (D, worst))
    assert worst <= 0.4
