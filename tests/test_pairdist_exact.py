"""The exact references of tests/pairdist_exact.py checked on their own (CPU): the
correctly rounded sqrt against numpy's IEEE sqrt, the hard cases against their
stated distance from a rounding midpoint (rational arithmetic), the realised
coordinates against the squared distance they must reproduce, and the 50-digit
force against the numpy formulation on random data."""
import math
from fractions import Fraction

import numpy as np
import pytest

import pairdist_exact as PE
from oracle import ref_distance as RD


def test_hard_cases_are_within_c_2_minus_55_ulps_of_a_midpoint():
    cases = PE.hard_cases()
    assert len(cases) >= 100
    binades = {math.frexp(h.s)[1] for h in cases}
    assert len(binades) >= 8                          # [1, 2) and [2, 4) at every scale
    for h in cases:
        assert PE.check_near_midpoint(h), (h.M, h.c, h.side, h.k)
        # and NOT on the midpoint: M^2 -+ c is no square of a multiple of the half ulp
        assert Fraction(h.s) != h.midpoint() ** 2


def test_cr_sqrt_matches_numpy_on_the_hard_cases_and_the_edges():
    for h in PE.hard_cases():
        r = PE.cr_sqrt(h.s)
        assert r == h.expected() == float(np.sqrt(h.s)), (h.M, h.c, h.side, h.k)
    for s in PE.edge_values():
        assert PE.cr_sqrt(s) == float(np.sqrt(s)), s
    assert PE.cr_sqrt(0.0) == 0.0 and PE.cr_sqrt(math.inf) == math.inf
    assert math.isnan(PE.cr_sqrt(-1.0))


def test_cr_sqrt_matches_numpy_on_random_doubles():
    rs = np.random.RandomState(7)
    bits = rs.randint(0, 2 ** 62, size=3000, dtype=np.int64) & 0x7fefffffffffffff
    for s in bits.view(np.float64):
        assert PE.cr_sqrt(s) == float(np.sqrt(s)), s
    # exact squares: the tie rule never applies, the root is exact
    for v in rs.uniform(0.1, 10.0, size=200):
        v = float(np.float32(v))
        assert PE.cr_sqrt(v * v) == v


def test_realised_coordinates_reproduce_s_exactly():
    for s in [h.s for h in PE.hard_cases()] + PE.edge_values():
        a, b = PE.realise(s)
        assert PE.fp_sq(a, b, 0.0) == s, s
        # a carries at most 26 significant bits: a*a is exact where it is normal
        if a != 0.0:
            m = Fraction(a).numerator
            assert (m >> ((m & -m).bit_length() - 1)).bit_length() <= 26
            if a * a > 2.0 ** -1022:
                assert Fraction(a * a) == Fraction(a) ** 2
        # numpy evaluates the same expression to the same bits
        d = np.array([[a, b, 0.0]])
        assert np.sum(d ** 2, axis=1)[0] == s


@pytest.mark.parametrize('n,seed', [(5, 0), (12, 1), (30, 2)])
def test_decimal_force_agrees_with_the_numpy_formulation(n, seed):
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((n, 3)) * 2.0
    I, J = np.triu_indices(n, 1)
    ys = np.abs(RD.forward(x.reshape(-1), n) + 0.1 * rs.standard_normal(len(I)))
    ymat = np.zeros((n, n))
    ymat[I, J] = ys
    ymat[J, I] = ys
    tau = 1.7
    rows = list(range(n))
    ex = PE.force_rows(x, ymat, tau, rows)
    A, W = PE.force_scales(x, ymat, rows)
    g = RD.gradient(x.reshape(-1), ys, tau, n).reshape(n, 3)
    u = PE.U
    for i in rows:
        for k in range(3):
            # numpy: d correctly rounded from an s of three rounded terms, one division, one
            # multiplication by the difference, n - 1 additions (np.add.at)
            bound = tau * (8 * u * A[i][k] + (n + 4) * u * W[i][k])
            assert abs(float(ex[i][k]) - g[i, k]) <= bound, (i, k)


def test_decimal_force_is_nan_for_coincident_beads_only():
    x = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 2.0], [1.0, 2.0, 2.0], [4.0, 0.0, 0.0]])
    ymat = np.ones((4, 4))
    f = PE.force_rows(x, ymat, 1.0, range(4))
    assert all(v.is_nan() for v in f[1] + f[2])
    assert not any(v.is_nan() for v in f[0] + f[3])
    # the numpy formulation's pattern is the same (d = 0: 0 * inf)
    with np.errstate(divide='ignore', invalid='ignore'):
        g = RD.gradient(x.reshape(-1), ymat[np.triu_indices(4, 1)], 1.0, 4).reshape(4, 3)
    assert np.array_equal(np.isnan(g), np.array([[v.is_nan() for v in f[i]] for i in range(4)]))


def test_exact_leapfrog_matches_a_float_leapfrog_to_rounding():
    n = 6
    rs = np.random.RandomState(3)
    x = rs.standard_normal((n, 3))
    I, J = np.triu_indices(n, 1)
    ys = np.abs(RD.forward(x.reshape(-1), n) + 0.1)
    ymat = np.zeros((n, n))
    ymat[I, J] = ys
    ymat[J, I] = ys
    p0 = rs.standard_normal((n, 3))
    dt, L, tau, prior = 0.01, 3, 2.0, (0.05, 0.1)
    q, p, grads = PE.exact_leapfrog(x, p0, ymat, tau, prior, dt, L)
    assert len(grads) == L + 1
    post = RD.DistancePosterior(ys, tau, n)

    def grad(v):
        return post.gradient(coordinates=v) + prior[0] * (v - prior[1])
    qf, pf = x.reshape(-1).copy(), p0.reshape(-1).copy()
    pf = pf - 0.5 * dt * grad(qf)
    for _ in range(L - 1):
        qf = qf + dt * pf
        pf = pf - dt * grad(qf)
    qf = qf + dt * pf
    pf = pf - 0.5 * dt * grad(qf)
    assert np.allclose(PE.to_f64(q).reshape(-1), qf, rtol=0, atol=1e-14)
    assert np.allclose(PE.to_f64(p).reshape(-1), pf, rtol=0, atol=1e-13)
