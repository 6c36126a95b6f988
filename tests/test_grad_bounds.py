"""tests/grad_bounds.py is itself tested on the CPU: its exact force is the rational one, its
bounds contain numpy's force in several summation orders and reject injected errors that
the old ``1e-10 sum|A||r|`` bar let through, the float-evaluated bound is never below the
exact one, and the integer data of the GPU tests is exact in double precision in ANY order
of summation (a condition on the inputs, asserted from Python ints -- not a tolerance)."""
from fractions import Fraction

import numpy as np
import pytest

import grad_bounds as GB
import linear_bounds as LB


def test_self_test_bounds_hold_and_reject_what_the_old_bar_let_through():
    figs = GB.self_test()
    for f in figs:
        print(f)
    assert [(f['K'], f['N']) for f in figs] == [(5, 48), (33, 1040), (33, 16384)]
    for f in figs:
        assert f['bar_over_bound'] >= 50.0                   # gamma_16384 = 1.8e-12
        assert f['numpy'] <= 1.0
        assert f['tau_float32'] > 1.0
    assert all(f['mock_moved'] > 1.0 for f in figs[:2])
    assert all(f['product_dropped'] > 1.0 for f in figs[1:])


def test_exact_force_is_the_rational_force():
    rs = np.random.RandomState(3)
    K, N = 3, 5
    A = rs.standard_normal((K, N)) * 2.0 ** rs.randint(-20, 21, size=(K, 1))
    ys, theta, tau = rs.standard_normal(N), rs.standard_normal(K), 1.0 / 3.0
    fA = [[Fraction(float(v)) for v in row] for row in A]
    r = [(sum(Fraction(float(theta[k])) * fA[k][n] for k in range(K)) - Fraction(float(ys[n])))
         * Fraction(tau) for n in range(N)]
    want = [sum(fA[i][n] * r[n] for n in range(N)) for i in range(K)]
    ef = GB.ExactForce(A, ys)
    G, s = ef.force(theta, tau)
    assert [Fraction(int(g), 1 << s) for g in G] == want
    # the error of a value is measured from it: the rounded exact force is within half an ulp
    near = GB.exact_to_float((G, s))
    assert np.all(ef.error((G, s), near) <= 0.5 * np.spacing(np.abs(near)))
    off = near + 1.0
    assert np.array_equal(ef.error((G, s), off), [float(abs(Fraction(float(off[i])) - want[i])) for i in range(K)])
    # the contraction's exact error likewise
    J, v = rs.standard_normal((K, N)), rs.standard_normal(N)
    dot = [sum(Fraction(float(J[k, n])) * Fraction(float(v[n])) for n in range(N)) for k in range(K)]
    got = J.dot(v)
    assert np.array_equal(GB.contract_error(J, v, got), [float(abs(Fraction(float(got[k])) - dot[k])) for k in range(K)])
    assert np.all(GB.contract_error(J, v, got) <= GB.contract_bound(J, v))
    assert np.array_equal(GB.contract_bound(J, v), LB.gamma(N) * np.abs(J).dot(np.abs(v)) * LB.SLACK)


@pytest.mark.parametrize('kind', GB.DESIGNS)
@pytest.mark.parametrize('K,N', [(1, 1), (5, 48), (17, 35), (33, 272), (64, 31)])
def test_float_bound_is_never_below_the_exact_one(kind, K, N):
    C = 6
    A, ys, theta, tau = GB.float_case(kind, K, N, C, 100 * K + N)
    ef = GB.ExactForce(A, ys)
    for t in (2.5, tau):
        force, bound = GB.force_float(theta, A, ys, t)
        assert np.all(GB.old_bar(theta, A, ys, t) >= 50.0 * bound)
        for c in range(C):
            tc = float(np.broadcast_to(t, (C,))[c])
            info = ef.chain(theta[c], tc)
            assert np.all(bound[c] >= info['bound']), (c, float(np.min(bound[c] / info['bound'])))
            assert np.all(bound[c] <= 1.01 * info['bound'])      # ... and not vacuous beside it
            assert np.all(ef.error(info['G'], force[c]) <= info['bound'])


def test_integer_data_is_exact_in_any_order():
    """sum|terms| of every sum, in units of the granularity, fits 53 bits: the worst case of
    the generator's ranges for every shape of the GPU tests, and the actual data of one."""
    widths = {}
    for K, N, C in GB.force_cases():
        widths[(K, N)] = GB.integer_case_width(K, N)
    assert max(widths.values()) == widths[(64, 3072)] < 53
    print('integer force data: at most %d bits' % max(widths.values()))
    for K, N, C in ((33, 1027, 17), (64, 3072, 17), (5, 17, 4113)):
        A, ys, theta, tau = GB.integer_case(K, N, C, 7)
        assert set(np.unique(tau)) <= set(GB.INT_TAUS) and len(np.unique(A)) > 9
        ints = lambda x: np.array([int(v) for v in np.asarray(x).ravel()], dtype=object).reshape(np.shape(x))
        absA, absT = np.abs(ints(A)), np.abs(ints(theta))
        resid4 = (absT.dot(absA) + np.abs(ints(ys))) * ints(tau * 4)[:, None]       # quarters
        worst = max(int(v) for v in resid4.dot(absA.T).ravel())
        assert worst.bit_length() <= widths[(K, N)] < 53
        # the int64 reference is that exact value
        ef = GB.ExactForce(A, ys)
        want = GB.integer_force(A, ys, theta, tau)
        for c in (0, C - 1):
            assert np.array_equal(GB.exact_to_float(ef.force(theta[c], tau[c])), want[c])
            assert np.all(ef.error(ef.force(theta[c], tau[c]), want[c]) == 0.0)


@pytest.mark.parametrize('K,N,L,k', GB.LEAPFROG_CASES)
def test_integer_leapfrog_is_exact_in_any_order(K, N, L, k):
    for C in (17, 4100):
        A, ys, q, p, tau_exp = GB.leapfrog_case(K, N, C, K + N)
        dt_exp = k - (np.arange(C) % 2)
        for te, de in ((0, k), (tau_exp, k), (tau_exp, dt_exp)):
            Q, P, width = GB.leapfrog_ints(A, ys, q, p, te, de, L)
            print('K=%d N=%d L=%d dt=2**-%d C=%d: %d bits' % (K, N, L, k, C, int(width)))
            assert isinstance(width, int) and width < 53
            te_c, de_c = np.broadcast_to(te, (C,)), np.broadcast_to(de, (C,))
            for c in (0, 1, C - 1):
                fq, fp = GB.leapfrog_fraction(A, ys, q[c], p[c], Fraction(2) ** int(te_c[c]),
                                              Fraction(1, 2 ** int(de_c[c])), L)
                assert [Fraction(float(v)) for v in Q[c]] == fq
                assert [Fraction(float(v)) for v in P[c]] == fp
    # 4 x 1040, L = 2, dt = 2**-8 does not fit: the check is not vacuous
    A, ys, q, p, tau_exp = GB.leapfrog_case(4, 1040, 17, 1)
    assert GB.leapfrog_ints(A, ys, q, p, 0, 8, 2)[2] >= 53


def test_shapes_reach_every_listed_path():
    cases = GB.force_cases()
    for K in GB.K_LIST:
        assert any(k == K and n % 16 and c % 16 for k, n, c in cases)
        assert any(k == K and n % 16 == 0 and c % 16 for k, n, c in cases)
    for K in GB.K_CORE:
        for N in GB.N_GENERAL + GB.N_TRIMMED:
            assert any((k, n) == (K, N) for k, n, c in cases)
        for C in GB.C_LIST:
            assert any((k, c) == (K, C) and n % 16 for k, n, c in cases)
            assert any((k, c) == (K, C) and n % 16 == 0 for k, n, c in cases)
        assert any((k, n) == (K, 272) and c >= 4096 for k, n, c in cases)
    for C in (1, 3, 5, 17, 4113):
        chains = GB.sample_chains(C, C)
        assert len(chains) >= min(C, 4) and all(0 <= c < C for c in chains)
