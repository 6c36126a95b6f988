"""The host restatement of the free-energy estimator (tests/free_energy_ref.py) against exact
arithmetic, against the closed form of the harmonic ladder on exact iid draws, and on
hand-built records.  No GPU, nothing from the library."""
import numpy as np
import pytest

import free_energy_ref as FE
import stationarity as ST

CHUNK = FE.header_chunk()


def small_problems():
    """(name, u, v): good overlap, poor overlap (the two slots 30 apart in units of their
    width), and samples of weight 0 among finite ones."""
    rs = np.random.RandomState(5)
    good = (rs.standard_normal(40) * 1.5 - 2.0, rs.standard_normal(40) * 1.5 + 1.0)
    poor = (rs.standard_normal(30) * 0.5 - 18.0, rs.standard_normal(30) * 0.5 - 12.0)
    u, v = rs.standard_normal(50) * 2.0 + 0.5, rs.standard_normal(50) * 2.0 - 1.0
    u[::3] = -np.inf
    v[1::4] = -np.inf
    wide = (rs.standard_normal(CHUNK + 37) * 3.0 - 1.0, rs.standard_normal(CHUNK + 37) * 3.0 + 2.5)
    return [('good', ) + good, ('poor', ) + poor, ('minus_inf', u, v), ('two_chunks', ) + wide]


@pytest.mark.parametrize('case', small_problems(), ids=lambda c: c[0])
def test_restated_delta_against_the_exact_root(case):
    """|delta - root| <= e_g / S + 2 ulp(delta), derived, not chosen:

    * an error e_g in evaluating g moves its root by e_g / g' = e_g / S;
    * e_g (``FE.g_error_bound``): every one of the 2 n terms sigma in [0, 1] carries the
      rounding of z (|z| sigma (1 - sigma) <= 0.23 ulp), one exp (1 ulp), one add and one
      divide (half an ulp each) -- under 3 * 2^-52 absolute; each of the two sums of n terms
      <= 1 passes chunk / 256 + 6 + 3 + n_chunks additions, every level rounding partial sums
      that total <= n; the final subtraction rounds a value <= n;
    * the iteration stops when the Newton step is under half an ulp of delta or the bracket is
      two neighbouring doubles: 2 ulp(delta) covers both.
    S comes from mpmath, at the exact root."""
    name, u, v = case
    if name == 'two_chunks':
        u, v = u[:600].copy(), v[:600].copy()       # mpmath's cost; the chunked sums: next test
    got = FE.solve(u, v, CHUNK)
    root = FE.exact_root(u, v)
    S = float(FE.exact_g(u, v, root)[1])
    n = u.shape[0]
    tol = FE.delta_bound(n, S, float(root), CHUNK)
    err = abs(float(FE._mp().mpf(float(got['delta'])) - root))
    print('%s: n %d, S %.3g, delta %.17g, error %.3g, bound %.3g, %d iterations'
          % (name, n, S, got['delta'], err, tol, got['iterations']))
    assert got['status'] == FE.OK and got['n'] == n and got['n_invalid'] == 0
    assert err <= tol
    # S is taken at the root, info at delta: FE.info_bound with delta's error bound
    assert abs(got['info'] - S) <= FE.info_bound(n, S, tol)
    # the exponential averages against exact arithmetic: FE.average_bound
    for key, x, sign in (('delta_forward', u, 1), ('delta_reverse', v, -1)):
        exact = sign * FE.exact_average(x)
        assert abs(float(FE._mp().mpf(float(got[key])) - exact)) <= FE.average_bound(n, float(exact)), key


def test_chunked_sums_against_exact_arithmetic():
    """More than one chunk (n = chunk + 37): the exponential averages within
    ``FE.average_bound`` of mpmath's, and mpmath's g changes sign inside [delta - tol, delta +
    tol], tol = ``FE.delta_bound`` with S from mpmath at delta (the derivation of the test
    above; the root itself is not bisected here, which would cost 170 exact evaluations)."""
    _, u, v = small_problems()[3]
    n = u.shape[0]
    assert CHUNK < n < 2 * CHUNK
    got = FE.solve(u, v, CHUNK)
    mp = FE._mp()
    for key, x, sign in (('delta_forward', u, 1), ('delta_reverse', v, -1)):
        exact = sign * FE.exact_average(x)
        assert abs(float(mp.mpf(float(got[key])) - exact)) <= FE.average_bound(n, float(exact)), key
    d = float(got['delta'])
    S = float(FE.exact_g(u, v, d)[1])
    tol = FE.delta_bound(n, S, d, CHUNK)
    assert FE.exact_g(u, v, mp.mpf(d) - mp.mpf(tol))[0] < 0 < FE.exact_g(u, v, mp.mpf(d) + mp.mpf(tol))[0]
    assert abs(got['info'] - S) <= FE.info_bound(n, S, 0.0)


def test_edge_contract_of_the_restatement():
    z = np.zeros(10)
    same = FE.solve(z, z, CHUNK)
    assert same['delta'] == 0.0 and same['delta_forward'] == 0.0 and same['delta_reverse'] == 0.0
    assert same['info'] == 20 * 0.25 and same['status'] == FE.OK
    ninf = np.full(10, -np.inf)
    one = FE.solve(ninf, z, CHUNK)
    assert one['delta_forward'] == -np.inf and one['delta_reverse'] == 0.0
    assert one['delta'] == -np.inf and one['status'] == FE.ONE_SIDED
    other = FE.solve(z, ninf, CHUNK)
    assert other['delta_reverse'] == np.inf and other['delta'] == np.inf and other['status'] == FE.ONE_SIDED
    none = FE.solve(ninf, ninf, CHUNK)
    assert none['delta_forward'] == -np.inf and none['delta_reverse'] == np.inf
    assert np.isnan(none['delta']) and none['status'] == FE.NO_FINITE
    bad = z.copy()
    bad[3], bad[7] = np.nan, np.inf
    inv = FE.solve(bad, z, CHUNK)
    assert inv['n_invalid'] == 2 and inv['status'] == FE.INVALID
    assert all(np.isnan(inv[k]) for k in ('delta', 'delta_forward', 'delta_reverse', 'info'))
    # both sides 2000 from the iterate: every sigma underflows, g is flat 0, no root determined
    far = FE.solve(z - 2000.0, z - 2000.0, CHUNK)
    assert far['status'] == FE.NO_OVERLAP and far['info'] == 0.0 and far['delta'] == 0.0
    assert abs(far['delta_forward'] + 2000.0) <= FE.average_bound(10, 2000.0)
    assert far['delta_reverse'] == -far['delta_forward']
    empty = FE.solve(np.zeros(0), np.zeros(0), CHUNK)
    assert empty['status'] == FE.EMPTY and empty['n'] == 0 and np.isnan(empty['delta'])


def test_rows_by_parity_and_groups_by_ladder_on_hand_built_records():
    R, n_ladders, T = 4, 4, 5
    C = R * n_ladders
    rec = np.arange(T)[:, None] * 100.0 + np.arange(C)[None, :]        # w[t, c] = 100 t + c
    # first_round 0: pair 0 and 2 live in rows 0, 2, 4; pair 1 in rows 1, 3
    u, v = FE.problem_samples(rec, R, 0, 1, 0, 0)
    assert u.tolist() == [100.0 * t + 4 * l for t in (0, 2, 4) for l in range(4)]
    assert v.tolist() == [100.0 * t + 4 * l + 1 for t in (0, 2, 4) for l in range(4)]
    u, v = FE.problem_samples(rec, R, 0, 1, 0, 1)
    assert u.tolist() == [100.0 * t + 4 * l + 1 for t in (1, 3) for l in range(4)]
    assert v.tolist() == [100.0 * t + 4 * l + 2 for t in (1, 3) for l in range(4)]
    # first_round 1 turns the rows round
    u, _ = FE.problem_samples(rec, R, 1, 1, 0, 0)
    assert u.tolist() == [100.0 * t + 4 * l for t in (1, 3) for l in range(4)]
    u, _ = FE.problem_samples(rec, R, 7, 1, 0, 1)
    assert u.tolist() == [100.0 * t + 4 * l + 1 for t in (0, 2, 4) for l in range(4)]
    # two groups: ladders 0, 1 and ladders 2, 3
    u, v = FE.problem_samples(rec, R, 0, 2, 1, 2)
    assert u.tolist() == [100.0 * t + 4 * l + 2 for t in (0, 2, 4) for l in (2, 3)]
    assert v.tolist() == [100.0 * t + 4 * l + 3 for t in (0, 2, 4) for l in (2, 3)]
    # the groups of a pair partition its pooled samples
    pooled = sorted(FE.problem_samples(rec, R, 0, 1, 0, 1)[0].tolist())
    parts = [FE.problem_samples(rec, R, 0, 4, g, 1)[0].tolist() for g in range(4)]
    assert sorted(sum(parts, [])) == pooled and all(len(p) == 2 for p in parts)
    res = FE.bar(rec[:1], R, 0, 2)
    assert res['n'].tolist() == [[2, 0, 2], [2, 0, 2]]
    assert res['status'][:, 1].tolist() == [FE.EMPTY, FE.EMPTY]


@pytest.mark.parametrize('R', [1, 2, 3, 4, 5])
def test_work_row_pairs_and_nans(R):
    rs = np.random.RandomState(R)
    C = 3 * R
    lp_own, lp_sw = rs.standard_normal(C), rs.standard_normal(C)
    for parity in (0, 1):
        w = FE.work_row(lp_own, lp_sw, R, parity)
        for c in range(C):
            r = c % R
            low = r >= parity and (r - parity) % 2 == 0 and r + 1 < R
            up = r - 1 >= parity and (r - 1 - parity) % 2 == 0
            if low:
                assert w[c] == lp_sw[c] - lp_own[c + 1]
            elif up:
                assert w[c] == lp_sw[c] - lp_own[c - 1]
            else:
                assert np.isnan(w[c])
        # a pair is active exactly in the rounds whose parity is r & 1
        p = FE.partner_or_minus_one(C, R, parity)
        active = [r for r in range(R - 1) if p[r] == r + 1]
        assert active == [r for r in range(R - 1) if (r & 1) == parity]


def test_iid_harmonic_ladder_recovers_the_closed_form():
    """Exact independent draws x = z / sqrt(k_r): delta must lie within z(ST.ALPHA / pairs) iid
    standard errors sqrt(1 / S - 2 / n) of (D / 2) ln(k_{r+1} / k_r), the level of the
    stationarity tests, Bonferroni over the pairs."""
    R = len(FE.HARMONIC_K)
    rec = FE.harmonic_iid_record(400, 16, seed=11)
    res = FE.bar(rec, R, 0, 1)
    exact = FE.harmonic_exact()
    zmax = ST.z_of(ST.ALPHA / (R - 1))
    for r in range(R - 1):
        n, S = res['n'][0, r], res['info'][0, r]
        se = np.sqrt(1.0 / S - 2.0 / n)
        z = (res['delta'][0, r] - exact[r]) / se
        print('pair %d: n %d, delta %.5f (exact %.5f), iid stderr %.4f, z %+.2f, forward %.4f, reverse %.4f, '
              'overlap %.3f' % (r, n, res['delta'][0, r], exact[r], se, z, res['delta_forward'][0, r],
                                res['delta_reverse'][0, r], S / n))
        assert n == 200 * 16 and res['status'][0, r] == FE.OK
        assert abs(z) <= zmax


def test_iid_draws_pass_the_end_to_end_gate_with_factor_one():
    """The gate of the GPU end-to-end test, on exact iid draws, autocorrelation factor 1: every
    delta and the total within 6 group-spread standard errors of the closed form, and the
    group-spread standard errors under 1 * 2 * the iid standard error (2: the spread of 32
    groups is itself known to 13 % only)."""
    y = FE.harmonic_yardstick()
    exact = FE.harmonic_exact()
    assert np.all(np.abs(y['delta'] - exact) <= FE.E2E_SIGMAS * y['stderr'])
    assert abs(y['delta'].sum() - exact.sum()) <= FE.E2E_SIGMAS * y['total_stderr']
    print('stderr / iid stderr', y['stderr'] / y['iid_stderr'], y['total_stderr'] / y['iid_total_stderr'])
    assert np.all(y['stderr'] <= 2.0 * y['iid_stderr'])
    assert y['total_stderr'] <= 2.0 * y['iid_total_stderr']
