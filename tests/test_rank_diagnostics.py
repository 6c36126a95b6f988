"""CPU tests of the rank layer's host side: the restatement ``tests/rank_diagnostics_ref.py``
against numpy and scipy, the table of normal scores ``binf_amd.diagnostics.rank_z_table``
against 50-digit arithmetic, and the known answers that make the layer worth having (chains
that agree in mean and differ in scale; heavy tails)."""
import mpmath
import numpy as np
import scipy.stats

import diagnostics_ref as DR
import rank_diagnostics_ref as RR
from binf_amd import diagnostics

PROBS = (0.0, 1.0, 1.0 / 3.0, 0.05, 0.5, 0.95, 0.25, 0.975, 0.1, 2.0 / 3.0)


def ztab(S):
    return diagnostics.rank_z_table(S, 'cpu').numpy()


def test_restated_quantiles_equal_numpy_bit_for_bit():
    """200 sizes from 2 to 12800 x ten probabilities (0, 1 and 1/3 among them): the formula
    of the contract is np.quantile(method='linear'), to the last bit."""
    rng = np.random.default_rng(11)
    sizes = [2, 3, 4, 5, 12800] + [int(s) for s in rng.integers(2, 12801, size=195)]
    n = 0
    for S in sizes:
        scale = 10.0 ** rng.integers(-3, 4)
        s = np.sort(rng.standard_normal(S) * scale + rng.standard_normal())
        want = np.quantile(s, PROBS, method='linear')
        for p, w in zip(PROBS, want):
            got = RR.quantile_sorted(s, p)
            assert np.float64(got).tobytes() == np.float64(w).tobytes(), (S, p, got, w)
            n += 1
    assert n == 2000


def test_restated_quantile_of_a_record_with_a_nan_is_nan():
    x = np.random.default_rng(0).standard_normal((6, 2, 2))
    x[3, 1, 0] = np.nan
    q = RR.quantiles(x, (0.5,))
    assert np.isnan(q[0, 0]) and q[0, 1] == np.quantile(x[:, :, 1], 0.5)


def test_restated_sort_order_of_zeros_and_nans():
    v = np.array([0.0, np.nan, -0.0, 1.0, -np.inf, -np.nan, np.inf, -0.0, 0.0, -1.0])
    s = RR.sort_values(v)
    assert np.array_equal(s[:8], [-np.inf, -1.0, -0.0, -0.0, 0.0, 0.0, 1.0, np.inf])
    assert list(np.signbit(s[2:6])) == [True, True, False, False]
    assert np.isnan(s[8:]).all()


def test_restated_doubled_ranks_equal_scipy_on_heavy_ties():
    rng = np.random.default_rng(7)
    for S, hi in ((1, 1), (2, 1), (17, 2), (400, 5), (4096, 3), (5000, 50)):
        v = rng.integers(0, hi, size=S).astype(np.float64)
        if S > 10:
            v[::7] = -0.0                                  # ties with +0.0 by numeric equality
        want = 2.0 * scipy.stats.rankdata(v, method='average')
        got = RR.doubled_ranks(v)
        assert got.dtype == np.int64 and np.array_equal(got.astype(np.float64), want), S
        assert got.min() >= 2 and got.max() <= 2 * S


def test_rank_z_table_is_antisymmetric_to_the_bit():
    for S in (1, 2, 3, 64, 1000, 12801):
        t = ztab(S)
        assert t.shape == (2 * S + 1,) and t.dtype == np.float64
        assert np.isnan(t[0]) and np.isnan(t[1])
        assert t[S + 1] == 0.0 and not np.signbit(t[S + 1])
        k = np.arange(2, 2 * S + 1)
        assert np.array_equal(t[k], -t[2 * S + 2 - k])
        assert np.all(np.diff(t[2:]) > 0.0)
    assert diagnostics.rank_z_table(64, 'cpu') is diagnostics.rank_z_table(64, 'cpu')      # cached


def exact_score(k, S):
    """ndtri((k / 2 - 3 / 8) / (S + 1 / 4)) at 50 digits."""
    p = (mpmath.mpf(k) / 2 - mpmath.mpf(3) / 8) / (mpmath.mpf(S) + mpmath.mpf(1) / 4)
    return mpmath.sqrt(2) * mpmath.erfinv(2 * p - 1)


def test_rank_z_table_is_within_1e_12_of_50_digit_arithmetic():
    """Every entry for S <= 64 and 2000 sampled entries for S = 2**20.  The bar comes from
    need, not from measurement: a rank's own Monte-Carlo error is at least S**-0.5 >= 3e-5."""
    mpmath.mp.dps = 50
    worst = 0.0
    for S in range(1, 65):
        t = ztab(S)
        for k in range(2, 2 * S + 1):
            worst = max(worst, abs(float(mpmath.mpf(float(t[k])) - exact_score(k, S))))
    S = 1 << 20
    t = ztab(S)
    ks = np.unique(np.concatenate([[2, 3, 4, S, S + 1, S + 2, 2 * S - 1, 2 * S],
                                   np.random.default_rng(5).integers(2, 2 * S + 1, size=1992)]))
    big = max(abs(float(mpmath.mpf(float(t[int(k)])) - exact_score(int(k), S))) for k in ks)
    print('worst error of rank_z_table: %.3g (S <= 64), %.3g (S = 2**20)' % (worst, big))
    assert worst <= 1e-12 and big <= 1e-12


def test_folded_rank_rhat_sees_chains_that_differ_in_scale_only():
    """8 chains of 400 normal draws, chains 4..7 scaled by 3: classic split-R^ is below 1.01
    and the folded rank-R^ above 1.10 in every dimension."""
    x = np.random.default_rng(3).standard_normal((400, 8, 4))
    x[:, 4:, :] *= 3.0
    r = RR.rank_summary(x, ztab(400 * 8))
    classic = DR.diagnose(x, 2)['rhat']
    print('classic %s\nbulk %s\nfolded %s' % (classic, r['rhat_bulk'], r['rhat_folded']))
    assert np.all(classic < 1.01)
    assert np.all(r['rhat_folded'] > 1.10) and np.array_equal(r['rhat'], r['rhat_folded'])
    assert np.all(r['ess_tail'] > 0.0) and np.all(np.isfinite(r['ess_bulk']))
    assert np.array_equal(r['quantiles'], np.quantile(x.reshape(-1, 4), (0.05, 0.5, 0.95), axis=0))


def test_rank_rhat_and_bulk_ess_stay_meaningful_for_cauchy_draws():
    x = np.random.default_rng(4).standard_cauchy((400, 8, 1))
    r = RR.rank_summary(x, ztab(400 * 8))
    print('rhat %s ess_bulk %s ess_tail %s' % (r['rhat'], r['ess_bulk'], r['ess_tail']))
    assert np.all(r['rhat'] < 1.01)
    assert np.all(np.isfinite(r['ess_bulk'])) and np.all(r['ess_bulk'] > 0.0)


def test_restated_summary_does_not_depend_on_the_other_dimensions():
    x = DR.ar1(0.5, 21, 3, 4, seed=8)
    whole = RR.rank_summary(x, ztab(20 * 3), max_lag=5)
    for i in range(4):
        one = RR.rank_summary(x[:, :, i:i + 1], ztab(20 * 3), max_lag=5)
        for k in RR.FIELDS:
            assert np.array_equal(one[k].reshape(-1), whole[k][..., i].reshape(-1), equal_nan=True), (i, k)
