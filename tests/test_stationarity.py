"""The power table of the exact stationarity tests, on the CPU: for every setting that
``tests/test_gpu_stationarity.py`` uses (``stationarity.ROUTES``: shape, step, trajectory
length, number of transitions, statistics, level) the host sampler of ``tests/stationarity.py``
from exact draws, on fixed seeds,

* is accepted by every statistic when it is correct,
* is rejected when it carries a mutant that applies to the route -- ``always_accept``,
  ``flipped_sign`` (of Delta E in the accept test), ``no_kinetic_energy`` (in the accept test),
  ``swap_always`` (the ladder), ``gamma_shape_plus_one`` (the Gibbs loop) --
* and each mutant's pooled chi^2 |z| is at least twice the threshold's z: the room for device
  draws that differ from numpy's.

One exception to the last point, by construction: ``gamma_shape_plus_one`` leaves theta | tau
exactly invariant, so the whitened theta's chi^2 cannot see it; its margin is asserted on the
statistic built for it, the mean normal score of F(tau) (a N(0, 1 / C) law, z in the same units).

Routes with the same settings share a row (the device routes differ in the kernel they select,
which the host sampler does not have).  Then the pieces: the quadrature CDF of the Gibbs
target against the Gamma law it collapses to without coefficients, its inverse, and the derived
variance of exp(-Delta) against the host sampler's sample variance."""
import numpy as np
import pytest
from scipy import stats

import stationarity as S


def _signature(name):
    r = S.ROUTES[name]
    skip = ('seed', 'how', 'mode', 'test', 'host_seeds')
    return tuple(sorted((k, repr(v)) for k, v in r.items() if k not in skip)) + (S.alpha_of(name),)


def _rows():
    rows = {}
    for name in sorted(S.ROUTES):
        rows.setdefault(_signature(name), []).append(name)
    return sorted(rows.values())


ROWS = _rows()


def test_every_route_has_a_row():
    assert sorted(n for row in ROWS for n in row) == sorted(S.ROUTES)
    for row in ROWS:
        for name in row[1:]:                      # same level, so one row's verdict holds for all
            assert S.alpha_of(name) == S.alpha_of(row[0])
            assert S.ROUTES[name]['energy'] == S.ROUTES[row[0]]['energy']


def _run(name, seed, mutant):
    res = S.run_host(name, seed, mutant)
    return res, S.evaluate(name, res['x'], res['tau'], res['energies'])


@pytest.mark.parametrize('row', ROWS, ids=lambda row: row[0])
def test_power_table(row):
    name = row[0]
    r = S.ROUTES[name]
    print('row %s (also: %s), level per statistic %.3g' % (name, ', '.join(row[1:]) or '-', S.alpha_of(name)))
    for seed in S.HOST_SEEDS[:r['host_seeds']]:
        res, checks = _run(name, seed, None)
        print('seed %d correct: acceptance %.3f' % (seed, res['acceptance']))
        for c in checks:
            print('    ' + S.describe(c))
        assert S.ACCEPT_WINDOW[0] < res['acceptance'] < S.ACCEPT_WINDOW[1]
        assert all(S.inside(c) for c in checks), 'the correct sampler is rejected'
        for mutant in r['mutants']:
            res, checks = _run(name, seed, mutant)
            if mutant == 'gamma_shape_plus_one':
                m = max(abs(c['z']) / c['z_threshold'] for c in checks if c['name'].startswith('mean normal score'))
            else:
                m = S.chi2_margin(checks)
            print('seed %d %-22s rejected by %d of %d statistics, |z| / threshold %.2f'
                  % (seed, mutant, sum(not S.inside(c) for c in checks), len(checks), m))
            assert any(not S.inside(c) for c in checks), '%s is accepted' % mutant
            assert m >= S.MARGIN, (mutant, m)


# ---------------------------------------------------------------------------
# the Gibbs target's quadrature
# ---------------------------------------------------------------------------
def test_quadrature_cdf_without_coefficients_is_the_gamma_law():
    """K = 0 (no coefficients, so no prior on them either): f(tau) ~ tau^(s-1) exp(-(b + |y|^2 / 2) tau)."""
    rs = np.random.RandomState(3)
    y = rs.standard_normal(24) * 0.7
    s, b = 13.0, 2.0
    t = S.GibbsJoint(np.zeros((0, 24)), y, 5.0, s, b)
    law = stats.gamma(s, scale=1.0 / (b + 0.5 * y.dot(y)))
    tau = law.ppf(np.linspace(1e-6, 1.0 - 1e-6, 501))
    err = np.abs(t.cdf(tau) - law.cdf(tau)).max()
    print('largest |F - Gamma cdf| %.3g' % err)
    assert err < 1e-13
    assert np.abs(t.ppf(law.cdf(tau)) / tau - 1.0).max() < 1e-9       # (limited by scipy's cdf at the ends)
    assert np.abs(t.pdf(tau) / law.pdf(tau) - 1.0).max() < 1e-12


def test_quadrature_cdf_agrees_with_one_mpmath_integral_and_inverts():
    t = S.target_of('gibbs_poly_hmc')
    tau = t.ppf(np.array([1e-9, 1e-4, 0.03, 0.5, 0.97, 1.0 - 1e-6]))
    for x, F in zip(tau, t.cdf(tau)):
        assert abs(F - t.cdf_mp(float(x))) < 1e-14, x
    u = np.random.RandomState(4).uniform(size=2000)
    x = t.ppf(u)
    assert np.abs(t.cdf(x) - u).max() < 1e-13
    assert np.all(np.diff(t.F) >= 0.0) and t.F[0] == 0.0 and abs(t.F[-1] + t.tail - 1.0) < 1e-15


@pytest.mark.parametrize('name', ['gibbs_poly_hmc', 'gibbs_linear_hmc'])
def test_inverse_cdf_draws_pass_their_own_tests(name):
    """The exact start of the Gibbs routes, as the device test builds it."""
    theta, tau = S.start_of(name)
    checks = S.evaluate(name, theta, tau)
    for c in checks:
        print(S.describe(c))
    assert all(S.inside(c) for c in checks)
    # the conjugate conditional the loop draws from, at the start: tau (chi^2 / 2 + b) ~ Gamma(s)
    t, r = S.target_of(name), S.ROUTES[name]
    g = tau * (0.5 * t.chi2(theta) + r['prior_shape'])
    _, y, A = S.design_of(name)
    assert np.allclose(t.chi2(theta), np.sum((theta.dot(A) - y) ** 2, axis=1), rtol=1e-10)
    c = S.dkw(g, stats.gamma(S.gibbs_shape(r)).cdf, 1e-9)
    print(S.describe(c))
    assert S.inside(c)


# ---------------------------------------------------------------------------
# the derived variance of exp(-Delta)
# ---------------------------------------------------------------------------
def test_energy_moments_are_those_of_the_host_sampler():
    """C = 4096 chains x D = 64 at effective step 0.1, L = 7: the sample variance of exp(-Delta)
    against the derived one.  (C - 1) s^2 / Var is chi^2 with C - 1 degrees of freedom for a normal
    variable; exp(-Delta) is close to one here -- its derived kurtosis is printed and lies within
    0.25 of 3, which widens the interval's true level by less than a tenth of its width."""
    C, D, a, L = 4096, 64, 0.1, 7
    t = S.isotropic(1.0, 0.0)
    steps = np.full(D, a)
    assert abs(S.energy_moment(steps, L, 1.0) - 1.0) < 1e-12          # the identity itself
    var, kurt = S.energy_variance(steps, L), S.energy_kurtosis(steps, L)
    print('derived variance %.6g, kurtosis %.3f' % (var, kurt))
    assert abs(kurt - 3.0) < 0.25
    lo, hi = stats.chi2.ppf(0.5e-6, C - 1), stats.chi2.isf(0.5e-6, C - 1)
    for seed in S.HOST_SEEDS:
        rs = np.random.RandomState(seed)
        x = t.sample(rs, C, D)
        _, _, eb, ea = S.hmc_transition(rs, x, t.potential, t.force, a, L)
        w = np.exp(eb - ea)
        T = (C - 1) * w.var(ddof=1) / var
        print('seed %d: mean %.5f, (C - 1) s^2 / Var = %.1f in [%.1f, %.1f]' % (seed, w.mean(), T, lo, hi))
        assert lo <= T <= hi
        assert abs(w.mean() - 1.0) <= S.z_of(1e-6) * np.sqrt(var / C)


def test_infinite_variance_is_refused():
    with pytest.raises(ValueError):
        S.energy_variance(np.full(8, 1.6), 6)
    assert S.energy_variance(np.full(8, 1.0), 5) > 0.0
