"""Host helpers of the exact stationarity tests (``tests/test_stationarity.py`` on the CPU,
``tests/test_gpu_stationarity.py`` on the device).  numpy, scipy.stats and mpmath only:
nothing here calls into the library.

The design.  Chains are independent.  If they START as exact draws of the target and the
transition leaves the target invariant, the C states at any later time are again i.i.d.
exact draws: every statistic below has a known null law, there is no autocorrelation to
estimate and no tolerance is taken from the code under test.

    pooled_chi2      sum of the squared standardised entries: chi^2 with (number of entries)
                     degrees of freedom, two-sided interval from ``scipy.stats.chi2``
    pooled_mean      mean of the standardised entries: N(0, 1/n)
    dkw              sup |F_n - F| against ``sqrt(log(2 / alpha) / (2 n))``, the
                     Dvoretzky-Kiefer-Wolfowitz bound (Massart's constant), valid for every n
    energy_identity  mean of exp(E_before - E_after) = 1; its variance is derived from the
                     leapfrog map (``energy_moment``), its threshold a normal quantile (CLT)

Levels.  Every test function has a total false-alarm level ``ALPHA = 1e-9``, split evenly
(Bonferroni) over its parametrisations and their statistics; the energy identity rests on a
CLT and gets ``ALPHA_ENERGY = 1e-6`` of its own, split the same way.  Seeds are fixed and
written into ``ROUTES`` / ``HOST_SEEDS`` below: a failure at these levels is a finding.

``ROUTES`` is THE table of settings: the device tests read their shapes, steps, trajectory
lengths, numbers of transitions and seeds from it and the CPU power table runs the host
sampler at exactly those settings, correct and with every applicable mutant, so a device
test cannot drift to a setting whose power was never shown.

The Gibbs target.  ``GammaSampler`` draws the precision with shape ``0.5 n + prior.shape - 1``
(reference ``binf/example/samplers.py:27-32``, restated in ``oracle/ref_numpy.py:296-299``
``gamma_shape``: "one less than the textbook value") and rate ``0.5 chi^2 + prior.rate`` where
the prior is the CONDITIONAL posterior's copy, whose rate equals its shape (quirk Q6,
``binf_amd/example/priors.py:36-43``).  The sweep is therefore exactly invariant for

    pi(theta, tau)  ~  tau^(s - 1) exp(-tau (chi^2(theta) / 2 + b)) N(theta; 0, diag(v)),
    s = 0.5 n + prior.shape - 1,   b = prior.shape

-- the posterior under a Gamma prior of shape ``prior.shape - 1`` (not ``prior.shape``) and
rate ``prior.shape``.  ``GibbsJoint`` is parametrised by (s, b) directly; the tests choose
``prior.shape = 2 > 1`` so that this prior is proper.  theta integrates out analytically;
the marginal of tau is integrated with ``mpmath.quad`` at 40 digits.
"""
import numpy as np
import mpmath
from scipy import stats

f64 = np.float64
ALPHA = 1e-9
ALPHA_ENERGY = 1e-6
MARGIN = 2.0                       # a mutant's pooled-chi^2 |z| over the threshold's z (CPU power table)
ACCEPT_WINDOW = (0.6, 0.8)

HMC_MUTANTS = ('always_accept', 'flipped_sign', 'no_kinetic_energy')


# ---------------------------------------------------------------------------
# statistics: each returns a dict(name, value, lo, hi, [z, z_threshold])
# ---------------------------------------------------------------------------
def z_of(alpha):
    """The two-sided normal quantile of level ``alpha``."""
    return float(stats.norm.isf(0.5 * alpha))


def pooled_chi2(z, alpha, name='pooled chi2'):
    z = np.asarray(z, dtype=f64).reshape(-1)
    df = z.size
    T = float(np.sum(z * z))
    lo, hi = float(stats.chi2.ppf(0.5 * alpha, df)), float(stats.chi2.isf(0.5 * alpha, df))
    return dict(name=name, kind='chi2', value=T, lo=lo, hi=hi, df=df,
                z=(T - df) / np.sqrt(2.0 * df), z_threshold=z_of(alpha))


def pooled_mean(z, alpha, name='pooled mean'):
    z = np.asarray(z, dtype=f64).reshape(-1)
    t = z_of(alpha) / np.sqrt(z.size)
    m = float(z.mean())
    return dict(name=name, kind='mean', value=m, lo=-t, hi=t, z=m * np.sqrt(z.size), z_threshold=z_of(alpha))


def dkw_threshold(n, alpha):
    return float(np.sqrt(np.log(2.0 / alpha) / (2.0 * n)))


def dkw(z, cdf, alpha, name='DKW'):
    """sup |F_n - F| of the sample ``z`` against the continuous CDF ``cdf``."""
    z = np.sort(np.asarray(z, dtype=f64).reshape(-1))
    n = z.size
    F = cdf(z)
    i = np.arange(1, n + 1, dtype=f64)
    d = float(max(np.max(i / n - F), np.max(F - (i - 1.0) / n)))
    return dict(name=name, kind='dkw', value=d, lo=0.0, hi=dkw_threshold(n, alpha))


def unit_interval(u, alpha, name='DKW uniform'):
    return dkw(u, lambda x: np.clip(x, 0.0, 1.0), alpha, name)


def inside(check):
    return bool(check['lo'] <= check['value'] <= check['hi'])


def describe(check):
    z = '' if 'z' not in check else ', z %+.2f (threshold %.2f)' % (check['z'], check['z_threshold'])
    return '%-28s %.6g in [%.6g, %.6g]%s%s' % (check['name'], check['value'], check['lo'], check['hi'], z,
                                               '' if inside(check) else '   <-- OUTSIDE')


# ---------------------------------------------------------------------------
# the energy identity: moments of exp(-s Delta) from the leapfrog map
# ---------------------------------------------------------------------------
def leapfrog_map(a, L):
    """(q, r) -> (q', r') of L leapfrog steps of size ``a`` on the unit oscillator
    (U = q^2 / 2, K = r^2 / 2): half kick, L - 1 x [drift, kick], drift, half kick."""
    half = np.array([[1.0, 0.0], [-0.5 * a, 1.0]])
    drift = np.array([[1.0, a], [0.0, 1.0]])
    step = half.dot(drift).dot(half)
    return np.linalg.matrix_power(step, int(L))


def energy_moment(steps, L, s):
    """E[exp(-s Delta)] in stationarity for a product of unit oscillators integrated with the
    per-dimension effective steps ``steps`` (``dt sqrt(k)``; with a metric ``dt scale_i /
    sigma_i``): Delta = 1/2 z'(M'M - I) z per dimension, z ~ N(0, I_2), so the moment is
    prod_i det(I + s (M_i'M_i - I))^(-1/2).  Refuses (ValueError) where a factor is not
    positive definite: the moment is infinite there."""
    out = 1.0
    for a in np.asarray(steps, dtype=f64).reshape(-1):
        M = leapfrog_map(a, L)
        B = np.eye(2) + s * (M.T.dot(M) - np.eye(2))
        if np.min(np.linalg.eigvalsh(B)) <= 0.0:
            raise ValueError('energy_moment: I + %g (M\'M - I) is not positive definite at step %g, L = %d: '
                             'the moment is infinite' % (s, a, L))
        out *= np.linalg.det(B) ** -0.5
    return float(out)


def energy_variance(steps, L):
    """Var exp(-Delta) = E exp(-2 Delta) - 1; ``steps`` is ``[D]`` or ``[G x D]`` (one row per
    group of chains: the average over the groups is the variance of a chain drawn from
    equally large groups)."""
    steps = np.atleast_2d(np.asarray(steps, dtype=f64))
    return float(np.mean([energy_moment(row, L, 2.0) - 1.0 for row in steps]))


def energy_kurtosis(steps, L):
    """E (X - 1)^4 / Var^2 of X = exp(-Delta), one group."""
    m1, m2, m3, m4 = (energy_moment(steps, L, s) for s in (1.0, 2.0, 3.0, 4.0))
    var = m2 - 1.0
    return float((m4 - 4.0 * m3 + 6.0 * m2 - 4.0 * m1 + 1.0) / (var * var))


def energy_identity(e_before, e_after, steps, L, alpha, name='energy identity'):
    """mean exp(E_before - E_after) over n independent transitions against 1 +- a normal
    quantile of sqrt(Var / n), Var derived (``energy_variance``)."""
    d = np.asarray(e_before, dtype=f64).reshape(-1) - np.asarray(e_after, dtype=f64).reshape(-1)
    m = float(np.mean(np.exp(d)))
    t = z_of(alpha) * np.sqrt(energy_variance(steps, L) / d.size)
    return dict(name=name, kind='energy', value=m, lo=1.0 - t, hi=1.0 + t,
                z=(m - 1.0) / t * z_of(alpha), z_threshold=z_of(alpha))


# ---------------------------------------------------------------------------
# exact targets: sampler, standardiser, potential and the force the sampler integrates
# ---------------------------------------------------------------------------
class GaussTarget(object):
    """N(mu, sd^2) per entry: ``mu`` scalar, ``sd`` scalar, ``[D]`` or ``[C x D]``."""

    def __init__(self, mu, sd):
        self.mu, self.sd = f64(mu), np.asarray(sd, dtype=f64)
        self.w = 1.0 / (self.sd * self.sd)

    def sample(self, rs, C, D):
        return self.mu + self.sd * rs.standard_normal((C, D))

    def standardise(self, x):
        return (np.asarray(x, dtype=f64) - self.mu) / self.sd

    def potential(self, x):
        z = (x - self.mu) / self.sd
        return 0.5 * np.sum(z * z, axis=1)

    def force(self, x):
        g = x - self.mu
        g *= self.w
        return g


def isotropic(k, x0):
    return GaussTarget(x0, 1.0 / np.sqrt(k))


SIGMA8 = 100.0 ** (np.arange(8) / 7.0)            # tests/metric_ref.SIGMA8: 1 ... 100


def metric_rows(sigma, G, seed=41):
    """The MISMATCHED metric of the metric routes: row g is sigma times fixed factors in
    [0.5, 2], a different set per row (invariance must hold for any positive scale)."""
    rs = np.random.RandomState(seed)
    return sigma[None, :] * 2.0 ** rs.uniform(-1.0, 1.0, size=(G, sigma.size))


LADDER_K = (1.0, 0.5, 0.25, 0.125)


def ladder(n_ladders, ks=LADDER_K):
    """Chain c = ladder * R + r is N(0, 1 / k_r): ``[C x 1]`` standard deviations."""
    k = np.tile(np.asarray(ks, dtype=f64), n_ladders)
    return GaussTarget(0.0, 1.0 / np.sqrt(k)[:, None]), k


class LinearConditional(object):
    """p(theta | tau, data) of ``mock = theta . A`` with Gaussian errors of precision tau and
    the prior N(0, diag(prior_var)): Gaussian with precision matrix
    P = tau A A' + diag(1 / prior_var), mean P^-1 tau A y.  Whitened with the Cholesky factor
    of P (z = L'(theta - mean), P = L L').  The potential has the prior, the force the sampler
    integrates does not (quirk Q4); the target is the full conditional all the same."""

    def __init__(self, A, y, tau, prior_var):
        self.A, self.y, self.tau = np.asarray(A, dtype=f64), np.asarray(y, dtype=f64), f64(tau)
        K = self.A.shape[0]
        self.var = np.broadcast_to(np.asarray(prior_var, dtype=f64), (K,)).copy()
        self.P = self.tau * self.A.dot(self.A.T) + np.diag(1.0 / self.var)
        self.L = np.linalg.cholesky(self.P)
        self.mean = np.linalg.solve(self.P, self.tau * self.A.dot(self.y))

    def sample(self, rs, C, D=None):
        z = rs.standard_normal((C, self.A.shape[0]))
        return self.mean + np.linalg.solve(self.L.T, z.T).T

    def standardise(self, x):
        return (np.asarray(x, dtype=f64) - self.mean).dot(self.L)

    def potential(self, x):
        r = x.dot(self.A) - self.y
        return 0.5 * self.tau * np.sum(r * r, axis=1) + 0.5 * np.sum(x * x / self.var, axis=1)

    def force(self, x):
        return self.tau * (x.dot(self.A) - self.y).dot(self.A.T)


def polynomial_case(K, N, tau=2.5, seed=5):
    """The example's data: a polynomial on [-1, 1] plus noise; (xs, ys, Vandermonde A [K x N])."""
    rs = np.random.RandomState(seed)
    xs = np.linspace(-1.0, 1.0, N)
    truth = np.array([2.0, -4.0, 1.0, 1.5, -0.5, 0.25])[:K]
    A = np.vstack([xs ** i for i in range(K)])
    return xs, truth.dot(A) + rs.standard_normal(N) / np.sqrt(tau), A


def dense_case(K, N, tau=2.5, seed=6):
    """A dense design matrix (not Vandermonde) for the linear kinds; (ys, A [K x N])."""
    rs = np.random.RandomState(seed)
    A = rs.standard_normal((K, N))
    truth = rs.standard_normal(K)
    return truth.dot(A) + rs.standard_normal(N) / np.sqrt(tau), A


class GibbsJoint(object):
    """pi(theta, tau) ~ tau^(s-1) exp(-tau (|y - theta.A|^2 / 2 + b)) N(theta; 0, diag(v)) (see
    the module docstring for s and b).  With B = diag(sqrt v) A, the eigen-decomposition
    B B' = U diag(lam) U' and w = U' B y,

        theta | tau  =  diag(sqrt v) U [ tau w / (tau lam + 1) + z / sqrt(tau lam + 1) ]
        log f(tau)   =  (s - 1) log tau - b tau - 1/2 sum log(tau lam_i + 1)
                        - tau / 2 (rss + sum w_i^2 / (lam_i (tau lam_i + 1)))

    with rss = |y|^2 - sum w_i^2 / lam_i >= 0 the residual sum of squares (the subtraction of
    the two large terms of the completed square is done once, analytically).  K = 0 (an
    empty design matrix) leaves the Gamma law Gamma(s, b + |y|^2 / 2).

    The CDF: ``mpmath.quad`` at 40 digits over the cells of a grid of ``nodes`` points from 0
    to far in the upper tail (``F[j]``, cumulative, normalised by their total); inside a cell
    a 24-point Gauss-Legendre rule in float64 on the (smooth) density, whose agreement with the
    mpmath value to 1e-14 the CPU tests check.  Inverse: bracketing by the cells, then
    bisection on tau to 1e-14 relative."""

    def __init__(self, A, y, prior_var, s, b, nodes=100, dps=40):
        A, y = np.asarray(A, dtype=f64), np.asarray(y, dtype=f64)
        K = A.shape[0]
        self.K, self.s, self.b = K, f64(s), f64(b)
        self.sv = np.sqrt(np.broadcast_to(np.asarray(prior_var, dtype=f64), (K,)))
        B = self.sv[:, None] * A
        if K:
            self.lam, self.U = np.linalg.eigh(B.dot(B.T))
            self.w = self.U.T.dot(B.dot(y))
        else:
            self.lam, self.U, self.w = np.zeros(0), np.zeros((0, 0)), np.zeros(0)
        assert np.all(self.lam > 0.0)
        self.rss = float(y.dot(y) - np.sum(self.w * self.w / self.lam))
        assert self.rss >= 0.0
        self._tabulate(nodes, dps)

    # -- the marginal of tau -------------------------------------------------------------
    def log_f(self, tau):
        tau = np.asarray(tau, dtype=f64)[..., None]
        t = tau * self.lam + 1.0
        quad = self.rss + np.sum(self.w * self.w / (self.lam * t), axis=-1)
        return (self.s - 1.0) * np.log(tau[..., 0]) - self.b * tau[..., 0] - 0.5 * np.sum(np.log(t), axis=-1) \
            - 0.5 * tau[..., 0] * quad

    def _mp_f(self, shift):
        lam, w = [mpmath.mpf(float(v)) for v in self.lam], [mpmath.mpf(float(v)) for v in self.w]
        s, b, rss = mpmath.mpf(float(self.s)), mpmath.mpf(float(self.b)), mpmath.mpf(self.rss)

        def f(tau):
            if tau == 0:
                return mpmath.mpf(0)
            t = [tau * l + 1 for l in lam]
            quad = rss + sum(wi * wi / (l * ti) for wi, l, ti in zip(w, lam, t))
            return mpmath.exp((s - 1) * mpmath.log(tau) - b * tau - sum(mpmath.log(ti) for ti in t) / 2
                              - tau * quad / 2 - shift)
        return f

    def _tabulate(self, nodes, dps):
        # mode and curvature of log f in float64: the grid spans mode +- 40 "standard deviations"
        # (at least [0, 3 mode]), which leaves less than 1e-40 of the mass outside
        grid = np.exp(np.linspace(np.log(1e-8), np.log(1e8), 200001))
        lf = self.log_f(grid)
        j = int(np.argmax(lf))
        mode, top = grid[j], lf[j]
        within = grid[lf > top - 0.5]
        sd = 0.5 * (within[-1] - within[0])
        hi = max(3.0 * mode, mode + 40.0 * sd)
        self.shift = float(top)
        self.t = np.linspace(0.0, hi, int(nodes) + 1)
        with mpmath.workdps(dps):
            f = self._mp_f(mpmath.mpf(self.shift))
            cells = [mpmath.quad(f, [mpmath.mpf(float(a)), mpmath.mpf(float(c))])
                     for a, c in zip(self.t[:-1], self.t[1:])]
            tail = mpmath.quad(f, [mpmath.mpf(float(hi)), mpmath.inf])
            total = sum(cells) + tail
            self.tail = float(tail / total)
            cum, acc = [mpmath.mpf(0)], mpmath.mpf(0)
            for c in cells:
                acc += c
                cum.append(acc)
            self.F = np.array([float(c / total) for c in cum])
            self.log_norm = float(mpmath.log(total)) + self.shift
            self._total, self._dps = total, dps
        assert self.tail < 1e-30
        self._gx, self._gw = np.polynomial.legendre.leggauss(24)

    def pdf(self, tau):
        return np.exp(self.log_f(tau) - self.log_norm)

    def cdf(self, tau):
        tau = np.asarray(tau, dtype=f64)
        flat = np.clip(tau.reshape(-1), 0.0, self.t[-1])
        j = np.clip(np.searchsorted(self.t, flat, side='right') - 1, 0, self.t.size - 2)
        a = self.t[j]
        half = 0.5 * (flat - a)
        x = a[:, None] + half[:, None] * (self._gx[None, :] + 1.0)
        with np.errstate(divide='ignore'):
            inc = half * np.sum(self._gw[None, :] * self.pdf(x), axis=1)
        return np.minimum(self.F[j] + inc, 1.0).reshape(tau.shape)

    def cdf_mp(self, tau):
        """F(tau) by one mpmath quadrature from 0 (the check of ``cdf``)."""
        with mpmath.workdps(self._dps):
            f = self._mp_f(mpmath.mpf(self.shift))
            cuts = [mpmath.mpf(0)] + [mpmath.mpf(float(v)) for v in self.t[1:-1:25] if v < tau] + [mpmath.mpf(float(tau))]
            return float(mpmath.quad(f, cuts) / self._total)

    def ppf(self, u):
        u = np.asarray(u, dtype=f64).reshape(-1)
        j = np.clip(np.searchsorted(self.F, u, side='right') - 1, 0, self.t.size - 2)
        lo, hi = self.t[j].copy(), self.t[j + 1].copy()
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            below = self.cdf(mid) < u
            lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
            if np.all(hi - lo <= 1e-14 * hi):
                break
        return 0.5 * (lo + hi)

    # -- theta | tau ----------------------------------------------------------------------
    def sample(self, rs, C, D=None):
        """(theta [C x K], tau [C]): tau = F^-1(u), then theta | tau."""
        tau = self.ppf(rs.uniform(size=C))
        t = tau[:, None] * self.lam + 1.0
        e = tau[:, None] * self.w / t + rs.standard_normal((C, self.K)) / np.sqrt(t)
        return e.dot(self.U.T) * self.sv, tau

    def standardise(self, theta, tau):
        """The whitened theta | tau: N(0, I_K) per chain."""
        tau = np.asarray(tau, dtype=f64)
        t = tau[:, None] * self.lam + 1.0
        e = (np.asarray(theta, dtype=f64) / self.sv).dot(self.U)
        return np.sqrt(t) * e - tau[:, None] * self.w / np.sqrt(t)

    def chi2(self, theta):
        """|y - theta.A|^2 per chain, through the eigenbasis: rss + sum lam_i (e_i - w_i / lam_i)^2."""
        e = (np.asarray(theta, dtype=f64) / self.sv).dot(self.U)
        return self.rss + np.sum(self.lam * (e - self.w / self.lam) ** 2, axis=1)


# ---------------------------------------------------------------------------
# the host sampler (vectorised numpy), with mutants.  The mutants live here alone.
# ---------------------------------------------------------------------------
def _accept(rs, C, e_before, e_after, k_before, k_after, mutant):
    """The Metropolis test of an HMC transition; ``e_*`` potential, ``k_*`` kinetic energies."""
    u = rs.uniform(size=C)
    if mutant == 'no_kinetic_energy':
        d = e_after - e_before
    else:
        d = (e_after + k_after) - (e_before + k_before)
    if mutant == 'flipped_sign':
        d = -d
    with np.errstate(over='ignore'):
        acc = u < np.exp(np.minimum(0.0, -d))
    if mutant == 'always_accept':
        acc = np.ones(C, dtype=bool)
    return acc


def hmc_transition(rs, x, potential, force, dt, L, scale=None, mutant=None):
    """One transition of every chain.  ``dt`` a number or ``[C]``, ``scale`` None or
    ``[C x D]`` / ``[D]`` (the diagonal metric's scale per entry).  Returns
    (new state, accepted, E_before, E_after) with the TRUE total energies."""
    C = x.shape[0]
    r = rs.standard_normal(x.shape)
    h = np.asarray(dt, dtype=f64).reshape(-1, 1) if np.ndim(dt) else f64(dt)
    if scale is not None:
        h = h * scale
    def kick(p, q, half):                      # p -= (h or h / 2) * force(q), without temporaries
        g = force(q)
        g *= 0.5 * h if half else h
        p -= g

    q, p = x.copy(), r.copy()
    kick(p, q, True)
    for _ in range(int(L) - 1):
        q += h * p
        kick(p, q, False)
    q += h * p
    kick(p, q, True)
    u0, u1 = potential(x), potential(q)
    k0, k1 = 0.5 * np.sum(r * r, axis=1), 0.5 * np.sum(p * p, axis=1)
    acc = _accept(rs, C, u0, u1, k0, k1, mutant)
    return np.where(acc[:, None], q, x), acc, u0 + k0, u1 + k1


def swap_round(rs, x, k, R, parity, mutant=None):
    """One swap round of the tempered ladder log p_c(x) = -k_c |x|^2 / 2: slot r is the lower
    member of (r, r + 1) iff r >= parity, r - parity even, r + 1 < R; accept iff
    u < exp((lp_sw[i] + lp_sw[j]) - (lp_own[i] + lp_own[j]))."""
    C = x.shape[0]
    r = np.arange(C) % R
    low = np.nonzero((r >= parity) & ((r - parity) % 2 == 0) & (r + 1 < R))[0]
    n2 = np.sum(x * x, axis=1)
    delta = -0.5 * (k[low] - k[low + 1]) * (n2[low + 1] - n2[low])
    u = rs.uniform(size=C)[low]
    with np.errstate(over='ignore'):
        acc = u < np.exp(np.minimum(delta, 700.0))
    if mutant == 'swap_always':
        acc[:] = True
    i = low[acc]
    out = x.copy()
    out[i], out[i + 1] = x[i + 1], x[i]
    return out, acc


# ---------------------------------------------------------------------------
# THE table of settings
# ---------------------------------------------------------------------------
def _gauss(test, C, D, dt, L, n, seed, how, **kw):
    d = dict(kind='gauss', test=test, C=C, D=D, dt=dt, L=L, n=n, seed=seed, how=how, k=2.5, x0=0.3,
             mode='exact', energy=False, stats=('chi2', 'mean', 'dkw'), mutants=HMC_MUTANTS, host_seeds=3)
    d.update(kw)
    return d


def _metric(test, G, mode, seed, dt, L, **kw):
    d = dict(kind='metric', test=test, C=4098, D=8, G=G, dt=dt, L=L, n=30, seed=seed, mode=mode, energy=True,
             stats=('chi2', 'mean', 'dkw', 'groups'), mutants=HMC_MUTANTS, host_seeds=3)
    d.update(kw)
    return d


def _linear(how, K, N, dt, L, n, seed, **kw):
    d = dict(kind='linear', test='linear', C=4096, K=K, N=N, tau=2.5, prior_var=5.0, dt=dt, L=L, n=n, seed=seed,
             how=how, energy=False, stats=('chi2', 'dkw'), mutants=HMC_MUTANTS, host_seeds=3)
    d.update(kw)
    return d


def _gibbs(how, move, seed, **kw):
    d = dict(kind='gibbs', test='gibbs', C=4096, K=3, N=24, n=30, prior_shape=2.0, prior_rate=0.2, prior_var=5.0,
             move=move, how=how, seed=seed, dt=0.21, L=5, stepsize=0.18, energy=False,
             stats=('tau_dkw', 'tau_score', 'chi2', 'dkw', 'corr'),
             mutants=('gamma_shape_plus_one', 'always_accept', 'flipped_sign'), host_seeds=3)
    d.update(kw)
    return d


# dt = 0.62 / sqrt(k) and 1.0 / sqrt(k): the steps of the measured power table (effective step
# dt sqrt(k) = 0.62 at D = 64, 1.0 at D = 8, 0.3 at D = 1024); the long chains scale as D^(-1/4)
_S = 1.0 / np.sqrt(2.5)
ROUTES = {
    # -- the Gaussian kind ------------------------------------------------------------------
    'gauss_n_rng_4096x64': _gauss('gauss', 4096, 64, 0.62 * _S, 7, 20, 101, 'sample_n_rng'),
    'gauss_n_rng_4096x33': _gauss('gauss', 4096, 33, 0.72 * _S, 7, 20, 102, 'sample_n_rng'),
    'gauss_n_rng_1024x1024': _gauss('gauss', 1024, 1024, 0.3 * _S, 7, 8, 103, 'sample_n_rng_always'),
    'gauss_n_split_1024x1024': _gauss('gauss', 1024, 1024, 0.3 * _S, 7, 8, 104, 'sample_n_split'),
    'gauss_n_supplied_4096x64': _gauss('gauss', 4096, 64, 0.62 * _S, 7, 20, 105, 'sample_n_supplied'),
    'gauss_single_4096x64': _gauss('gauss', 4096, 64, 0.62 * _S, 7, 20, 106, 'sample'),
    'gauss_fma_4096x64': _gauss('gauss', 4096, 64, 0.62 * _S, 7, 20, 107, 'sample_n_rng', mode='fma'),
    'gauss_per_step_4096x8': _gauss('gauss_steps', 4096, 8, 1.0 * _S, 5, 40, 108, 'per_step', energy=True),
    'gauss_graph_4096x8': _gauss('gauss_steps', 4096, 8, 1.0 * _S, 5, 40, 109, 'graph', energy=True),
    'gauss_long_single_1024x8200': _gauss('gauss_long', 1024, 8200, 0.18 * _S, 7, 3, 110, 'long_sample',
                                          host_seeds=2),
    'gauss_long_n_1024x8200': _gauss('gauss_long', 1024, 8200, 0.18 * _S, 7, 3, 111, 'long_sample_n',
                                     host_seeds=2),
    # -- the diagonal-metric tier -------------------------------------------------------------
    # (the largest effective step dt * factor stays below 1.42 at L = 3 and 1.56 at L = 4, beyond
    # which exp(-Delta) has no variance; ``energy_moment`` refuses such a setting)
    'metric_3x8': _metric('metric', 3, 'exact', 201, 0.97, 3),
    'metric_8': _metric('metric', 1, 'exact', 202, 0.95, 4),
    'metric_3x8_fma': _metric('metric', 3, 'fma', 203, 0.97, 3),
    # 70 adapting transitions from step 1.0 at rates 1.06 / 0.9 (a chain's step settles at acceptance
    # ln(1 / 0.9) / (ln 1.06 + ln(1 / 0.9)) = 0.64; ten transitions after the last window it is not
    # settled yet and the 40 kept transitions accept 0.73 in tests/metric_ref.py's warm-up), then exact draws and 40 more
    'after_warmup': _metric('warmup', 1, 'exact', 204, 1.0, 6, kind='warmup', n=40, n_warmup=70,
                            uprate=1.06, downrate=0.9, energy=False, stats=('chi2', 'mean', 'dkw')),
    # -- polynomial and linear conditionals at fixed tau --------------------------------------
    'poly_fused_sample': _linear('poly_sample', 4, 20, 0.2, 4, 30, 301),
    'poly_fused_sample_n': _linear('poly_sample_n', 4, 20, 0.2, 4, 30, 302),
    'poly_wave_sample': _linear('poly_sample', 4, 136, 0.08, 4, 30, 303),
    'poly_per_step': _linear('poly_per_step', 4, 20, 0.2, 4, 30, 304),
    'linear_resident_sample': _linear('linear_sample', 4, 20, 0.17, 5, 30, 305),
    'linear_resident_sample_n': _linear('linear_sample_n', 4, 20, 0.17, 5, 30, 306),
    'linear_per_step': _linear('linear_per_step', 4, 20, 0.17, 5, 30, 307),
    # -- the joint (coefficients, precision) Gibbs loop ---------------------------------------
    'gibbs_poly_hmc': _gibbs('sample_n', 'hmc', 401, model='poly'),
    'gibbs_poly_rwmc': _gibbs('sample_n', 'rwmc', 402, model='poly'),
    'gibbs_linear_hmc': _gibbs('sample_n', 'hmc', 403, model='linear', dt=0.17, L=5, stepsize=0.12),
    'gibbs_linear_rwmc': _gibbs('sample_n', 'rwmc', 404, model='linear', dt=0.17, L=5, stepsize=0.12),
    'gibbs_poly_loop': _gibbs('loop', 'hmc', 405, model='poly'),
    # -- replica exchange ------------------------------------------------------------------------
    'ladder': dict(kind='ladder', test='ladder', C=4096, D=8, R=4, n_ladders=1024, dt=1.0, L=5, n=40, seed=501,
                   energy=False, stats=('slots',), mutants=HMC_MUTANTS + ('swap_always',), host_seeds=3),
}
HOST_SEEDS = (11, 12, 13)          # the CPU power table's seeds (the first ``host_seeds`` of them)


def parametrisations(test):
    return sorted(n for n, r in ROUTES.items() if r['test'] == test)


def n_statistics(route):
    n = 0
    for s in route['stats']:
        n += {'groups': route.get('G', 1), 'slots': route.get('R', 1)}.get(s, 1)
    return n


def alpha_of(name):
    """The level of ONE statistic of route ``name``: its test function's ALPHA split over the
    function's parametrisations and over the route's statistics."""
    return ALPHA / len(parametrisations(ROUTES[name]['test'])) / n_statistics(ROUTES[name])


def alpha_energy_of(name):
    with_energy = [n for n in parametrisations(ROUTES[name]['test']) if ROUTES[n]['energy']]
    return ALPHA_ENERGY / max(1, len(with_energy))


# ---------------------------------------------------------------------------
# a route's exact target and its evaluation
# ---------------------------------------------------------------------------
_cache = {}


def target_of(name):
    """The exact target of a route (built once: the Gibbs quadrature takes seconds)."""
    r = ROUTES[name]
    key = (r['kind'], r.get('model'), r.get('K'), r.get('N'), r.get('G'), r.get('how') if r['kind'] == 'linear' else None)
    if key in _cache:
        return _cache[key]
    if r['kind'] == 'gauss':
        t = isotropic(r['k'], r['x0'])
    elif r['kind'] in ('metric', 'warmup'):
        t = GaussTarget(0.0, SIGMA8)
    elif r['kind'] == 'ladder':
        t = ladder(r['n_ladders'])[0]
    elif r['kind'] == 'linear':
        _, y, A = design_of(name)
        t = LinearConditional(A, y, r['tau'], r['prior_var'])
    else:
        _, y, A = design_of(name)
        t = GibbsJoint(A, y, r['prior_var'], gibbs_shape(r), r['prior_shape'])
    _cache[key] = t
    return t


def gibbs_shape(r, mutant=None):
    """oracle/ref_numpy.py:296-299: 0.5 n + prior.shape - 1."""
    return 0.5 * r['N'] + r['prior_shape'] - 1.0 + (1.0 if mutant == 'gamma_shape_plus_one' else 0.0)


def design_of(name):
    """(xs or None, ys, A [K x N]) of a linear / Gibbs route."""
    r = ROUTES[name]
    poly = r.get('model', 'poly') == 'poly' and not r.get('how', '').startswith('linear')
    if poly:
        return polynomial_case(r['K'], r['N'])
    y, A = dense_case(r['K'], r['N'])
    return None, y, A


def effective_steps(name):
    """dt sqrt(k) per dimension (``[G x D]`` with a metric): the oscillators' steps of the
    energy identity."""
    r = ROUTES[name]
    if r['kind'] == 'gauss':
        return np.full((1, r['D']), r['dt'] * np.sqrt(r['k']))
    return r['dt'] * metric_rows(SIGMA8, r['G']) / SIGMA8[None, :]


def start_of(name):
    """The exact start draws of the device test (fixed by the route's seed)."""
    r = ROUTES[name]
    rs = np.random.RandomState(r['seed'])
    return target_of(name).sample(rs, r['C'], r.get('D'))


def evaluate(name, x, tau=None, energies=None):
    """Every statistic of route ``name`` on the states ``x`` (``[C x D]``; Gibbs: also ``tau``
    ``[C]``) of ONE time point and, where the route has it, the energies
    ``(E_before, E_after)`` of ONE transition.  A list of checks."""
    r, t = ROUTES[name], target_of(name)
    a = alpha_of(name)
    z = t.standardise(x, tau) if r['kind'] == 'gibbs' else t.standardise(x)
    out = []
    for s in r['stats']:
        if s == 'chi2':
            out.append(pooled_chi2(z, a))
        elif s == 'mean':
            out.append(pooled_mean(z, a))
        elif s == 'dkw':
            out.append(dkw(z, stats.norm.cdf, a, 'DKW against Phi'))
        elif s == 'groups':
            for g in range(r['G']):
                out.append(pooled_chi2(z[g::r['G']], a, 'chi2 of group %d' % g))
        elif s == 'slots':
            for g in range(r['R']):
                out.append(pooled_chi2(z[g::r['R']], a, 'pooled chi2 of slot %d' % g))
        elif s == 'tau_dkw':
            out.append(unit_interval(t.cdf(tau), a, 'DKW of F(tau) against U(0,1)'))
        elif s == 'tau_score':
            u = np.clip(t.cdf(tau), 1e-300, 1.0 - 1e-16)
            out.append(pooled_mean(stats.norm.ppf(u), a, 'mean normal score of F(tau)'))
        elif s == 'corr':
            # u ~ U(0, 1) and |z|^2 ~ chi^2_K independent: known moments, N(0, 1 / C) by the CLT
            u, n2 = t.cdf(tau), np.sum(z * z, axis=1)
            c = (u - 0.5) * (n2 - r['K']) / np.sqrt(2.0 * r['K'] / 12.0)
            out.append(pooled_mean(c, a, 'corr(F(tau), |z|^2)'))
        else:
            raise KeyError(s)
    if r['energy'] and energies is not None:
        out.append(energy_identity(energies[0], energies[1], effective_steps(name), r['L'], alpha_energy_of(name)))
    return out


def chi2_margin(checks):
    """The largest |z| / threshold over the chi^2 statistics of a run."""
    return max(abs(c['z']) / c['z_threshold'] for c in checks if c['kind'] == 'chi2')


def margin(checks):
    """The largest |z| / threshold over every statistic that has a z."""
    return max(abs(c['z']) / c['z_threshold'] for c in checks if 'z' in c)


# ---------------------------------------------------------------------------
# the host sampler at a route's settings
# ---------------------------------------------------------------------------
def run_host(name, seed, mutant=None):
    """The host sampler at the settings of route ``name`` from exact draws; returns
    dict(x, tau, energies, acceptance)."""
    r, t = ROUTES[name], target_of(name)
    rs = np.random.RandomState(seed)
    C, n = r['C'], r['n']
    kind = r['kind']
    hmc_mut = mutant if mutant in HMC_MUTANTS else None
    n_acc, en, tau = 0.0, None, None
    if kind == 'gibbs':
        # the start depends on the seed alone: the inverse-CDF draws are made once per (target, seed)
        key = ('start', id(t), seed)
        if key not in _cache:
            _cache[key] = t.sample(rs, C) + (rs.get_state(),)
        theta, tau, state = _cache[key]
        rs.set_state(state)
        y, A = design_of(name)[1:]
        var = np.full(r['K'], r['prior_var'])
        for _ in range(n):
            tc = tau[:, None]
            pot = lambda q: 0.5 * tau * np.sum((q.dot(A) - y) ** 2, axis=1) + 0.5 * np.sum(q * q / var, axis=1)
            if r['move'] == 'hmc':
                theta, acc, _, _ = hmc_transition(rs, theta, pot, lambda q: tc * (q.dot(A) - y).dot(A.T),
                                                  r['dt'], r['L'], mutant=hmc_mut)
            else:
                prop = theta + rs.uniform(-r['stepsize'], r['stepsize'], size=theta.shape)
                zero = np.zeros(C)
                acc = _accept(rs, C, pot(theta), pot(prop), zero, zero, hmc_mut)
                theta = np.where(acc[:, None], prop, theta)
            n_acc += acc.mean()
            chi2 = np.sum((theta.dot(A) - y) ** 2, axis=1)
            tau = rs.gamma(gibbs_shape(r, mutant), size=C) / (0.5 * chi2 + r['prior_shape'])
        return dict(x=theta, tau=tau, energies=None, acceptance=n_acc / n)
    x = t.sample(rs, C, r.get('D'))
    scale, dt = None, r['dt']
    if kind in ('metric', 'warmup'):
        scale = np.tile(metric_rows(SIGMA8, r['G']), (C // r['G'], 1))
    if kind == 'ladder':
        k = ladder(r['n_ladders'])[1]
        dt = r['dt'] / np.sqrt(k)
    if kind == 'warmup':
        # the step-size rule of the warm-up (the metric stays the fixed mismatched one): every chain's
        # step times uprate after an accepted move, times downrate otherwise -- not invariant, so from
        # over-dispersed starts like a warm-up; then exact draws again
        dt = np.full(C, r['dt'])
        x = 2.0 * x
        for _ in range(r['n_warmup']):
            x, acc, _, _ = hmc_transition(rs, x, t.potential, t.force, dt, r['L'], scale)
            dt = np.where(acc, dt * r['uprate'], dt * r['downrate'])
        x = t.sample(rs, C, r['D'])
    for i in range(n):
        x, acc, eb, ea = hmc_transition(rs, x, t.potential, t.force, dt, r['L'], scale, hmc_mut)
        n_acc += acc.mean()
        en = (eb, ea)
        if kind == 'ladder':
            x, _ = swap_round(rs, x, k, r['R'], i & 1, mutant)
    return dict(x=x, tau=None, energies=en, acceptance=n_acc / n)
