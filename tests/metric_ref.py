"""Host restatement (numpy) of the diagonal-metric layer: the three scaled leapfrog updates of
``csrc/metric.hip``, the streaming moments, the pooled scale, the window schedule, a whole
metric transition and a whole windowed warm-up -- written from the contract in
``include/binf_hip.h``, not from the kernels.  Nothing here calls into the library.

Every multiply and add is one numpy operation on float64, so each is rounded separately; FMA
mode goes through the C oracle's ``fma`` (one rounding), as ``tests/chain_contract.py`` does.
Sums over chains take the diagnostics' order (``diagnostics_ref.blocked_sum``); the energies
of a transition are the existing oracle's (``ref_numpy``: numpy's pairwise ``np.sum``, the
clipped exponential of the accept test).

    h = d * s[c % G, i]      d = dt_c or the scalar timestep, 0.5 * d first for a half kick
    kick    p - h * g        FMA: fma(-h, g, p)
    drift   q + p * h        FMA: fma(p, h, q)

    accumulate   first: k0 = x, s1 = s2 = 0; always d = x - k0, s1 += d, s2 += d * d
    pool         mean_c = k0 + s1 / n, m2_c = s2 - (s1 * s1) / n over the chains c = g (mod G)
                 W = blocked(m2_c), mbar = blocked(mean_c) / Cg, B = blocked((mean_c - mbar)^2)
                 var = (W + n * B) / (N - 1), N = n * Cg
                 regularised: (N / (N + 5)) * var + 1e-3 * (5 / (N + 5))
                 scale = sqrt(var) where var is finite and > 0, else unchanged
"""
import numpy as np

import diagnostics_ref as DR
from oracle import c_oracle
from oracle import ref_numpy as R

f64 = np.float64


# ---------------------------------------------------------------------------
# scaled leapfrog pieces
# ---------------------------------------------------------------------------
def step_matrix(scale, C, timestep, dt_chain=None, half=False):
    """h [C x D]: one rounding per element."""
    scale = np.atleast_2d(np.asarray(scale, dtype=f64))
    G = scale.shape[0]
    assert C % G == 0
    d = np.full(C, f64(timestep)) if dt_chain is None else np.asarray(dt_chain, dtype=f64)
    if half:
        d = f64(0.5) * d
    with np.errstate(all='ignore'):
        return d[:, None] * scale[np.arange(C) % G]


def kick(p, g, scale, timestep, dt_chain=None, half=False, fma=False):
    h = step_matrix(scale, p.shape[0], timestep, dt_chain, half)
    with np.errstate(all='ignore'):
        return c_oracle.fma(-h, g, p) if fma else p - h * g


def drift(q, p, scale, timestep, dt_chain=None, fma=False):
    h = step_matrix(scale, q.shape[0], timestep, dt_chain)
    with np.errstate(all='ignore'):
        return c_oracle.fma(p, h, q) if fma else q + p * h


def kick_drift(q, p, g, scale, timestep, dt_chain=None, fma=False):
    """(q, p): the kick, then the drift with the new p."""
    pn = kick(p, g, scale, timestep, dt_chain, False, fma)
    return drift(q, pn, scale, timestep, dt_chain, fma), pn


def leapfrog(q, p, grad, scale, timestep, dt_chain, nsteps, fma=False):
    """The sampler's sequence: half kick, drift, (nsteps - 1) x [kick + drift], half kick."""
    p = kick(p, grad(q), scale, timestep, dt_chain, True, fma)
    q = drift(q, p, scale, timestep, dt_chain, fma)
    for _ in range(max(1, int(nsteps)) - 1):
        q, p = kick_drift(q, p, grad(q), scale, timestep, dt_chain, fma)
    p = kick(p, grad(q), scale, timestep, dt_chain, True, fma)
    return q, p


# ---------------------------------------------------------------------------
# streaming moments and the pooled scale
# ---------------------------------------------------------------------------
class Moments(object):
    """k0, s1, s2 [C x D] after ``add`` calls; the first call starts them."""

    def __init__(self):
        self.k0 = self.s1 = self.s2 = None
        self.n = 0

    def add(self, x, first=None):
        x = np.asarray(x, dtype=f64)
        if first is None:
            first = self.n == 0
        with np.errstate(all='ignore'):
            if first:
                self.k0, self.s1, self.s2 = x.copy(), np.zeros_like(x), np.zeros_like(x)
                self.n = 0
            d = x - self.k0
            self.s1 = self.s1 + d
            self.s2 = self.s2 + d * d
        self.n += 1
        return self

    def mean(self):
        with np.errstate(all='ignore'):
            return self.k0 + self.s1 / f64(self.n)

    def m2(self):
        with np.errstate(all='ignore'):
            return self.s2 - (self.s1 * self.s1) / f64(self.n)


def accumulate(record):
    """The moments of a stacked ``[n x C x D]`` record, streamed draw by draw."""
    m = Moments()
    for x in record:
        m.add(x)
    return m


def pool_parts(k0, s1, s2, n, G):
    """dict(W, mbar, B, var, N, Cg), each [G x D] (var before the shrinkage)."""
    C, D = k0.shape
    assert G >= 1 and C % G == 0 and n >= 1
    Cg = C // G
    fn = f64(n)
    N = f64(n * Cg)
    with np.errstate(all='ignore'):
        mean = k0 + s1 / fn
        m2 = s2 - (s1 * s1) / fn
        W, mbar, B = np.empty((G, D)), np.empty((G, D)), np.empty((G, D))
        for g in range(G):
            W[g] = DR.blocked_sum(m2[g::G])
            mbar[g] = DR.blocked_sum(mean[g::G]) / f64(Cg)
            e = mean[g::G] - mbar[g]
            B[g] = DR.blocked_sum(e * e)
        var = (W + fn * B) / (N - f64(1.0))
    return dict(W=W, mbar=mbar, B=B, var=var, N=N, Cg=Cg, mean=mean, m2=m2)


def pool(k0, s1, s2, n, G, regularise, scale):
    """The new ``[G x D]`` scale (``scale``: the previous one, kept where the variance is not a
    positive finite number)."""
    parts = pool_parts(k0, s1, s2, n, G)
    var, N = parts['var'], parts['N']
    with np.errstate(all='ignore'):
        if regularise:
            var = (N / (N + f64(5.0))) * var + f64(1e-3) * (f64(5.0) / (N + f64(5.0)))
        ok = np.isfinite(var) & (var > 0.0)
        return np.where(ok, np.sqrt(np.where(ok, var, 1.0)), np.atleast_2d(scale))


# ---------------------------------------------------------------------------
# window schedule
# ---------------------------------------------------------------------------
def window_schedule(n, init=75, term=50, base=25):
    """Stan's slow windows, [(start, stop)), by walking the transitions as Stan's
    windowed_adaptation does (a counter and the index of the next window's last transition)."""
    if n < init + term + base:
        init, term = int(0.15 * n), int(0.1 * n)
        base = n - init - term
    if base < 1:
        return []
    out, size, next_end, start = [], base, init + base - 1, init
    for t in range(n):
        inside = init <= t < n - term
        if inside and t == next_end:
            out.append((start, t + 1))
            start = t + 1
            if next_end == n - term - 1:
                continue
            size *= 2
            next_end = t + size
            if next_end == n - term - 1:
                continue
            if next_end + 2 * size >= n - term:
                next_end = n - term - 1
    return out


# ---------------------------------------------------------------------------
# a whole transition, a whole warm-up
# ---------------------------------------------------------------------------
def row_sums(a):
    """np.sum of every row (each a contiguous vector: numpy's pairwise order)."""
    return np.array([np.sum(np.ascontiguousarray(r)) for r in a])


class GaussTarget(object):
    """The isotropic Gaussian as the package evaluates it (reference TestHO)."""

    def __init__(self, k=1.0, x0=0.0):
        self.k, self.x0 = f64(k), f64(x0)

    def log_prob(self, x):
        return (f64(-0.5) * self.k) * row_sums((x - self.x0) ** 2)

    def gradient(self, x):
        return self.k * (x - self.x0)


class DiagGaussTarget(object):
    """log p = -0.5 sum (x / sigma)^2: the anisotropic Gaussian of the warm-up tests."""

    def __init__(self, sigma):
        self.sigma = np.asarray(sigma, dtype=f64)

    def log_prob(self, x):
        z = x / self.sigma
        return f64(-0.5) * np.sum(z * z, axis=1)

    def gradient(self, x):
        return x / (self.sigma * self.sigma)


class MetricHMC(object):
    """``HMCSampler(pdf, state, ..., metric=scale)`` on the per-step tier, chain-batched."""

    def __init__(self, target, state, timestep, nsteps, scale, adaption_limit=0, uprate=1.05,
                 downrate=0.95, fma=False):
        self.target, self.state = target, np.array(state, dtype=f64)
        C = self.state.shape[0]
        self.timestep, self.dt_chain = f64(timestep), None
        self.nsteps, self.limit = int(nsteps), adaption_limit
        self.uprate, self.downrate, self.fma = f64(uprate), f64(downrate), fma
        self.scale = np.atleast_2d(np.array(scale, dtype=f64))
        self.counter = 0
        self.n_accepted = np.zeros(C, dtype=np.int64)
        self.accepted = self.e_before = self.e_after = None

    def energy(self, q, p):
        return (-self.target.log_prob(q)) + f64(0.5) * row_sums(p ** 2)

    def sample(self, p0, u):
        C = self.state.shape[0]
        adapt = (self.counter + 1) < self.limit
        if adapt and self.dt_chain is None:
            self.dt_chain = np.full(C, self.timestep)
        q0, p = self.state, np.array(p0, dtype=f64)
        eb = self.energy(q0, p)
        q, p = leapfrog(q0.copy(), p, self.target.gradient, self.scale, self.timestep, self.dt_chain,
                        self.nsteps, self.fma)
        with np.errstate(all='ignore'):
            ea = self.energy(q, p)
            acc = np.asarray(u, dtype=f64) < R.exp(-(ea - eb))
        self.state = np.where(acc[:, None], q, q0)
        self.n_accepted += acc
        if adapt:
            self.dt_chain = np.where(acc, self.dt_chain * self.uprate, self.dt_chain * self.downrate)
        self.accepted, self.e_before, self.e_after = acc, eb, ea
        self.counter += 1
        return self.state


class Warmup(object):
    """``WindowedWarmup`` around a :class:`MetricHMC`."""

    def __init__(self, hmc, n_warmup, init=75, term=50, base=25, regularise=True):
        self.hmc, self.n = hmc, int(n_warmup)
        self.windows = window_schedule(self.n, init, term, base)
        self.regularise = regularise
        self.G = hmc.scale.shape[0]
        hmc.limit = max(hmc.limit, hmc.counter + self.n + 1)
        self.t = 0
        self.mom = Moments()

    def step(self, p0, u):
        x = self.hmc.sample(p0, u)
        for a, b in self.windows:
            if a <= self.t < b:
                self.mom.add(x, first=self.t == a)
                if self.t == b - 1:
                    self.hmc.scale = pool(self.mom.k0, self.mom.s1, self.mom.s2, self.mom.n, self.G,
                                          self.regularise, self.hmc.scale)
        self.t += 1
        return x


# ---------------------------------------------------------------------------
# the statistical experiment of the warm-up tests, in numpy
# ---------------------------------------------------------------------------
SIGMA8 = 100.0 ** (np.arange(8) / 7.0)          # 1 ... 100, a constant ratio between neighbours


def max_split_rhat(draws):
    """draws [T x C x D] -> max over dimensions of split-R^ (diagnostics_ref)."""
    mo = DR.moments(draws, 2)
    return float(np.max(DR.summary(mo['mean'], mo['m2'], None, mo['n'])['rhat']))


def experiment(seed, with_metric, sigma=SIGMA8, C=16, nsteps=5, timestep=0.5, n_warmup=300, n_keep=200,
               windows=(20, 40, 20), rates=(1.02, 0.9)):
    """The 8-dimensional Gaussian: 16 chains started at 3 sigma z, 300 adapting transitions
    (with or without the windowed metric), 200 kept.  Returns (max split-R^, scale / sigma
    [G x D], kept draws)."""
    rs = np.random.RandomState(seed)
    D = len(sigma)
    start = 3.0 * sigma * rs.standard_normal((C, D))
    hmc = MetricHMC(DiagGaussTarget(sigma), start, timestep, nsteps, np.ones((1, D)),
                    uprate=rates[0], downrate=rates[1])
    if with_metric:
        w = Warmup(hmc, n_warmup, *windows)
        for _ in range(n_warmup):
            w.step(rs.standard_normal((C, D)), rs.uniform(size=C))
    else:
        hmc.limit = n_warmup + 1
        for _ in range(n_warmup):
            hmc.sample(rs.standard_normal((C, D)), rs.uniform(size=C))
    kept = np.empty((n_keep, C, D))
    for t in range(n_keep):
        kept[t] = hmc.sample(rs.standard_normal((C, D)), rs.uniform(size=C))
    return max_split_rhat(kept), hmc.scale / sigma, kept
