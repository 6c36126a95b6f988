"""Host restatement (numpy) of the dense-metric layer: the three triangular matrix-vector
leapfrog updates of ``csrc/dense_metric.hip``, the streaming pooled co-moments, the pooled
covariance with its Cholesky factor, a whole dense-metric transition and a whole windowed
covariance warm-up -- written from the contract in ``include/binf_hip.h``, not from the
kernels.  Nothing here calls into the library.

Every multiply and add is one numpy operation on float64, so each is rounded separately; FMA
mode goes through the C oracle's ``fma`` (one rounding), as ``tests/chain_contract.py`` does.
Sums over chains take the diagnostics' order (``diagnostics_ref.blocked_sum``).

    d = dt_c or the scalar timestep, 0.5 * d first for a half kick;  L = chol[c % G]
    kick    t_i = sum_{j = i .. D-1} L[j][i] g_j      p - d * t      FMA: fma(-d, t, p)
    drift   v_i = sum_{j = 0 .. i}   L[i][j] p_j      q + v * d      FMA: fma(v, d, q)
            one chain of additions in ascending j, the first term the rounded product alone,
            later terms t + L * g (FMA: fma(L, g, t)); nothing above the diagonal is read

    comoments    first: k0[g] = x[chain g], s1 = s2 = 0; always d_c = x_c - k0[g] over the
                 chains c = g (mod G): s1 += blocked(d_ci), s2_ij += blocked(d_ci * d_cj), j <= i
    factor       N = n * C / G;  cov_ij = (s2_ij - (s1_i * s1_j) / N) / (N - 1)
                 regularised: (N / (N + 5)) * cov_ij, + 1e-3 * (5 / (N + 5)) on the diagonal
                 L column by column: a = cov_ij - sum_k L_ik L_jk (sequential, unfused),
                 L_jj = sqrt(a), L_ij = a / L_jj; taken if every pivot is finite and > 0 and
                 every entry finite, else the group keeps its factor and status = 1
"""
import numpy as np

import diagnostics_ref as DR
import metric_ref as MR
from oracle import c_oracle
from oracle import ref_numpy as R

f64 = np.float64


# ---------------------------------------------------------------------------
# triangular matrix-vector products, chain-batched
# ---------------------------------------------------------------------------
def _chol3(chol):
    chol = np.asarray(chol, dtype=f64)
    return chol[None] if chol.ndim == 2 else chol


def _dt(C, timestep, dt_chain, half):
    d = np.full(C, f64(timestep)) if dt_chain is None else np.asarray(dt_chain, dtype=f64)
    return f64(0.5) * d if half else d


def lt_matvec(chol, g, fma=False):
    """t [C x D], t_ci = sum_{j >= i} L[j][i] g_cj with L = chol[c % G]: ascending j."""
    chol, g = _chol3(chol), np.asarray(g, dtype=f64)
    C, D = g.shape
    G = chol.shape[0]
    assert C % G == 0 and chol.shape[1:] == (D, D)
    t = np.empty((C, D))
    with np.errstate(all='ignore'):
        for gi in range(G):
            L, gg = chol[gi], g[gi::G]
            tt = np.empty_like(gg)
            for j in range(D):
                row, gj = L[j, :j + 1], gg[:, j:j + 1]              # L[j][i], i <= j: below the diagonal
                if j:
                    tt[:, :j] = c_oracle.fma(row[None, :j], gj, tt[:, :j]) if fma else tt[:, :j] + row[None, :j] * gj
                tt[:, j] = row[j] * gj[:, 0]                        # the first term of t_j
            t[gi::G] = tt
    return t


def l_matvec(chol, p, fma=False):
    """v [C x D], v_ci = sum_{j <= i} L[i][j] p_cj with L = chol[c % G]: ascending j."""
    chol, p = _chol3(chol), np.asarray(p, dtype=f64)
    C, D = p.shape
    G = chol.shape[0]
    assert C % G == 0 and chol.shape[1:] == (D, D)
    v = np.empty((C, D))
    with np.errstate(all='ignore'):
        for gi in range(G):
            L, pp = chol[gi], p[gi::G]
            vv = L[:, 0][None, :] * pp[:, 0:1]                      # the first term of every v_i
            for j in range(1, D):
                col, pj = L[j:, j], pp[:, j:j + 1]                  # L[i][j], i >= j
                vv[:, j:] = c_oracle.fma(col[None, :], pj, vv[:, j:]) if fma else vv[:, j:] + col[None, :] * pj
            v[gi::G] = vv
    return v


def kick(p, g, chol, timestep, dt_chain=None, half=False, fma=False):
    d = _dt(p.shape[0], timestep, dt_chain, half)[:, None]
    t = lt_matvec(chol, g, fma)
    with np.errstate(all='ignore'):
        return c_oracle.fma(-d, t, p) if fma else p - d * t


def drift(q, p, chol, timestep, dt_chain=None, fma=False):
    d = _dt(q.shape[0], timestep, dt_chain, False)[:, None]
    v = l_matvec(chol, p, fma)
    with np.errstate(all='ignore'):
        return c_oracle.fma(v, d, q) if fma else q + v * d


def kick_drift(q, p, g, chol, timestep, dt_chain=None, fma=False):
    """(q, p): the kick of the whole row, then the drift with the new p."""
    pn = kick(p, g, chol, timestep, dt_chain, False, fma)
    return drift(q, pn, chol, timestep, dt_chain, fma), pn


def leapfrog(q, p, grad, chol, timestep, dt_chain, nsteps, fma=False):
    """The sampler's sequence: half kick, drift, (nsteps - 1) x [kick + drift], half kick."""
    p = kick(p, grad(q), chol, timestep, dt_chain, True, fma)
    q = drift(q, p, chol, timestep, dt_chain, fma)
    for _ in range(max(1, int(nsteps)) - 1):
        q, p = kick_drift(q, p, grad(q), chol, timestep, dt_chain, fma)
    p = kick(p, grad(q), chol, timestep, dt_chain, True, fma)
    return q, p


# ---------------------------------------------------------------------------
# streaming pooled co-moments, covariance, factor
# ---------------------------------------------------------------------------
class CoMoments(object):
    """k0, s1 [G x D], s2 [G x D x D] (lower triangle; what lies above is left as given)."""

    def __init__(self, G, above=0.0):
        self.G, self.above = int(G), above
        self.k0 = self.s1 = self.s2 = None
        self.n = 0

    def add(self, x, first=None):
        x = np.asarray(x, dtype=f64)
        C, D = x.shape
        G = self.G
        assert C % G == 0
        if first is None:
            first = self.n == 0
        low = np.tril(np.ones((D, D), dtype=bool))
        with np.errstate(all='ignore'):
            if first:
                self.k0, self.s1 = x[:G].copy(), np.zeros((G, D))
                s2 = np.full((G, D, D), f64(self.above)) if self.s2 is None else self.s2.copy()
                s2[:, low] = 0.0
                self.s2, self.n = s2, 0
            s1, s2 = self.s1.copy(), self.s2.copy()
            for g in range(G):
                d = x[g::G] - self.k0[g]
                s1[g] = self.s1[g] + DR.blocked_sum(d)
                pair = DR.blocked_sum(d[:, :, None] * d[:, None, :])
                s2[g][low] = (self.s2[g] + pair)[low]
            self.s1, self.s2 = s1, s2
        self.n += 1
        return self


def comoments(record, G):
    """The co-moments of a stacked ``[n x C x D]`` record, streamed draw by draw."""
    m = CoMoments(G)
    for x in record:
        m.add(x)
    return m


def covariance(s1, s2, n, C, regularise):
    """cov [G x D x D], lower triangle (zeros above)."""
    G, D = s1.shape
    N = f64(n * (C // G))
    assert C % G == 0 and n >= 1 and N >= 2
    with np.errstate(all='ignore'):
        cov = (s2 - (s1[:, :, None] * s1[:, None, :]) / N) / (N - f64(1.0))
        if regularise:
            cov = (N / (N + f64(5.0))) * cov
            eye = np.eye(D, dtype=bool)
            cov[:, eye] = cov[:, eye] + f64(1e-3) * (f64(5.0) / (N + f64(5.0)))
    return np.where(np.tril(np.ones((D, D), dtype=bool)), cov, 0.0)


def cholesky_lower(a):
    """(L, ok) of one [D x D] matrix (lower triangle read).  Every entry loses L_ik * L_jk in
    ascending k, the product rounded first -- here one outer product per k over the trailing
    block, the same sequence per entry as the column-by-column statement.  ``ok``: every pivot
    finite and > 0, every entry finite."""
    a = np.tril(np.array(a, dtype=f64))
    D = a.shape[0]
    ok = True
    with np.errstate(all='ignore'):
        for k in range(D):
            piv = a[k, k]
            ok = ok and bool(np.isfinite(piv) and piv > 0.0)
            lkk = np.sqrt(piv)
            col = a[k + 1:, k] / lkk
            a[k, k], a[k + 1:, k] = lkk, col
            a[k + 1:, k + 1:] = a[k + 1:, k + 1:] - col[:, None] * col[None, :]
        a = np.where(np.tril(np.ones((D, D), dtype=bool)), a, 0.0)
    return a, ok and bool(np.isfinite(a).all())


def cholesky_columns(a):
    """The header's statement, literally (column by column, scalar loops): for small D."""
    D = a.shape[0]
    L = np.zeros((D, D))
    with np.errstate(all='ignore'):
        for j in range(D):
            for i in range(j, D):
                s = f64(a[i, j])
                for k in range(j):
                    s = s - L[i, k] * L[j, k]
                L[i, j] = np.sqrt(s) if i == j else s / L[j, j]
    return L


def factor(s1, s2, n, C, regularise, chol):
    """(chol, work, status): the new ``[G x D x D]`` factors (``chol``: the previous ones, kept
    where the factorisation fails), what the work buffer holds, int32 ``[G]`` flags."""
    cov = covariance(s1, s2, n, C, regularise)
    G = cov.shape[0]
    out, work, status = np.array(_chol3(chol), dtype=f64), np.empty_like(cov), np.zeros(G, dtype=np.int32)
    for g in range(G):
        work[g], ok = cholesky_lower(cov[g])
        if ok:
            out[g] = work[g]
        else:
            status[g] = 1
    return out, work, status


# ---------------------------------------------------------------------------
# a whole transition, a whole warm-up
# ---------------------------------------------------------------------------
class CorrelatedGaussTarget(object):
    """log p = -0.5 x^T P x with a dense precision P."""

    def __init__(self, precision):
        self.P = np.asarray(precision, dtype=f64)

    def log_prob(self, x):
        return f64(-0.5) * np.sum(x * (x @ self.P), axis=1)

    def gradient(self, x):
        return x @ self.P


class DenseHMC(MR.MetricHMC):
    """``HMCSampler(pdf, state, ..., dense_metric=chol)`` on the per-step tier."""

    def __init__(self, target, state, timestep, nsteps, chol, **kw):
        D = np.asarray(state).shape[1]
        MR.MetricHMC.__init__(self, target, state, timestep, nsteps, np.ones((1, D)), **kw)
        self.chol = np.tril(np.array(_chol3(chol), dtype=f64))

    def sample(self, p0, u):
        C = self.state.shape[0]
        adapt = (self.counter + 1) < self.limit
        if adapt and self.dt_chain is None:
            self.dt_chain = np.full(C, self.timestep)
        q0, p = self.state, np.array(p0, dtype=f64)
        eb = self.energy(q0, p)
        q, p = leapfrog(q0.copy(), p, self.target.gradient, self.chol, self.timestep, self.dt_chain,
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


class DenseWarmup(object):
    """``WindowedWarmup(..., dense=True)`` around a :class:`DenseHMC`."""

    def __init__(self, hmc, n_warmup, init=75, term=50, base=25, regularise=True):
        self.hmc, self.n = hmc, int(n_warmup)
        self.windows = MR.window_schedule(self.n, init, term, base)
        self.regularise = regularise
        self.G = hmc.chol.shape[0]
        hmc.limit = max(hmc.limit, hmc.counter + self.n + 1)
        self.t = 0
        self.mom = CoMoments(self.G)
        self.status = np.zeros(self.G, dtype=np.int32)
        self.factors = []                                   # the factor after every window

    def step(self, p0, u):
        x = self.hmc.sample(p0, u)
        for a, b in self.windows:
            if a <= self.t < b:
                self.mom.add(x, first=self.t == a)
                if self.t == b - 1:
                    self.hmc.chol, _, self.status = factor(self.mom.s1, self.mom.s2, self.mom.n, x.shape[0],
                                                           self.regularise, self.hmc.chol)
                    self.factors.append(self.hmc.chol.copy())
        self.t += 1
        return x


# ---------------------------------------------------------------------------
# the statistical experiment: SIGMA8 rotated by a fixed random orthogonal matrix
# ---------------------------------------------------------------------------
def rotated_target(sigma=MR.SIGMA8, seed=1000):
    """(covariance, precision, its lower factor): Q diag(sigma^2) Q^T, Q the orthogonal factor
    of a fixed standard-normal matrix."""
    D = len(sigma)
    Q, _ = np.linalg.qr(np.random.RandomState(seed).standard_normal((D, D)))
    S = (Q * sigma ** 2) @ Q.T
    S = 0.5 * (S + S.T)
    P = (Q / sigma ** 2) @ Q.T
    return S, 0.5 * (P + P.T), np.linalg.cholesky(S)


def whitened_eigenvalues(chol, true_chol):
    """Eigenvalues of Ls^-1 (L L^T) Ls^-T: all 1 when the learnt factor is the true one."""
    M = np.linalg.solve(true_chol, chol)
    return np.linalg.eigvalsh(M @ M.T)


def experiment(seed, kind, C=16, nsteps=5, timestep=0.5, n_warmup=300, n_keep=200, windows=(20, 40, 20),
               rates=(1.02, 0.9)):
    """``metric_ref.experiment`` on the rotated Gaussian: ``kind`` 'none', 'diag' or 'dense'.
    Returns (max split-R^, whitened eigenvalues of the learnt M^-1 or None, kept draws)."""
    S, P, Ls = rotated_target()
    D = S.shape[0]
    rs = np.random.RandomState(seed)
    start = 3.0 * rs.standard_normal((C, D)) @ Ls.T
    target = CorrelatedGaussTarget(P)
    kw = dict(uprate=rates[0], downrate=rates[1])
    if kind == 'dense':
        hmc = DenseHMC(target, start, timestep, nsteps, np.eye(D), **kw)
        w = DenseWarmup(hmc, n_warmup, *windows)
    else:
        hmc = MR.MetricHMC(target, start, timestep, nsteps, np.ones((1, D)), **kw)
        w = MR.Warmup(hmc, n_warmup, *windows) if kind == 'diag' else None
    hmc.limit = n_warmup + 1
    for _ in range(n_warmup):
        p0, u = rs.standard_normal((C, D)), rs.uniform(size=C)
        w.step(p0, u) if w is not None else hmc.sample(p0, u)
    kept = np.empty((n_keep, C, D))
    for t in range(n_keep):
        kept[t] = hmc.sample(rs.standard_normal((C, D)), rs.uniform(size=C))
    if kind == 'dense':
        ev = whitened_eigenvalues(hmc.chol[0], Ls)
    elif kind == 'diag':
        ev = whitened_eigenvalues(np.diag(hmc.scale[0]), Ls)
    else:
        ev = None
    return MR.max_split_rhat(kept), ev, kept
