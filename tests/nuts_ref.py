"""Host restatement (numpy) of the no-U-turn transition of ``csrc/nuts.hip`` and of
``NUTSSampler``, written from the contract in ``include/binf_hip.h`` -- not from the kernel.
Nothing here calls into the library (FMA-mode leapfrog pieces go through the C oracle's
``fma``, as ``tests/metric_ref.py`` does).

Iterative multinomial NUTS.  Sub-tree U-turn checks go through per-depth checkpoints
(NumPyro's iterative tree); progressive sampling is uniform inside a sub-tree and biased at
the top (Stan).  Momenta are the whitened r ~ N(0, I) and keep their forward-time orientation:
a backward extension is a negative step, never a flip.

Every multiply and add is one numpy operation on float64; ``dot(a, b) = np.sum(a * b)`` and
``K = 0.5 * np.sum(r * r)`` per row (numpy's pairwise order), ``H = -logp + K``;
``expc(x) = np.exp(np.clip(x, -308, 709))`` -- numpy's exponential, which may differ from the
device's by an ulp: the weights ``w_sub, w_tree, acc`` are compared within a bound, and a test
that wants the same DECISIONS asserts ``Tree.min_margin`` first.

Per-chain uniforms of a transition: ``u[c, 0:S]``, ``S = 2 md + 2^md - 1``:
``udir = u[:md]``, ``umerge = u[md:2md]``, ``uleaf = u[2md:]`` by the leaf's number.
"""
import numpy as np

f64 = np.float64
RUN, TURN, SUBTURN, MAXD, DIV = 0, 1, 2, 3, 4
MUTANTS = ('no_subtree_check', 'cand_last_leaf', 'edges_not_updated')


def n_uniforms(max_depth):
    return 2 * max_depth + (1 << max_depth) - 1


def expc(x):
    with np.errstate(all='ignore'):
        return np.exp(np.clip(x, -308.0, 709.0))


def rowdot(a, b):
    """np.sum(a[c] * b[c]) for every row (the pairwise order of a contiguous row)."""
    with np.errstate(all='ignore'):
        return np.sum(np.ascontiguousarray(a * b), axis=1)


def trailing_ones(n):
    t = 0
    while (n >> t) & 1:
        t += 1
    return t


def checkpoint_range(n):
    """(lo, hi): checkpoint levels leaf ``n`` of a sub-tree is checked against (odd n), or
    ``hi`` the level an even leaf is stored at."""
    hi = bin(n >> 1).count('1')
    return hi - trailing_ones(n) + 1, hi


class Tree(object):
    """The device's tree state, field for field (``binf_nuts_args``), for C chains."""

    ROWS = ('q', 'r', 'g', 'cand', 'prop', 'q_out', 'rho_sub', 'rho_tree')

    def __init__(self, C, D, max_depth, max_delta=1000.0, mutant=None, fill=None):
        assert mutant is None or mutant in MUTANTS
        self.C, self.D, self.md, self.max_delta, self.mutant = C, D, int(max_depth), f64(max_delta), mutant
        z = (lambda *s: np.zeros(s)) if fill is None else (lambda *s: np.full(s, f64(fill)))
        for n in self.ROWS:
            setattr(self, n, z(C, D))
        self.edge_q, self.edge_r, self.edge_g = z(2, C, D), z(2, C, D), z(2, C, D)
        self.ck_r, self.ck_rho = z(C, self.md, D), z(C, self.md, D)
        for n in ('logp', 'eps', 'dt_dir', 'H0', 'href', 'w_sub', 'w_tree', 'acc', 'accept_stat'):
            setattr(self, n, z(C))
        self.u = z(C, n_uniforms(self.md))
        for n in ('j', 'n_sub', 'n_leap', 'v', 'status', 'tree_depth'):
            setattr(self, n, np.zeros(C, dtype=np.int32))
        self.moved, self.diverging = np.zeros(C, dtype=np.uint8), np.zeros(C, dtype=np.uint8)
        self.n_accepted, self.n_divergent = np.zeros(C, dtype=np.int64), np.zeros(C, dtype=np.int64)
        self.min_margin = np.inf          # smallest |u w - w'| / w of a selection so far
        self.href_lowered = 0             # leaves that took the H < href branch
        self.visited = [[] for _ in range(C)]     # (CPU tests) leaves in visiting order: copies of q

    def pending(self):
        return int(np.sum(self.status == RUN))

    def begin(self, q0, r0, g0, logp, eps, u):
        C, md = self.C, self.md
        self.q[...], self.r[...], self.g[...] = q0, r0, g0
        self.logp[...], self.eps[...], self.u[...] = logp, eps, u
        H = -self.logp + f64(0.5) * rowdot(self.r, self.r)
        self.H0[...], self.href[...] = H, H
        self.w_tree[...], self.w_sub[...], self.acc[...], self.accept_stat[...] = 1.0, 0.0, 0.0, 0.0
        self.rho_tree[...] = self.r
        for e in (0, 1):
            self.edge_q[e], self.edge_r[e], self.edge_g[e] = self.q, self.r, self.g
        self.prop[...] = self.q
        for n in ('j', 'n_sub', 'n_leap', 'status', 'tree_depth'):
            getattr(self, n)[...] = 0
        self.moved[...], self.diverging[...] = 0, 0
        self.v[...] = np.where(self.u[:, 0] < 0.5, 1, -1)
        self.dt_dir[...] = self.v.astype(f64) * self.eps
        self.visited = [[] for _ in range(C)]

    def _margin(self, lhs, rhs, w):
        with np.errstate(all='ignore'):
            m = np.abs(lhs - rhs) / w
        if m.size:
            self.min_margin = min(self.min_margin, float(np.min(m)))

    def leaf(self, logp, track=False):
        """One leaf for every chain that is still RUN; ``logp`` ``[C]`` of the working q."""
        md = self.md
        self.logp[...] = logp
        run = np.nonzero(self.status == RUN)[0]
        if run.size == 0:
            return
        q, r, g = self.q[run], self.r[run], self.g[run]
        if track:
            for k, c in enumerate(run):
                self.visited[c].append(q[k].copy())
        with np.errstate(all='ignore'):
            H = -self.logp[run] + f64(0.5) * rowdot(r, r)
            n = self.n_sub[run].copy()
            self.n_leap[run] += 1
            nl = self.n_leap[run]
            delta = H - self.H0[run]
            div = ~(delta <= self.max_delta)
        # ---- diverging chains finish at once -------------------------------------------
        status = np.where(div, DIV, RUN).astype(np.int32)
        ok = ~div
        acc, href = self.acc[run].copy(), self.href[run].copy()
        w_sub, w_tree = self.w_sub[run].copy(), self.w_tree[run].copy()
        j, v = self.j[run].copy(), self.v[run].copy()
        with np.errstate(all='ignore'):
            acc = np.where(ok, acc + np.minimum(1.0, expc(-delta)), acc)
            low = ok & (H < href)
            self.href_lowered += int(np.sum(low))
            s = np.where(low, expc(H - href), 1.0)
            wl = np.where(low, 1.0, expc(href - H))
            w_sub = np.where(low, w_sub * s, w_sub)
            w_tree = np.where(low, w_tree * s, w_tree)
            href = np.where(low, H, href)
            w_sub = np.where(ok, w_sub + wl, w_sub)
            uleaf = self.u[run, 2 * md + nl - 1]
            sel_cand = ok & (uleaf * w_sub < wl)
            self._margin((uleaf * w_sub)[ok], wl[ok], w_sub[ok])
            if self.mutant == 'cand_last_leaf':
                sel_cand = ok.copy()
        cand = self.cand[run]
        cand[sel_cand] = q[sel_cand]
        first = n == 0
        with np.errstate(all='ignore'):
            rho_sub = np.where(first[:, None], r, self.rho_sub[run] + r)
        rho_sub[div] = self.rho_sub[run][div]
        even = ok & (n % 2 == 0)
        hi = np.array([checkpoint_range(int(x))[1] for x in n], dtype=np.int64)
        nchk = np.array([trailing_ones(int(x)) for x in n], dtype=np.int64)
        ck_r, ck_rho = self.ck_r[run], self.ck_rho[run]
        ar = np.arange(run.size)
        ck_r[ar[even], hi[even]] = r[even]
        ck_rho[ar[even], hi[even]] = rho_sub[even]
        turn = np.zeros(run.size, dtype=bool)
        odd = ok & (n % 2 == 1)
        for t in range(int(nchk[odd].max()) if odd.any() else 0):
            m = odd & (nchk > t)
            lvl = hi[m] - t
            cr, crho = ck_r[ar[m], lvl], ck_rho[ar[m], lvl]
            with np.errstate(all='ignore'):
                sub = (rho_sub[m] - crho) + cr
                tt = (rowdot(cr, sub) <= 0.0) | (rowdot(r[m], sub) <= 0.0)
            turn[m] |= tt
        if self.mutant == 'no_subtree_check':
            turn[:] = False
        n_sub = np.where(ok, n + 1, n)
        status[turn] = SUBTURN
        merge = ok & ~turn & (n_sub == (1 << j.astype(np.int64)))
        umerge = self.u[run, md + np.minimum(j, md - 1)]
        with np.errstate(all='ignore'):
            sel_prop = merge & (umerge * w_tree < w_sub)
            self._margin((umerge * w_tree)[merge], w_sub[merge], w_tree[merge])
            w_tree = np.where(merge, w_tree + w_sub, w_tree)
            rho_tree = np.where(merge[:, None], self.rho_tree[run] + rho_sub, self.rho_tree[run])
        prop = self.prop[run]
        prop[sel_prop] = cand[sel_prop]
        moved = self.moved[run].copy()
        moved[sel_prop] = 1
        side = (v > 0).astype(np.int64)
        eq, er, eg = self.edge_q[:, run], self.edge_r[:, run], self.edge_g[:, run]
        if self.mutant != 'edges_not_updated':
            mm = ar[merge]
            eq[side[merge], mm], er[side[merge], mm], eg[side[merge], mm] = q[merge], r[merge], g[merge]
        j = np.where(merge, j + 1, j)
        with np.errstate(all='ignore'):
            tt = (rowdot(er[0], rho_tree) <= 0.0) | (rowdot(er[1], rho_tree) <= 0.0)
        status[merge & tt] = TURN
        status[merge & ~tt & (j == md)] = MAXD
        go = merge & (status == RUN)
        vnew = np.where(self.u[run, np.minimum(j, md - 1)] < 0.5, 1, -1).astype(np.int32)
        v = np.where(go, vnew, v)
        w_sub = np.where(go, 0.0, w_sub)
        n_sub = np.where(go, 0, n_sub)
        sd = (v > 0).astype(np.int64)
        q[go], r[go], g[go] = eq[sd[go], ar[go]], er[sd[go], ar[go]], eg[sd[go], ar[go]]
        # ---- finish ------------------------------------------------------------------------
        fin = status != RUN
        q_out = self.q_out[run]
        q_out[fin] = prop[fin]
        tree_depth = np.where(fin, j, self.tree_depth[run])
        with np.errstate(all='ignore'):
            accept_stat = np.where(fin, acc / nl.astype(f64), self.accept_stat[run])
            dt_dir = np.where(fin, 0.0, v.astype(f64) * self.eps[run])
        diverging = np.where(fin, status == DIV, self.diverging[run]).astype(np.uint8)
        self.n_divergent[run] += (status == DIV)
        self.n_accepted[run] += (fin & (moved != 0))
        # ---- scatter ----------------------------------------------------------------------
        self.q[run], self.r[run], self.g[run] = q, r, g
        self.cand[run], self.prop[run], self.q_out[run] = cand, prop, q_out
        self.rho_sub[run], self.rho_tree[run] = rho_sub, rho_tree
        self.ck_r[run], self.ck_rho[run] = ck_r, ck_rho
        self.edge_q[:, run], self.edge_r[:, run], self.edge_g[:, run] = eq, er, eg
        self.acc[run], self.href[run], self.w_sub[run], self.w_tree[run] = acc, href, w_sub, w_tree
        self.j[run], self.v[run], self.n_sub[run], self.status[run] = j, v, n_sub, status
        self.moved[run], self.diverging[run] = moved, diverging
        self.tree_depth[run], self.accept_stat[run], self.dt_dir[run] = tree_depth, accept_stat, dt_dir


# ---------------------------------------------------------------------------
# the leapfrog step of a leaf: the library's per-step launches, restated
# ---------------------------------------------------------------------------
class Integrator(object):
    """``kind``: 'identity', 'diag' (``param`` = scales ``[G x D]``) or 'dense' (``param`` =
    lower factors ``[G x D x D]``); ``fma``: the library's 'fma' mode."""

    def __init__(self, kind='identity', param=None, fma=False):
        self.kind, self.param, self.fma = kind, param, bool(fma)

    def _fma(self, a, b, c):
        from oracle import c_oracle
        return c_oracle.fma(a, b, c)

    def kick_half(self, p, g, dt):
        with np.errstate(all='ignore'):
            if self.kind == 'diag':
                import metric_ref as MR
                return MR.kick(p, g, self.param, 0.0, dt, True, self.fma)
            if self.kind == 'dense':
                import dense_metric_ref as DM
                return DM.kick(p, g, self.param, 0.0, dt, True, self.fma)
            d = (f64(0.5) * dt)[:, None]
            return self._fma(-d * np.ones_like(g), g, p) if self.fma else p - d * g

    def drift(self, q, p, dt):
        with np.errstate(all='ignore'):
            if self.kind == 'diag':
                import metric_ref as MR
                return MR.drift(q, p, self.param, 0.0, dt, self.fma)
            if self.kind == 'dense':
                import dense_metric_ref as DM
                return DM.drift(q, p, self.param, 0.0, dt, self.fma)
            d = dt[:, None]
            return self._fma(p, d * np.ones_like(p), q) if self.fma else q + p * d

    def step(self, tree, grad):
        """One leapfrog step of the tree's working state with ``dt_dir``, in place."""
        dt = tree.dt_dir.copy()
        tree.r[...] = self.kick_half(tree.r, tree.g, dt)
        tree.q[...] = self.drift(tree.q, tree.r, dt)
        tree.g[...] = grad(tree.q)
        tree.r[...] = self.kick_half(tree.r, tree.g, dt)


def transition(tree, integ, logp, grad, q0, r0, eps, u, track=False, on_leaf=None):
    """A whole transition of every chain; returns ``tree.q_out`` (a copy)."""
    tree.begin(q0, r0, grad(q0), logp(q0), eps, u)
    for _ in range((1 << tree.md) - 1):
        if tree.pending() == 0:
            break
        integ.step(tree, grad)
        tree.leaf(logp(tree.q), track=track)
        if on_leaf is not None:
            on_leaf(tree)
    assert tree.pending() == 0
    return tree.q_out.copy()


# ---------------------------------------------------------------------------
# dual averaging (Hoffman & Gelman 2014, algorithm 5), per chain
# ---------------------------------------------------------------------------
class DualAveraging(object):
    def __init__(self, eps, target=0.8, gamma=0.05, t0=10.0, kappa=0.75):
        self.eps = np.array(eps, dtype=f64)
        self.target, self.gamma, self.t0, self.kappa = f64(target), float(gamma), float(t0), float(kappa)
        C = self.eps.size
        self.hbar, self.logeps, self.logeps_bar, self.mu = np.zeros(C), np.zeros(C), np.zeros(C), np.zeros(C)
        self.restart()

    @staticmethod
    def scalars(t, gamma, t0, kappa):
        """(w1, k1, eta) of update number t = 1, 2, ...: what the host hands the kernel."""
        return 1.0 / (t + t0), float(np.sqrt(float(t))) / gamma, float(t) ** -kappa

    def restart(self):
        self.t = 0
        self.mu = np.log(f64(10.0) * self.eps)
        self.hbar[...], self.logeps_bar[...] = 0.0, 0.0

    def update(self, accept_stat):
        self.t += 1
        w1, k1, eta = (f64(x) for x in self.scalars(self.t, self.gamma, self.t0, self.kappa))
        self.hbar = (f64(1.0) - w1) * self.hbar + w1 * (self.target - accept_stat)
        self.logeps = self.mu - k1 * self.hbar
        self.logeps_bar = eta * self.logeps + (f64(1.0) - eta) * self.logeps_bar
        self.eps = np.exp(self.logeps)

    def finalise(self):
        self.eps = np.exp(self.logeps_bar)


class NUTS(object):
    """``NUTSSampler`` restated: ``sample(r0, u)`` is one transition of every chain."""

    def __init__(self, logp, grad, q, eps, max_depth=10, integ=None, adaption_limit=0, target=0.8,
                 max_delta=1000.0, gamma=0.05, t0=10.0, kappa=0.75, mutant=None):
        self.logp, self.grad = logp, grad
        self.q = np.array(q, dtype=f64)
        C, D = self.q.shape
        self.integ = integ if integ is not None else Integrator()
        self.tree = Tree(C, D, max_depth, max_delta, mutant)
        self.da = DualAveraging(np.full(C, f64(eps)) if np.ndim(eps) == 0 else eps, target, gamma, t0, kappa)
        self.adaption_limit, self.counter = int(adaption_limit), 0

    @property
    def eps(self):
        return self.da.eps

    def sample(self, r0, u):
        self.q = transition(self.tree, self.integ, self.logp, self.grad, self.q, r0, self.da.eps, u)
        if self.counter + 1 < self.adaption_limit:
            self.da.update(self.tree.accept_stat)
            if self.counter + 2 >= self.adaption_limit:
                self.da.finalise()
        self.counter += 1
        return self.q


# ---------------------------------------------------------------------------
# the stationarity cases (CPU and device tests share settings, seeds and statistics)
# ---------------------------------------------------------------------------
SIGMA5 = np.array([1.0, 2.0, 3.0, 5.0, 10.0])
STATIONARITY = {            # metric -> step, seed; 4000 chains x 3 transitions, max_depth 6
    'identity': dict(eps=0.9, seed=0),
    'diag': dict(eps=0.45, seed=1),
    'dense': dict(eps=0.45, seed=2),
}
STATIONARITY_C, STATIONARITY_N, STATIONARITY_MD = 4000, 3, 6


def rotation(D, seed=1000):
    rs = np.random.RandomState(seed)
    Q, R = np.linalg.qr(rs.standard_normal((D, D)))
    return Q * np.sign(np.diag(R))


class Case(object):
    """A Gaussian target and a (mismatched) metric: ``identity`` and ``diag`` on N(0, diag
    sigma^2), ``dense`` on its rotation; the metric is the target's scale times fixed factors
    in [0.5, 2] (invariance must hold for any positive definite metric)."""

    def __init__(self, kind, sigma=SIGMA5):
        self.kind, self.sigma = kind, np.asarray(sigma, dtype=f64)
        D = self.sigma.size
        factors = 2.0 ** np.random.RandomState(41).uniform(-1.0, 1.0, size=D)
        self.R = rotation(D) if kind == 'dense' else np.eye(D)
        self.precision = (self.R / (self.sigma * self.sigma)).dot(self.R.T)      # R diag(1/s^2) R'
        self.scale = self.chol = None
        if kind == 'diag':
            self.scale = (self.sigma * factors)[None, :]
        if kind == 'dense':
            m = (self.R * (self.sigma * factors) ** 2).dot(self.R.T)
            self.chol = np.linalg.cholesky(0.5 * (m + m.T))[None]
        self.integ = Integrator(kind, self.scale if kind == 'diag' else self.chol)

    def sample(self, rs, C):
        return (self.sigma * rs.standard_normal((C, self.sigma.size))).dot(self.R.T)

    def standardise(self, x):
        return np.asarray(x, dtype=f64).dot(self.R) / self.sigma

    def grad(self, q):
        return q / (self.sigma * self.sigma) if self.kind != 'dense' else q.dot(self.precision)

    def logp(self, q):
        return -0.5 * np.sum(q * self.grad(q), axis=1)


def stationarity_checks(case, x, alpha):
    import stationarity as S
    from scipy import stats
    z = case.standardise(x)
    return [S.pooled_chi2(z, alpha), S.pooled_mean(z, alpha), S.dkw(z, stats.norm.cdf, alpha, 'DKW against Phi')]


def stationarity_alpha():
    import stationarity as S
    return S.ALPHA / (3 * len(STATIONARITY))        # three statistics per metric, Bonferroni


def run_stationarity(kind, seed=None, mutant=None, C=STATIONARITY_C, n=STATIONARITY_N, md=STATIONARITY_MD):
    """The host sampler from exact draws; returns (case, final states, tree)."""
    cfg = STATIONARITY[kind]
    case = Case(kind)
    rs = np.random.RandomState(cfg['seed'] if seed is None else seed)
    x = case.sample(rs, C)
    s = NUTS(case.logp, case.grad, x, cfg['eps'], md, case.integ, mutant=mutant)
    for _ in range(n):
        x = s.sample(rs.standard_normal(x.shape), rs.uniform(size=(C, n_uniforms(md))))
    return case, x, s.tree


# ---------------------------------------------------------------------------
# the warm-up experiment: dense windowed warm-up around the restated sampler
# ---------------------------------------------------------------------------
WARMUP = dict(C=16, n_warmup=300, n_keep=200, timestep=0.5, max_depth=7)


def warmup_experiment(seed, C=WARMUP['C'], n_warmup=WARMUP['n_warmup'], n_keep=WARMUP['n_keep'],
                      timestep=WARMUP['timestep'], max_depth=WARMUP['max_depth']):
    """``warmup(NUTSSampler, 300, dense=True)`` on the rotated 8-dimensional Gaussian of
    ``dense_metric_ref`` (sigma 1 ... 100), 16 chains from 3 sigma out, then 200 kept draws.
    Returns (max split-R^, divergences after warm-up, frozen steps, kept draws)."""
    import dense_metric_ref as DM
    import metric_ref as MR
    S_, P, Ls = DM.rotated_target()
    D = S_.shape[0]
    rs = np.random.RandomState(seed)
    start = 3.0 * rs.standard_normal((C, D)) @ Ls.T
    target = DM.CorrelatedGaussTarget(P)
    integ = Integrator('dense', np.eye(D)[None])
    s = NUTS(target.log_prob, target.gradient, start, timestep, max_depth, integ, adaption_limit=n_warmup + 1)
    windows = MR.window_schedule(n_warmup)
    mom = DM.CoMoments(1)
    draw = lambda: (rs.standard_normal((C, D)), rs.uniform(size=(C, n_uniforms(max_depth))))
    for t in range(n_warmup):
        x = s.sample(*draw())
        for a, b in windows:
            if a <= t < b:
                mom.add(x, first=t == a)
                if t == b - 1:
                    s.da.restart()
                    integ.param = DM.factor(mom.s1, mom.s2, mom.n, C, True, integ.param)[0]
    div0 = int(s.tree.n_divergent.sum())
    kept = np.empty((n_keep, C, D))
    for t in range(n_keep):
        kept[t] = s.sample(*draw())
    return MR.max_split_rhat(kept), int(s.tree.n_divergent.sum()) - div0, s.eps.copy(), kept
