"""The arithmetic contract of the chain-resident kernels, restated on the host so that a
device result can be compared BIT FOR BIT (tests/test_gpu_chain_contract.py):

    linear_chain_kernel    csrc/linear_chain_kernel.hpp   layout 'linear'
    poly_chain_kernel      csrc/poly_chain_kernel.hpp     layout 'poly'
    hmc_poly_small_kernel  csrc/hmc_poly.hip              layout 'lane'

Written from the contracts in those headers, not from the kernel bodies; held on its own to
exact arithmetic and to the derived force bound by tests/test_chain_contract.py.  numpy,
vectorised over chains and lane slots: the Python loops run over rounds, coefficients and
leapfrog steps only.  Every order below is a function of (K, N) alone.

tree      numpy's pairwise rule: a leaf has at most 128 elements, a longer
          vector splits at n/2 rounded down to a multiple of 8, a leaf is summed with 8 strided
          accumulators ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) and its tail in order, fewer than 8
          elements in order from -0.0, the whole from the identity +0.0.  H is the height; a
          leaf above depth H is reached by 2**(H - depth) paths, the lowest is canonical.
lanes     slot = 8 path + j owns elements off + 8 t + j of its path's leaf, t = 0, 1, ...
          ("rounds"); a redundant path's slots contribute +0.0 to the force.
mock      linear: v = A[0][n] theta[0], v = fma(A[k][n], theta[k], v), k = 1 .. K-1: one chain,
          the same in the energy and in the force, in both modes.
          polynomial: unfused Horner (numpy's polyval) in the energy, FMA Horner in the force.
chi^2     np.sum((mock - ys)**2) in the tree above.
force     per slot g[k] = fma(c_k, (v - y) tau, g[k]) over the slot's rounds from +0.0, with
          c_k = A[k][n] (linear) or the running power pw = pw x from 1.0 (polynomial); then
          xor 1, 2, 4 over a leaf's 8 slots and xor 8, 16, 32 over the paths.
          Layout 'lane': one sequential FMA sum per g[k] over n = 0 .. N-1.
energy    prior and kinetic energy in np.sum's order over K; the log-prob terms added in the
          order pre, prior (if first), likelihood, prior (if last), post;
          lik = -0.5 chi^2 tau + (N 0.5) log tau.
leapfrog  p - dt g and q + p dt, unfused (EXACT) or one fma each (FMA); half kicks 0.5 dt.

``log tau`` is an INPUT: the device library's log is within one ulp of the correctly rounded
value, so a caller passes candidates ``[M x C]`` (:func:`log_candidates`) and
every energy and flag comes back with that leading axis.

``inject`` switches ONE deliberate departure into the force (tests only): 'swap_levels',
'redundant_weight', 'unfused_mock', 'reverse_rounds', 'drop_bit'."""
import numpy as np

from oracle import c_oracle

fma = c_oracle.fma
PW_BLOCK = 128
INJECTIONS = ('swap_levels', 'redundant_weight', 'unfused_mock', 'reverse_rounds', 'drop_bit')
TIE_MARGIN = 8 * 2.0 ** -52
MAX_HEIGHT = 3                # a chain's lane group is at most one wave: 8 paths of 8 accumulators


# ---------------------------------------------------------------------------
# the tree
# ---------------------------------------------------------------------------
def _split(n, off=0):
    """Nested pairs down to leaves ``(off, len)``."""
    if n <= PW_BLOCK:
        return (off, n)
    n2 = n // 2
    n2 -= n2 % 8
    return [_split(n2, off), _split(n - n2, off + n2)]


def _height(t):
    return 0 if isinstance(t, tuple) else 1 + max(_height(t[0]), _height(t[1]))


def tree_height(N):
    return _height(_split(N))


def leaves(N):
    """``(H, [(off, len, depth, canonical)] for path 0 .. 2**H - 1)``; a path's bit H-1 is
    the split at the root, 0 the left half."""
    t = _split(N)
    H = _height(t)
    out = []
    for path in range(1 << H):
        node, depth = t, 0
        while not isinstance(node, tuple):
            node = node[(path >> (H - 1 - depth)) & 1]
            depth += 1
        out.append((node[0], node[1], depth, int(path & ((1 << (H - depth)) - 1) == 0)))
    return H, out


def leaf_sum(x):
    """A leaf (last axis, at most 128 long) in numpy's order."""
    n = x.shape[-1]
    if n < 8:
        res = np.full(x.shape[:-1], -0.0)
        for i in range(n):
            res = res + x[..., i]
        return res
    r = x[..., :8]
    n8 = n - n % 8
    for i in range(8, n8, 8):
        r = r + x[..., i:i + 8]
    res = ((r[..., 0] + r[..., 1]) + (r[..., 2] + r[..., 3])) + ((r[..., 4] + r[..., 5]) + (r[..., 6] + r[..., 7]))
    for i in range(n8, n):
        res = res + x[..., i]
    return res


def np_sum(x):
    """np.sum over the last axis (at most 8192 long: one buffer of numpy's reduction)."""
    def walk(t):
        if isinstance(t, tuple):
            return leaf_sum(x[..., t[0]:t[0] + t[1]])
        return walk(t[0]) + walk(t[1])
    return 0.0 + walk(_split(x.shape[-1]))


class Lanes(object):
    """The lane slots of a chain for N data points: ``idx`` [TC x G] the datum of (round,
    slot) or -1, ``canon`` [G]."""

    def __init__(self, N):
        self.N = N
        self.H, lv = leaves(N)
        self.G = 8 << self.H
        self.TC = max(1, max((ln + 7) // 8 for _, ln, _, _ in lv))
        self.idx = np.full((self.TC, self.G), -1, dtype=np.int64)
        self.canon = np.zeros(self.G, dtype=bool)
        for path, (off, ln, _, canonical) in enumerate(lv):
            for j in range(8):
                e = np.arange(j, ln, 8)
                self.idx[:len(e), 8 * path + j] = off + e
                self.canon[8 * path + j] = bool(canonical)
        self.mask = self.idx >= 0

    def image(self, row):
        """``row`` [... x N] gathered to [... x TC x G], +0.0 where a slot has no datum."""
        row = np.asarray(row, dtype=np.float64)
        if self.N == 0:
            return np.zeros(row.shape[:-1] + self.idx.shape)
        return np.where(self.mask, row[..., np.maximum(self.idx, 0)], 0.0)

    def butterfly(self, g, swap=False):
        """[... x G] -> [...]: xor 1, 2, 4 inside a leaf, xor 8, 16, 32 across the paths."""
        P = 1 << self.H
        s = g.reshape(g.shape[:-1] + (P * 8,))
        lane = np.arange(P * 8)
        levels = [1, 2, 4, 8, 16, 32][:3 + self.H]
        if swap and self.H >= 2:
            levels[3], levels[4] = levels[4], levels[3]
        for m in levels:
            s = s + s[..., lane ^ m]
        return s[..., 0]


def _drop_bit0(a):
    """``a`` with bit 0 of its first element that has it set cleared."""
    a = np.array(a, dtype=np.float64)
    bits = a.reshape(-1).view(np.uint64)
    hit = np.nonzero(bits & np.uint64(1))[0]
    if len(hit):
        bits[hit[0]] &= ~np.uint64(1)
    return a


# ---------------------------------------------------------------------------
# the three layouts
# ---------------------------------------------------------------------------
class Contract(object):
    """One posterior under one layout.  ``design``: A [K x N] for 'linear', the abscissae
    [N] (and ``K``) for 'poly' and 'lane'.  ``prior`` = (means [K], vars [K], first) or None."""

    def __init__(self, layout, design, ys, K=None, prior=None, fused=False, inject=None):
        assert layout in ('linear', 'poly', 'lane') and inject in (None,) + INJECTIONS
        self.layout, self.fused, self.inject = layout, bool(fused), inject
        self.ys = np.asarray(ys, dtype=np.float64)
        self.N = len(self.ys)
        self.D = np.asarray(design, dtype=np.float64)
        self.K = self.D.shape[0] if layout == 'linear' else int(K)
        self.prior = prior
        self.lanes = Lanes(self.N)
        # what the force reads
        F = _drop_bit0(self.D[-1:] if layout == 'linear' else self.D) if inject == 'drop_bit' else None
        if layout == 'linear':
            DF = self.D if F is None else np.vstack([self.D[:-1], F])
            self.col = self.lanes.image(DF)                                   # [K x TC x G]
        else:
            self.xf = self.D if F is None else F
            self.ximg = self.lanes.image(self.xf)                             # [TC x G]
        self.yimg = self.lanes.image(self.ys)
        w = 2.0 ** -40 if inject == 'redundant_weight' else 0.0
        self.weight = np.where(self.lanes.canon, 1.0, w)                      # [G]

    # ---- energy -------------------------------------------------------------
    def mock(self, th):
        """[C x N]: the mock data of the energy."""
        C = th.shape[0]
        if self.layout == 'linear':
            v = self.D[0] * th[:, :1]
            for k in range(1, self.K):
                v = fma(self.D[k], th[:, k:k + 1], v)
            return v
        x = self.D[None, :]
        v = th[:, self.K - 1:self.K] + x * 0.0                # polyval: Horner, unfused
        for k in range(self.K - 2, -1, -1):
            v = th[:, k:k + 1] + v * x
        return np.broadcast_to(v, (C, self.N))

    def chi2(self, th):
        with np.errstate(all='ignore'):
            return 1.0 * np_sum((self.mock(th) - self.ys) ** 2)

    def log_prob(self, th, chi2, tau, logtau, pre=None, post=None):
        lik = -0.5 * chi2 * tau + float(self.N) * 0.5 * logtau
        terms = [] if pre is None else [pre]
        if self.prior is not None:
            mu, var, first = self.prior
            d = th - mu
            pri = -0.5 * np_sum(d * d / var)
            terms += [pri, lik] if first else [lik, pri]
        else:
            terms.append(lik)
        if post is not None:
            terms.append(post)
        total = terms[0]
        for t in terms[1:]:
            total = total + t
        return total

    def energy(self, th, p, chi2, tau, logtau, pre=None, post=None):
        with np.errstate(all='ignore'):
            return -self.log_prob(th, chi2, tau, logtau, pre, post) + 0.5 * np_sum(p * p)

    # ---- force --------------------------------------------------------------
    def _force_mock(self, th, img):
        """The mock data of the force on a data image ([TC x G], or [N] for 'lane')."""
        e = (slice(None),) + (None,) * (img.ndim if self.layout != 'linear' else img.ndim - 1)
        unfused = self.inject == 'unfused_mock'
        if self.layout == 'linear':
            v = img[0] * th[:, 0][e]
            for k in range(1, self.K):
                v = v + img[k] * th[:, k][e] if unfused else fma(img[k], th[:, k][e], v)
            return v
        v = np.broadcast_to(th[:, self.K - 1][e], (th.shape[0],) + img.shape)
        for k in range(self.K - 2, -1, -1):
            v = v * img + th[:, k][e] if unfused else fma(v, img, th[:, k][e])
        return v

    def force(self, th, tau):
        """[C x K]: the likelihood force at precision ``tau`` [C]."""
        with np.errstate(all='ignore'):
            return self._force(np.asarray(th, dtype=np.float64), np.asarray(tau, dtype=np.float64))

    def _force(self, th, tau):
        C, K = th.shape[0], self.K
        if self.layout == 'lane':
            x = self.xf
            r = (self._force_mock(th, x) - self.ys) * tau[:, None]            # [C x N]
            g = np.zeros((C, K))
            order = range(self.N - 1, -1, -1) if self.inject == 'reverse_rounds' else range(self.N)
            pw = np.ones((K, self.N))
            for k in range(1, K):
                pw[k] = pw[k - 1] * x
            for n in order:
                g = fma(pw[:, n], r[:, n:n + 1], g)
            return g
        L = self.lanes
        if self.layout == 'linear':
            col = self.col
            v = self._force_mock(th, col)
        else:
            col = np.ones((K,) + self.ximg.shape)
            for k in range(1, K):
                col[k] = col[k - 1] * self.ximg
            v = self._force_mock(th, self.ximg)
        r = (v - self.yimg) * (tau[:, None] * self.weight)[:, None, :]        # [C x TC x G]
        g = np.zeros((C, K, L.G))
        order = range(L.TC - 1, -1, -1) if self.inject == 'reverse_rounds' else range(L.TC)
        for t in order:
            g = np.where(L.mask[t], fma(col[None, :, t, :], r[:, None, t, :], g), g)
        return L.butterfly(g, swap=self.inject == 'swap_levels')

    # ---- moves ----------------------------------------------------------------
    def leapfrog(self, th, p, tau, dt, L):
        """hmc.py:116-123: half kick, (L - 1) x [drift, kick], drift, half kick; dt [C]."""
        th, p = np.array(th, dtype=np.float64), np.array(p, dtype=np.float64)
        dt = np.broadcast_to(np.asarray(dt, dtype=np.float64), (th.shape[0],))[:, None]
        tau = np.broadcast_to(np.asarray(tau, dtype=np.float64), (th.shape[0],))
        hdt = 0.5 * dt
        with np.errstate(all='ignore'):
            for l in range(L + 1):
                g = self._force(th, tau)
                kdt = hdt if l in (0, L) else dt
                p = fma(-kdt, g, p) if self.fused else p - kdt * g
                if l < L:
                    th = fma(p, dt, th) if self.fused else th + p * dt
        return th, p

    def hmc(self, th, p0, u, tau, logtau, dt, L, pre=None, post=None, chi2=None):
        """One transition.  ``logtau`` [C] or [M x C]; the energies, the flags and ``tie_free``
        carry its leading axis.  Returns dict(prop, p, chi2, chi2_new, e_before, e_after, acc,
        tie_free)."""
        th = np.asarray(th, dtype=np.float64)
        tau = np.broadcast_to(np.asarray(tau, dtype=np.float64), (th.shape[0],))
        chi2 = self.chi2(th) if chi2 is None else chi2
        eb = self.energy(th, p0, chi2, tau, logtau, pre, post)
        prop, p = self.leapfrog(th, p0, tau, dt, L)
        chi2_new = self.chi2(prop)
        ea = self.energy(prop, p, chi2_new, tau, logtau, pre, post)
        with np.errstate(all='ignore'):
            e = np.exp(np.clip(-(ea - eb), -308.0, 709.0))           # hmc.py:151, csb's clipped exp
        return dict(prop=prop, p=p, chi2=chi2, chi2_new=chi2_new, e_before=eb, e_after=ea, acc=u < e,
                    tie_free=tie_free(u, e))

    def rwmc(self, th, step, u, tau, logtau, pre=None, post=None, chi2=None):
        """samplers.py:78-92: proposal theta + step, ``u < np.exp(lp_new - lp_old)``."""
        th = np.asarray(th, dtype=np.float64)
        chi2 = self.chi2(th) if chi2 is None else chi2
        prop = th + step
        chi2_new = self.chi2(prop)
        with np.errstate(all='ignore'):
            lp_old = self.log_prob(th, chi2, tau, logtau, pre, post)
            lp_new = self.log_prob(prop, chi2_new, tau, logtau, pre, post)
            e = np.exp(lp_new - lp_old)
        return dict(prop=prop, chi2=chi2, chi2_new=chi2_new, acc=u < e, tie_free=tie_free(u, e))


def tie_free(u, e):
    """Is ``u`` outside ``e (1 +- 8 2**-52)``: can an exponential off by a few ulp not change
    ``u < e``?  A NaN exponential rejects whatever its last bits."""
    with np.errstate(all='ignore'):
        return np.isnan(e) | np.isinf(e) | (np.abs(u - e) > TIE_MARGIN * e)


def log_candidates(tau):
    """[3 x C]: the correctly rounded ``log tau`` (mpmath) and its two neighbours; at
    ``tau == 1`` all three are 0.0."""
    import mpmath as mp
    tau = np.atleast_1d(np.asarray(tau, dtype=np.float64))
    with mp.workprec(200):
        mid = np.array([float(mp.log(mp.mpf(float(t)))) if t > 0 else np.nan for t in tau])
    out = np.stack([mid, np.nextafter(mid, -np.inf), np.nextafter(mid, np.inf)])
    out[:, tau == 1.0] = 0.0
    return out


def gibbs(con, th, tau, n, move, p0, u, g, L=1, dt=None, n_adapt=0, uprate=1.05, downrate=0.95,
          gp_where=0, gp_shape=1.0, gp_rate=0.0, gamma_rate=0.0, keep_tau=False):
    """``n`` sweeps of gibbs.py:146-149 with supplied draws ``p0`` [n x C x K], ``u``, ``g``
    [n x C].  Every sweep is evaluated under the three candidates of ``log tau``; the state
    follows candidate 0's flag, and ``tie_free`` / ``flags_agree`` say whether that choice is
    immaterial.  Returns dict(theta [n x C x K], tau [n x C], acc [n x C], e_before, e_after
    [n x 3 x C], tie_free, flags_agree, n_accepted [C], dt [C])."""
    th = np.array(th, dtype=np.float64)
    C = th.shape[0]
    tau = np.array(np.broadcast_to(tau, (C,)), dtype=np.float64)
    dt = None if dt is None else np.array(np.broadcast_to(dt, (C,)), dtype=np.float64)
    chi2 = con.chi2(th)
    rec = dict(theta=[], tau=[], acc=[], e_before=[], e_after=[])
    ok, agree = True, True
    nacc = np.zeros(C, dtype=np.int64)
    for i in range(n):
        lt = log_candidates(tau)
        with np.errstate(all='ignore'):
            gp = (gp_shape - 1.0) * lt - tau * gp_rate                         # priors.py:23-25
        pre, post = (gp if gp_where == 1 else None), (gp if gp_where == 2 else None)
        if move == 'hmc':
            t = con.hmc(th, p0[i], u[i], tau, lt, dt, L, pre, post, chi2=chi2)
            rec['e_before'].append(t['e_before'])
            rec['e_after'].append(t['e_after'])
        else:
            t = con.rwmc(th, p0[i], u[i], tau, lt, pre, post, chi2=chi2)
        ok = ok and bool(np.all(t['tie_free']))
        agree = agree and bool(np.all(t['acc'] == t['acc'][0]))
        acc = t['acc'][0]
        th = np.where(acc[:, None], t['prop'], th)
        chi2 = np.where(acc, t['chi2_new'], chi2)
        nacc += acc
        if move == 'hmc' and i < n_adapt:
            dt = np.where(acc, dt * uprate, dt * downrate)                     # hmc.py:188-191
        if not keep_tau:
            with np.errstate(all='ignore'):
                lp1 = -0.5 * chi2 * 1.0 + float(con.N) * 0.5 * 0.0             # log_prob at tau = 1
                tau = g[i] / (-lp1 + gamma_rate)                               # samplers.py:34-49
        rec['theta'].append(th.copy())
        rec['tau'].append(tau.copy())
        rec['acc'].append(acc)
    out = {k: np.array(v) for k, v in rec.items() if v}
    out.update(tie_free=ok, flags_agree=agree, n_accepted=nacc, dt=dt)
    return out


# ---------------------------------------------------------------------------
# the cases of tests/test_gpu_chain_contract.py (shared with the CPU check of their accept
# tests, tests/test_chain_contract.py): the smallest shapes at which each mechanism runs
# ---------------------------------------------------------------------------
N_LIST = (0, 1, 7, 8, 9, 17, 25, 37, 127, 128, 129, 136, 257, 264, 513, 920, 1023, 1024)
K_LINEAR = (1, 3, 4, 5, 8, 9, 12, 13, 16)       # every KMAX, both interleaves, both branches of np_sum_k
K_POLY = (1, 4, 5, 8, 9, 16)
CHAINS = (1, 5, 300)                            # a ragged last wave for every group width; several workgroups


def ragged(N):
    H, lv = leaves(N)
    return any(depth < H for _, _, depth, _ in lv)


def shapes(ks, n_max=1024):
    """(K, N) round-robin over N_LIST; every K also meets N = 1024 and one ragged N that the
    kernels cover (N = 1023 is ragged but four levels deep: its cases assert that it is declined)."""
    ns = [N for N in N_LIST if N <= n_max]
    out = [(ks[i % len(ks)], N) for i, N in enumerate(ns)]
    rag = [N for N in ns if ragged(N) and tree_height(N) <= MAX_HEIGHT]
    for i, K in enumerate(ks):
        out += [(K, ns[-1])] + ([(K, rag[i % len(rag)])] if rag else [])
    return sorted(set(out), key=lambda s: (s[1], s[0]))


LINEAR_SHAPES = shapes(K_LINEAR)
POLY_SHAPES = shapes(K_POLY)
LANE_SHAPES = shapes(K_POLY, 128)


def stable_dt(A, tau_max, safety=0.45):
    """A leapfrog step inside the stability limit 2 / sqrt(lambda_max(tau A A^T)); 0.3 without data."""
    lam = np.linalg.eigvalsh(A.dot(A.T)).max() * float(tau_max) if A.shape[1] else 0.0
    return safety * 2.0 / np.sqrt(lam) if lam > 0 else 0.3


def data(layout, K, N, C, seed):
    """``(design, A, ys, theta [C x K], tau [C])``: data near a truth, chains around it; ``A``
    is the design matrix [K x N] of either model."""
    rs = np.random.RandomState(seed)
    if layout == 'linear':
        design = A = rs.standard_normal((K, N))
        truth = rs.standard_normal(K)
    else:
        design = rs.uniform(-1.2, 1.2, size=N)             # x**15 stays finite
        A = np.vstack([design ** k for k in range(K)])
        truth = rs.standard_normal(K) / (1.0 + np.arange(K))
    ys = truth.dot(A) + 0.3 * rs.standard_normal(N)
    theta = truth + 0.2 * rs.standard_normal((C, K)) / (1.0 + np.arange(K) if layout != 'linear' else 1.0)
    return design, A, ys, theta, rs.uniform(0.5, 4.0, size=C)


def hmc_case(layout, i, seed=0):
    """Case ``i`` of a layout's single-transition test: settings, inputs and draws."""
    K, N = {'linear': LINEAR_SHAPES, 'poly': POLY_SHAPES, 'lane': LANE_SHAPES}[layout][i]
    C = 300 if (K, N) == (16, 1024) else CHAINS[i % 3]
    c = dict(layout=layout, K=K, N=N, C=C, fused=bool(i & 1), L=(1, 2, 10)[(i + i // 3) % 3])
    design, A, ys, theta, tau = data(layout, K, N, C, 7919 * seed + 1000 * K + N + 7 * C)
    rs = np.random.RandomState(100 + i + 7919 * seed)
    per_tau, per_dt = bool((i >> 1) & 1), bool((i >> 2) & 1)
    dt0 = stable_dt(A, 4.0)
    c.update(design=design, A=A, ys=ys, theta=theta, p0=rs.standard_normal((C, K)), u=rs.uniform(size=C),
             tau=tau if per_tau else (1.0 if i % 4 == 0 else 2.5),
             dt=dt0 * rs.uniform(1.0, 2.15, size=C) if per_dt else 2.0 * dt0)    # up to 0.97 of the limit: rejections
    kind = (i // 3) % 3                                    # prior absent / first / last
    c['prior'] = None if kind == 0 else (0.1 * np.arange(K) - 0.2, 5.0 + 0.5 * np.arange(K), kind == 1)
    c['pre'] = rs.standard_normal(C) if i % 5 in (1, 2, 4) else None
    c['post'] = 3.0 * rs.standard_normal(C) if i % 7 in (0, 2, 3, 5) else None
    return c


def hmc_expect(c, inject=None):
    """The restated transition of a case under the three candidates of ``log tau``."""
    con = Contract(c['layout'], c['design'], c['ys'], K=c['K'], prior=c['prior'], fused=c['fused'], inject=inject)
    tau = np.broadcast_to(np.asarray(c['tau'], dtype=np.float64), (c['C'],))
    return con.hmc(c['theta'], c['p0'], c['u'], tau, log_candidates(tau), c['dt'], c['L'], c['pre'], c['post'])


GIBBS_SHAPES = {'linear': ((1, 1), (3, 37), (4, 129), (5, 257), (8, 513), (9, 136), (12, 1024), (13, 8), (16, 264)),
                'poly': ((1, 7), (4, 17), (5, 129), (8, 257), (9, 920), (16, 1024))}
GP_SHAPE, GP_RATE, GAMMA_RATE, UPRATE, DOWNRATE = 2.0, 0.2, 0.2, 1.07, 0.9


def gibbs_case(layout, move, i, seed=0):
    """Case ``i`` of a layout's Gibbs test: n in (1, 3) sweeps, supplied draws, the precision
    kept or drawn, adaption on for the first two sweeps of an HMC move."""
    K, N = GIBBS_SHAPES[layout][i]
    C = CHAINS[(i + (move == 'rwmc')) % 3]
    c = dict(layout=layout, move=move, K=K, N=N, C=C, n=(3, 1)[i % 2], keep_tau=i % 3 == 2, fused=bool(i & 2),
             L=(2, 10, 1)[i % 3], gp_where=i % 3, n_adapt=2 if move == 'hmc' else 0)
    design, A, ys, theta, tau = data(layout, K, N, C, 7919 * seed + 1000 * K + N + 7 * C + 3)
    rs = np.random.RandomState(200 + i + 7919 * seed)
    n = c['n']
    c.update(design=design, A=A, ys=ys, theta=theta, tau=tau, u=rs.uniform(size=(n, C)),
             gamma_shape=0.5 * N + 1.0, g=rs.gamma(0.5 * N + 1.0, size=(n, C)))
    if move == 'hmc':
        c.update(p0=rs.standard_normal((n, C, K)), dt=stable_dt(A, 4.0) * rs.uniform(1.0, 2.1, size=C))
    else:
        c.update(stepsize=0.3 / np.sqrt(max(N, 1)), dt=None)
        c['p0'] = rs.uniform(-c['stepsize'], c['stepsize'], size=(n, C, K))
    kind = (i // 2) % 3
    c['prior'] = None if kind == 0 else (0.1 * np.arange(K) - 0.2, 5.0 + 0.5 * np.arange(K), kind == 1)
    return c


def gibbs_expect(c):
    con = Contract(c['layout'], c['design'], c['ys'], K=c['K'], prior=c['prior'], fused=c['fused'])
    return gibbs(con, c['theta'], c['tau'], c['n'], c['move'], c['p0'], c['u'], c['g'], L=c['L'], dt=c['dt'],
                 n_adapt=c['n_adapt'], uprate=UPRATE, downrate=DOWNRATE, gp_where=c['gp_where'], gp_shape=GP_SHAPE,
                 gp_rate=GP_RATE, gamma_rate=GAMMA_RATE, keep_tau=c['keep_tau'])


def hmc_case_ids():
    return [(layout, i) for layout, sh in (('linear', LINEAR_SHAPES), ('poly', POLY_SHAPES), ('lane', LANE_SHAPES))
            for i in range(len(sh))]


def gibbs_case_ids():
    return [(layout, move, i) for layout in ('linear', 'poly') for move in ('hmc', 'rwmc')
            for i in range(len(GIBBS_SHAPES[layout]))]


# ---- the cross-checks and the non-finite cases: single transitions outside the lists above ----
CROSS_SHAPES = ((16, 17), (9, 129), (5, 513), (16, 1024))
ONE_COEFFICIENT_N = (7, 128, 257, 1024)
NON_FINITE_SHAPES = (('linear', 7, 37), ('linear', 16, 257), ('poly', 5, 17), ('poly', 9, 513), ('lane', 4, 20))


def cross_cases(K, N):
    """A polynomial case and the linear kernel's case on its design matrix (stored powers)."""
    c = hmc_case('poly', POLY_SHAPES.index((K, N)))
    return c, dict(c, layout='linear', design=c['A'])


def plain_case(layout, K, N, C, L, seed):
    """A transition with no prior and no constants, per-chain precision, one step size."""
    design, A, ys, theta, tau = data(layout, K, N, C, seed=seed)
    rs = np.random.RandomState(seed + 1)
    return dict(layout=layout, K=K, N=N, C=C, fused=False, L=L, design=design, A=A, ys=ys, theta=theta, tau=tau,
                p0=rs.standard_normal((C, K)), u=rs.uniform(size=C), dt=stable_dt(A, 4.0), prior=None, pre=None,
                post=None)


def one_coefficient_cases(N):
    """K = 1 under the polynomial group layout, the linear layout (A = ones) and, up to 128
    points, one lane per chain: the same inputs."""
    c = plain_case('poly', 1, N, 5 if N in (7, 257) else 300, 3, seed=N)
    out = [c, dict(c, layout='linear', design=c['A'])]
    return out + ([dict(c, layout='lane')] if N <= 128 else [])


def non_finite_case(layout, K, N):
    return plain_case(layout, K, N, 5, 4, seed=K * N)


def extra_hmc_cases():
    """Every single-transition case of the GPU file that is not in hmc_case_ids()."""
    out = [c for K, N in CROSS_SHAPES for c in cross_cases(K, N)]
    out += [c for N in ONE_COEFFICIENT_N for c in one_coefficient_cases(N)]
    return out + [non_finite_case(*s) for s in NON_FINITE_SHAPES]
