"""Host restatement (numpy) of ``csrc/smc.hip`` / ``binf_amd/samplers/smc.py``, written from
the contract in ``include/binf_hip.h``: the reweighting with its root search, systematic
resampling, the gather, and the whole tempered loop around a plain HMC mutation.  Nothing
here calls into the library.

THE SUM of a population's P terms (``block_sum``): thread j of 256 adds its terms j, j + 256,
... in ascending order onto 0.0; the 64 lanes of a wave join as a balanced tree over
neighbouring lanes; the four waves as ((w0 + w1) + w2) + w3.  The two sides differ only in
``exp`` / ``log`` (numpy's here, the device library's there, each within an ulp).
"""
import numpy as np

f64 = np.float64
THREADS = 256
OK, FINISHED, NO_FINITE, INVALID, STALLED = 0, 1, 2, 3, 4
PASS_THROUGH = (FINISHED, NO_FINITE, INVALID)
EPS = 2.0 ** -52


def block_sum(x):
    """THE SUM of a 1-D array of non-negative terms (zero padding adds exact zeros)."""
    P = x.shape[0]
    rows = (P + THREADS - 1) // THREADS
    full = np.zeros(rows * THREADS, dtype=f64)
    full[:P] = x
    a = full.reshape(rows, THREADS)
    lane = np.zeros(THREADS, dtype=f64)
    for i in range(rows):
        lane = lane + a[i]
    w = lane.reshape(4, 64)
    while w.shape[1] > 1:
        w = w[:, 0::2] + w[:, 1::2]
    w = w[:, 0]
    return ((w[0] + w[1]) + w[2]) + w[3]


def sum_depth(P):
    """Additions on the longest path of THE SUM."""
    return (P + THREADS - 1) // THREADS + 6 + 3


# ---------------------------------------------------------------------------
# the reweighting
# ---------------------------------------------------------------------------
def shifted(ll):
    """(m, e): the largest finite l and e_i = l_i - m, -inf where l_i is -inf or NaN."""
    ok = np.isfinite(ll)
    m = ll[ok].max()
    with np.errstate(invalid='ignore', over='ignore'):
        e = np.where(ok, ll - m, -np.inf)
    return m, e


def weights(e, d, exp=np.exp):
    with np.errstate(under='ignore', invalid='ignore', over='ignore'):
        return np.where(e > -np.inf, exp(f64(d) * np.where(e > -np.inf, e, 0.0)), 0.0)


def sums(e, d, exp=np.exp):
    """(w, S1, S2, ESS) at the step d."""
    w = weights(e, d, exp)
    s1, s2 = block_sum(w), block_sum(w * w)
    return w, s1, s2, (s1 * s1) / s2


def temper_at(ll, d, exp=np.exp, log=np.log):
    """dict(w, ess, log_z_inc, s1, s2) of one population at a GIVEN step d."""
    P = ll.shape[0]
    m, e = shifted(ll)
    w, s1, s2, ess = sums(e, d, exp)
    return dict(w=w, ess=ess, s1=s1, s2=s2, m=m, log_z_inc=f64(d) * m + (log(s1) - log(f64(P))))


def temper(ll, beta, rho, n_bisect=60, exp=np.exp, log=np.log):
    """One population: dict(delta, beta, w, log_z_inc, ess, n_invalid, status)."""
    P = ll.shape[0]
    beta = f64(beta)
    n_invalid = int(np.isnan(ll).sum())
    status = OK
    if not beta < 1.0:
        status = FINISHED
    elif np.any(ll == np.inf):
        status = INVALID
    elif not np.any(np.isfinite(ll)):
        status = NO_FINITE
    if status != OK:
        return dict(delta=f64(0.0), beta=beta, w=np.ones(P), log_z_inc=f64(0.0), ess=f64(P),
                    n_invalid=n_invalid, status=status)
    m, e = shifted(ll)
    need = f64(rho) * f64(P)
    hi0 = f64(1.0) - beta
    if sums(e, hi0, exp)[3] >= need:
        delta, beta_new = hi0, f64(1.0)
    else:
        lo, hi = f64(0.0), hi0
        for _ in range(n_bisect):
            mid = f64(0.5) * (lo + hi)
            if sums(e, mid, exp)[3] >= need:
                lo = mid
            else:
                hi = mid
        delta = lo
        if lo == 0.0:
            delta, status = hi, STALLED
        beta_new = beta + delta
    w, s1, s2, ess = sums(e, delta, exp)
    return dict(delta=delta, beta=beta_new, w=w, ess=ess, n_invalid=n_invalid, status=status,
                log_z_inc=delta * m + (log(s1) - log(f64(P))))


# ---------------------------------------------------------------------------
# systematic resampling
# ---------------------------------------------------------------------------
def prefix_sums(w):
    """cs [P] in the header's order: 256 contiguous segments of L = ceil(P / 256), a running
    sum in each, the segment totals added in ascending order, cs = E_j + r_i."""
    P = w.shape[0]
    L = (P + THREADS - 1) // THREADS
    full = np.zeros(THREADS * L, dtype=f64)
    full[:P] = w
    r = np.cumsum(full.reshape(THREADS, L), axis=1)         # sequential along a segment
    T = r[:, -1]
    E = np.concatenate([[0.0], np.cumsum(T)[:-1]])          # sequential over the segments
    return (E[:, None] + r).reshape(-1)[:P]


def targets(P, u, total):
    return ((np.arange(P, dtype=f64) + f64(u)) / f64(P)) * f64(total)


def resample(w, u, status=OK):
    """(ancestor [P] local indices, n_unique) of one population."""
    P = w.shape[0]
    ident = (np.arange(P, dtype=np.int64), P)
    if status in PASS_THROUGH or not (0.0 <= u < 1.0):
        return ident
    cs = prefix_sums(w)
    total = cs[-1]
    if not (0.0 < total < np.inf):
        return ident
    a = np.searchsorted(cs, targets(P, u, total), side='right').astype(np.int64)
    a[a >= P] = np.nonzero(w > 0.0)[0][-1]
    return a, int(np.unique(a).shape[0])


def resample_batch(w, u, P, status=None):
    """Every population of a [G * P] weight vector: (ancestor [C] global, n_unique [G])."""
    G = w.shape[0] // P
    anc, nu = np.empty(G * P, np.int64), np.empty(G, np.int64)
    for g in range(G):
        a, n = resample(w[g * P:(g + 1) * P], u[g], OK if status is None else int(status[g]))
        anc[g * P:(g + 1) * P] = g * P + a
        nu[g] = n
    return anc, nu


# ---------------------------------------------------------------------------
# bounds (derivations in the tests that use them)
# ---------------------------------------------------------------------------
def sum_bounds(P, s1, s2, sides=2):
    """(b1, b2): bounds on the error of S1 and S2 between ``sides`` evaluations that differ
    in exp alone (2: device against this file; 1: either against exact arithmetic).

    A weight w = exp(fl(d * e)) <= 1: one ulp of exp per side, and against exact arithmetic
    the roundings of e = l - m and of d * e move the exponent by |d e| 2^-52, the weight by
    |d e| exp(-|d e|) 2^-52 <= 2^-52 / e -- under 2 * 2^-52 absolute either way.  w * w <= 1:
    twice that relatively plus half an ulp of the product per side, under 5 * 2^-52.  THE SUM
    adds P such terms along paths of sum_depth(P) additions, each rounding a partial sum <=
    the total by half an ulp, on every side."""
    d = sum_depth(P) * 0.5 * EPS * max(sides, 2)
    return 2.0 * P * EPS + d * s1, 5.0 * P * EPS + d * s2


def ess_bound(P, s1, s2, sides=2):
    """ESS = (S1 * S1) / S2: twice the relative error of S1, once that of S2, and the two
    roundings of the quotient on each side, times the value (1.01: second-order terms)."""
    b1, b2 = sum_bounds(P, s1, s2, sides)
    return 1.01 * (s1 * s1 / s2) * (2.0 * b1 / s1 + b2 / s2 + 2.0 * EPS)


def log_z_bound(P, s1, s2, value, sides=2):
    """log_z_inc = d * m + (log S1 - log P): d * m is the same product on both sides (against
    exact arithmetic: half an ulp of it, inside |value| + the logs below); log S1 moves by b1 /
    S1 and an ulp of log; log P by an ulp per side; the difference and the final sum round by
    half an ulp of their values per side."""
    b1, _ = sum_bounds(P, s1, s2, sides)
    ls, lp = abs(np.log(s1)), np.log(f64(P))
    return 1.01 * b1 / s1 + EPS * (2.0 * ls + 2.0 * lp + (ls + lp) + 2.0 * abs(value) + 1e-300)


def slope_bound(P, e):
    """|d ESS / d delta| <= 2 P max|e|: d log S1 = <e>_w, d log S2 = 2 <e>_ww, both weighted
    means of e in [-max|e|, 0], and ESS <= P."""
    fin = e[e > -np.inf]
    return 2.0 * P * float(np.max(np.abs(fin)))


# ---------------------------------------------------------------------------
# exact arithmetic (mpmath, 100 digits)
# ---------------------------------------------------------------------------
def exact_ess(ll, d):
    """ESS at the step ``d`` (an mpf or a float) with every operation exact."""
    import mpmath
    mpmath.mp.dps = 100
    ok = np.isfinite(ll)
    m = mpmath.mpf(float(ll[ok].max()))
    d = mpmath.mpf(d)
    s1 = s2 = mpmath.mpf(0)
    for v in ll[ok]:
        w = mpmath.exp(d * (mpmath.mpf(float(v)) - m))
        s1 += w
        s2 += w * w
    return s1 * s1 / s2


# ---------------------------------------------------------------------------
# inputs and properties shared by the CPU and the GPU tests
# ---------------------------------------------------------------------------
PATTERNS = ('random', 'zeros_front', 'zeros_end', 'zero_runs', 'one_hot', 'subnormal')
U_EDGE = (0.0, 0.5, 1.0 - 2.0 ** -53)


def ll_sample(P, kind, seed):
    rs = np.random.RandomState(seed)
    ll = -0.5 * (rs.standard_normal((P, 4)) * 3.0 - 2.0) ** 2 @ np.ones(4) / 0.25
    if kind == 'holes' and P > 2:
        ll[1::5] = -np.inf
        ll[2::7] = np.nan
    return ll


def weight_pattern(P, kind, seed):
    rs = np.random.RandomState(seed)
    w = rs.uniform(0.05, 1.0, size=P) ** 3
    if kind == 'zeros_front':
        w[:max(1, P // 3)] = 0.0
        w[-1] = 0.7
    elif kind == 'zeros_end':
        w[P - max(1, P // 3):] = 0.0
        w[0] = 0.7
    elif kind == 'zero_runs':
        w[(np.arange(P) // 3) % 2 == 1] = 0.0
        w[0] = 0.3
    elif kind == 'one_hot':
        w[:] = 0.0
        w[(7 * P) // 11] = 0.625
    elif kind == 'subnormal':
        w = w * 1e-308 * 0.1                                 # 1e-313 .. 1e-309: far below 2.2e-308
    return w


def count_rule_holds(w, anc):
    """Every count in {floor, ceil} of P w_i / total, where that is no integer to 1e-9."""
    P = w.shape[0]
    n = P * w / w.sum()
    counts = np.bincount(anc, minlength=P)
    free = np.abs(n - np.round(n)) > 1e-9
    ok = (counts == np.floor(n)) | (counts == np.ceil(n))
    return bool(np.all(ok[free])) and bool(np.all(np.abs(counts[~free] - n[~free]) <= 1.0 + 1e-9))


def binomial_interval(n, f, alpha=1e-9):
    """[k_lo, k_hi] per entry of ``f``: the narrowest central interval of Binomial(n, f) that
    leaves at most ``alpha`` in each tail (exact pmf, summed from the tails)."""
    from math import lgamma
    k = np.arange(n + 1, dtype=f64)
    logc = np.array([lgamma(n + 1) - lgamma(i + 1) - lgamma(n - i + 1) for i in range(n + 1)])
    f = np.clip(np.asarray(f, dtype=f64), 0.0, 1.0)[:, None]
    with np.errstate(divide='ignore', invalid='ignore'):
        logp = logc[None, :] + np.where(k > 0, k * np.log(f), 0.0) + np.where(n - k > 0, (n - k) * np.log1p(-f), 0.0)
    pmf = np.exp(logp)
    lo = (np.cumsum(pmf, axis=1) <= alpha).sum(axis=1)                   # first k kept
    hi = n - (np.cumsum(pmf[:, ::-1], axis=1) <= alpha).sum(axis=1)      # last k kept
    return lo, hi


def mean_count_rule_holds(w, anc_rows):
    """``anc_rows`` [n x P]: the ancestors at n independent uniform u.  The number of draws in
    which particle i got ceil(P w_i / total) copies is Binomial(n, frac(P w_i / total))."""
    n, P = anc_rows.shape
    e = P * w / w.sum()
    counts = np.stack([np.bincount(a, minlength=P) for a in anc_rows])
    ups = (counts - np.floor(e)[None, :]).sum(axis=0)
    lo, hi = binomial_interval(n, e - np.floor(e))
    return bool(np.all((ups >= lo) & (ups <= hi)))


# ---------------------------------------------------------------------------
# the whole loop on the conjugate Gaussian of the end-to-end test
# ---------------------------------------------------------------------------
E2E = dict(D=4, prior_sd=3.0, noise_sd=0.5, y=2.0, G=16, P=256, rho=0.5, n_mutations=2, n_steps=8)


def e2e_analytic(D=E2E['D'], s0=E2E['prior_sd'], s=E2E['noise_sd'], y=E2E['y']):
    """log of the integral of N(x | 0, s0^2 I) N(y 1 | x, s^2 I) = log N(y 1 | 0, (s0^2 + s^2) I)."""
    v = s0 * s0 + s * s
    return D * (-0.5 * y * y / v - 0.5 * np.log(2.0 * np.pi * v))


def e2e_dt(beta, s0=E2E['prior_sd'], s=E2E['noise_sd']):
    return 0.5 / np.sqrt(1.0 / (s0 * s0) + beta / (s * s))


def e2e_loop(seed, control=False, P=E2E['P'], D=E2E['D'], rho=E2E['rho'], k=E2E['n_mutations'],
             L=E2E['n_steps'], s0=E2E['prior_sd'], s=E2E['noise_sd'], y=E2E['y'], max_stages=100):
    """One population through temper / resample / gather / k HMC transitions of L steps per
    stage: (log Z, stages, betas).  ``control``: the reweighting skipped -- no resampling,
    log_z_inc forced to delta * mean(l), the thermodynamic-integration integrand at the
    stage's start."""
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((P, D)) * s0

    def loglik(x):
        return -0.5 * ((x - y) ** 2).sum(1) / s ** 2 - 0.5 * D * np.log(2.0 * np.pi * s ** 2)
    beta, log_z, betas = f64(0.0), 0.0, []
    while beta < 1.0:
        assert len(betas) < max_stages
        l = loglik(x)
        t = temper(l, beta, rho)
        u = rs.uniform()
        if control:
            log_z += t['delta'] * l.mean()
        else:
            log_z += t['log_z_inc']
            x = x[resample(t['w'], u, t['status'])[0]]
        beta = t['beta']
        betas.append(float(beta))
        dt = e2e_dt(beta)

        def grad(q):
            return q / s0 ** 2 + beta * (q - y) / s ** 2

        def energy(q):
            return 0.5 * (q * q).sum(1) / s0 ** 2 + beta * 0.5 * ((q - y) ** 2).sum(1) / s ** 2
        for _ in range(k):
            p = rs.standard_normal(x.shape)
            q = x.copy()
            h0 = energy(q) + 0.5 * (p * p).sum(1)
            p = p - 0.5 * dt * grad(q)
            for i in range(L):
                q = q + dt * p
                p = p - (dt if i < L - 1 else 0.5 * dt) * grad(q)
            h1 = energy(q) + 0.5 * (p * p).sum(1)
            acc = rs.uniform(size=P) < np.exp(np.minimum(0.0, h0 - h1))
            x = np.where(acc[:, None], q, x)
    return log_z, len(betas), betas


_yardstick = {}
# e2e_yardstick(200) on the CPU: mean -9.0037, sd 0.16297, at most 6 stages; the control
# (control=True) -14.690 +- 0.243, at most 7 stages -- 5.70 below the analytic -8.98987
E2E_SD = 0.16297


def e2e_bound(sd=E2E_SD, G=E2E['G']):
    """5 sd / sqrt(G) for the mean of G populations + sd^2 / 2, the known bias of log Z (Z is
    unbiased, so E log Z = log Z - var / 2 to second order)."""
    return 5.0 * sd / np.sqrt(G) + 0.5 * sd * sd



def e2e_yardstick(n_seeds=200):
    """dict(mean, sd, stages_max, control_mean, control_sd) over ``n_seeds`` populations."""
    if n_seeds not in _yardstick:
        r = np.array([e2e_loop(i)[:2] for i in range(n_seeds)])
        c = np.array([e2e_loop(i, control=True)[:2] for i in range(n_seeds)])
        _yardstick[n_seeds] = dict(mean=r[:, 0].mean(), sd=r[:, 0].std(ddof=1), stages_max=int(r[:, 1].max()),
                                   control_mean=c[:, 0].mean(), control_sd=c[:, 0].std(ddof=1),
                                   control_stages_max=int(c[:, 1].max()))
    return _yardstick[n_seeds]
