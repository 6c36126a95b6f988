"""Host restatement (numpy) of ``csrc/free_energy.hip`` / ``binf_amd/free_energy.py``, written
from the contract in ``include/binf_hip.h``: the work row of a swap round, the selection of
a pair's rows and a group's ladders, the chunked sums in the library's order, the logistic,
the root bracket and its iteration.  Nothing here calls into the library.

Order of every sum (``block_reduce``): a chunk of ``chunk`` samples counted from the start of
the problem, positions past the end reading as -inf (the sample of weight 0); thread j of
256 adds samples j, j + 256, ... in order; the 64 lanes of a wave join as a balanced tree
over neighbouring lanes; the four waves as ((w0 + w1) + w2) + w3; chunks in ascending
order.  The two sides differ only in ``exp`` / ``log`` (numpy's here, the device library's
there, each within an ulp).
"""
import os
import re

import numpy as np

f64 = np.float64
THREADS = 256
OK, INVALID, NO_FINITE, EMPTY, NOT_CONVERGED, ONE_SIDED, NO_OVERLAP = 0, 1, 2, 3, 4, 5, 6
MAX_ITER = 2200


def header_chunk():
    """BINF_FE_CHUNK of include/binf_hip.h."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'binf_hip.h')
    return int(re.search(r'#define\s+BINF_FE_CHUNK\s+(\d+)', open(path).read()).group(1))


# ---------------------------------------------------------------------------
# the work row
# ---------------------------------------------------------------------------
def partner_or_minus_one(C, R, parity):
    """[C] int64: the other member of c's pair, -1 for an unpaired chain."""
    assert R >= 1 and C % R == 0 and parity in (0, 1)
    c = np.arange(C, dtype=np.int64)
    r = c % R
    low = (r >= parity) & ((r - parity) % 2 == 0) & (r + 1 < R)
    p = np.full(C, -1, dtype=np.int64)
    p[low] = c[low] + 1
    p[c[low] + 1] = c[low]
    return p


def work_row(lp_own, lp_sw, R, parity):
    """w[c] = lp_sw[c] - lp_own[partner(c)], NaN at unpaired chains."""
    C = lp_own.shape[0]
    p = partner_or_minus_one(C, R, parity)
    w = np.full(C, np.nan)
    paired = p >= 0
    with np.errstate(invalid='ignore'):
        w[paired] = lp_sw[paired] - lp_own[p[paired]]
    return w


# ---------------------------------------------------------------------------
# selection
# ---------------------------------------------------------------------------
def pair_rows(T, first_round, r):
    """Rows of a T-row record that hold the pair (r, r + 1): parity of the round == r & 1."""
    t = np.arange(T, dtype=np.int64)
    return t[((first_round + t) & 1) == (r & 1)]


def problem_samples(work, R, first_round, G, g, r):
    """(u, v): the samples of pair (r, r + 1) in group g, (row, ladder) order."""
    T, C = work.shape
    n_ladders = C // R
    assert C % R == 0 and G >= 1 and n_ladders % G == 0 and 0 <= r < R - 1
    Lg = n_ladders // G
    rows = pair_rows(T, first_round, r)
    cols = (g * Lg + np.arange(Lg, dtype=np.int64)) * R + r
    sub = work[np.ix_(rows, cols)] if rows.size and cols.size else np.zeros((0, 0))
    sub_v = work[np.ix_(rows, cols + 1)] if rows.size and cols.size else np.zeros((0, 0))
    return np.ascontiguousarray(sub).reshape(-1), np.ascontiguousarray(sub_v).reshape(-1)


# ---------------------------------------------------------------------------
# sums in the library's order
# ---------------------------------------------------------------------------
def block_reduce(x, chunk, op=np.add):
    """One chunk (``x`` holds ``chunk`` values, padded by the caller) -> one value."""
    a = x.reshape(chunk // THREADS, THREADS)
    lane = a[0].copy()
    for i in range(1, a.shape[0]):
        lane = op(lane, a[i])
    w = lane.reshape(4, 64)
    while w.shape[1] > 1:
        w = op(w[:, 0::2], w[:, 1::2])
    w = w[:, 0]
    return op(op(op(w[0], w[1]), w[2]), w[3])


def chunks_of(x, chunk, pad):
    n = x.shape[0]
    nch = (n + chunk - 1) // chunk
    full = np.full(nch * chunk, pad, dtype=f64)
    full[:n] = x
    return full.reshape(nch, chunk)


def logistic(z):
    """(sigma, sigma (1 - sigma)) of the header's fixed form."""
    with np.errstate(over='ignore', under='ignore'):
        t = np.exp(-np.abs(z))
        d = 1.0 + t
        return np.where(z >= 0.0, 1.0 / d, t / d), t / (d * d)


def pass1(x, chunk):
    """(M, total, min over finite, n_invalid) of one direction: chunk maxima m_c, chunk sums
    S_c = sum exp(x - m_c), total = sum_c S_c exp(m_c - M) in ascending order."""
    bad = ~(x <= np.finfo(f64).max)                  # NaN and +inf
    x = np.where(bad, -np.inf, x)
    M, mn, tot = -np.inf, np.inf, 0.0
    parts = []
    for row in chunks_of(x, chunk, -np.inf):
        m = block_reduce(row, chunk, np.maximum)
        low = block_reduce(np.where(row > -np.inf, row, np.inf), chunk, np.minimum)
        s = 0.0
        if m > -np.inf:
            with np.errstate(under='ignore'):
                s = block_reduce(np.exp(row - m), chunk)
        parts.append((m, s))
        M, mn = max(M, m), min(mn, low)
    for m, s in parts:
        if m > -np.inf:
            tot = tot + s * np.exp(m - M)
    return M, tot, mn, int(bad.sum())


def g_sums(u, v, D, chunk):
    """(A, B, S): sum sigma(u - D), sum sigma(v + D), sum of sigma (1 - sigma) of both."""
    A = B = S = 0.0
    for ru, rv in zip(chunks_of(u, chunk, -np.inf), chunks_of(v, chunk, -np.inf)):
        su, du = logistic(ru - D)
        sv, dv = logistic(rv + D)
        a = block_reduce(su, chunk)
        b = block_reduce(sv, chunk)
        # per thread: s = (s + d_u) + d_v, sample after sample
        lanes = np.zeros(THREADS)
        du, dv = du.reshape(-1, THREADS), dv.reshape(-1, THREADS)
        for i in range(du.shape[0]):
            lanes = (lanes + du[i]) + dv[i]
        s = block_reduce(np.concatenate([lanes, np.zeros(chunk - THREADS)]), chunk)
        A, B, S = A + a, B + b, S + s
    return A, B, S


def solve(u, v, chunk):
    """One problem: dict(delta, delta_forward, delta_reverse, info, n, n_invalid, status,
    iterations)."""
    n = int(u.shape[0])
    out = dict(delta=np.nan, delta_forward=np.nan, delta_reverse=np.nan, info=np.nan, n=n,
               n_invalid=0, status=EMPTY, iterations=0)
    if n == 0:
        return out
    Mu, tu, mnu, badu = pass1(u, chunk)
    Mv, tv, mnv, badv = pass1(v, chunk)
    out['n_invalid'] = badu + badv
    if badu + badv:
        out['status'] = INVALID
        return out
    logn = np.log(f64(n))
    fwd = (Mu + np.log(tu)) - logn if Mu > -np.inf else -np.inf
    rev = -((Mv + np.log(tv)) - logn) if Mv > -np.inf else np.inf
    out['delta_forward'], out['delta_reverse'] = fwd, rev
    if Mu == -np.inf and Mv == -np.inf:
        out['status'] = NO_FINITE
        return out
    if Mu == -np.inf or Mv == -np.inf:
        out.update(status=ONE_SIDED, delta=-np.inf if Mu == -np.inf else np.inf, info=0.0)
        return out
    lo, hi = min(mnu, -Mv), max(Mu, -mnv)
    D = 0.5 * fwd + 0.5 * rev
    if not (lo <= D <= hi):
        D = 0.5 * lo + 0.5 * hi
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        dxold = f64(hi) - f64(lo)
        for it in range(1, MAX_ITER + 1):
            A, B, S = g_sums(u, v, D, chunk)
            g = B - A
            out.update(delta=D, info=S, iterations=it, status=OK if S > 0.0 else NO_OVERLAP)
            if g == 0.0:
                return out
            if g < 0.0:
                lo = D
            else:
                hi = D
            step = f64(g) / f64(S)
            cand = D - step
            if lo < cand < hi and abs(2.0 * g) <= abs(dxold * S):
                Dn, dx = cand, abs(step)
            else:
                dx = 0.5 * hi - 0.5 * lo
                Dn = min(lo + dx, hi)
            if Dn == D:
                return out
            D, dxold = Dn, dx
    out['status'] = NOT_CONVERGED
    return out


def bar(work, R, first_round=0, G=1, chunk=None):
    """Every problem of a record: dict of [G x (R - 1)] arrays (floats f64, n / n_invalid
    int64, status int32)."""
    chunk = header_chunk() if chunk is None else chunk
    shape = (G, max(R - 1, 0))
    res = dict((k, np.full(shape, np.nan)) for k in ('delta', 'delta_forward', 'delta_reverse', 'info'))
    res.update(n=np.zeros(shape, np.int64), n_invalid=np.zeros(shape, np.int64),
               status=np.zeros(shape, np.int32), iterations=np.zeros(shape, np.int64))
    for g in range(G):
        for r in range(R - 1):
            u, v = problem_samples(work, R, first_round, G, g, r)
            one = solve(u, v, chunk)
            for k, val in one.items():
                res[k][g, r] = val
    return res


# ---------------------------------------------------------------------------
# bounds (derivations in the tests that use them)
# ---------------------------------------------------------------------------
EPS = 2.0 ** -52


def g_error_bound(n, chunk):
    """Bound on the error of an evaluation of g = B - A over n samples per direction, either
    side: each of the 2 n terms in [0, 1] carries the ulps of one exp, one add, one divide
    (<= 3 EPS relative, EPS absolute since a term <= 1 -- 3 EPS in all); the sum of n terms
    <= 1 in the fixed order has depth chunk / 256 + 6 + 3 + n / chunk additions, each
    rounding a partial sum <= n."""
    depth = chunk // THREADS + 9 + (n + chunk - 1) // chunk
    return 2.0 * n * 3.0 * EPS + 2.0 * depth * n * EPS + EPS * n


def average_bound(n, value):
    """Bound on the error of an exponential average (M + log(total)) - log n of n samples,
    against exact arithmetic or between the two sides: 16 * 2^-52 * (1 + |value| + log n) +
    n * 2^-52.
      * A term exp(x - m), d = m - x >= 0: the rounding of x - m (d * 2^-53 absolute) and one
        ulp of exp make it off by (1 + d / 2) * 2^-52 relative, i.e. by (1 + d / 2) e^-d *
        2^-52 <= 2^-52 absolute.  The n terms and the chunk factors exp(m_c - M) <= 1 move
        total by under n * 2^-52 absolute, and total >= 1 (the largest sample's term is 1):
        log(total) moves by n * 2^-52 at the most.
      * The additions (depth chunk / 256 + 9 + n_chunks <= 28 for up to three chunks, half
        an ulp of total each) move log(total) by 14 * 2^-52; log(total), log n (one ulp each)
        and the two roundings of M + . - . add under 3 * 2^-52 * (1 + |value| + log n).
        14 + 3 (1 + |value| + log n) <= 16 (1 + |value| + log n) whenever log n >= 0.1."""
    return 16.0 * EPS * (1.0 + abs(value) + np.log(n)) + n * EPS


def info_bound(n, S, delta_error):
    """Bound on the error of S = sum sigma (1 - sigma): 2 n terms <= 1/4, each within 4 ulp
    (one exp, 1 + t, its square, one divide: 4 * 2^-52 * 1/4 absolute, doubled for the
    rounding of z and the additions), plus |dS/dD| <= S times the error of delta."""
    return n * 8.0 * EPS + delta_error * S


def delta_bound(n, S, delta, chunk):
    """|delta - root| <= e_g / S + what one double's spacing at delta allows (the iteration
    stops when the step falls under half an ulp or the bracket is two neighbours)."""
    return g_error_bound(n, chunk) / S + 2.0 * EPS * max(abs(delta), 2.0 ** -1022)


# ---------------------------------------------------------------------------
# exact arithmetic (mpmath, 60 digits): g, S and the root, independent of everything above
# ---------------------------------------------------------------------------
def _mp():
    import mpmath
    mpmath.mp.dps = 60
    return mpmath


def exact_g(u, v, D):
    """(g, S) at D: g = sum sigma(v + D) - sum sigma(u - D), S = sum sigma (1 - sigma)."""
    mp = _mp()
    D = mp.mpf(float(D)) if not isinstance(D, mp.mpf) else D
    g = S = mp.mpf(0)
    for x, sign in [(x, -1) for x in u] + [(x, 1) for x in v]:
        if x == -np.inf:
            continue
        s = 1 / (1 + mp.exp(-(mp.mpf(float(x)) + sign * D)))
        g += sign * s
        S += s * (1 - s)
    return g, S


def exact_average(x):
    """log of the mean of exp(x) over all samples (-inf: weight 0), as an mpf."""
    mp = _mp()
    return mp.log(sum(mp.exp(mp.mpf(float(e))) for e in x if e != -np.inf) / len(x))


def exact_root(u, v):
    """The root of g by bisection to 50 digits between the extremes of the finite samples."""
    mp = _mp()
    fu, fv = u[np.isfinite(u)], v[np.isfinite(v)]
    lo = mp.mpf(float(min(fu.min(), -fv.max()))) - 1
    hi = mp.mpf(float(max(fu.max(), -fv.min()))) + 1
    assert exact_g(u, v, lo)[0] < 0 < exact_g(u, v, hi)[0]
    while hi - lo > mp.mpf(10) ** -50:
        mid = (lo + hi) / 2
        if exact_g(u, v, mid)[0] < 0:
            lo = mid
        else:
            hi = mid
    return (lo + hi) / 2


# ---------------------------------------------------------------------------
# exact iid draws of the harmonic ladder (no sampler): log p_r(x) = -1/2 k_r |x|^2
# ---------------------------------------------------------------------------
HARMONIC_K = (1.0, 0.5, 0.25, 0.125)
HARMONIC_D = 8


def harmonic_exact(ks=HARMONIC_K, D=HARMONIC_D):
    """delta[r] = log Z_r - log Z_{r+1} = (D / 2) ln(k_{r+1} / k_r)."""
    k = np.asarray(ks, dtype=f64)
    return 0.5 * D * np.log(k[1:] / k[:-1])


def group_statistics(group_delta):
    """(stderr [R - 1], total_stderr) of a [G x (R - 1)] array of group estimates: standard
    deviation over the groups / sqrt(G), of the pairs and of the per-group totals."""
    G = group_delta.shape[0]
    return (group_delta.std(axis=0, ddof=1) / np.sqrt(G),
            float(group_delta.sum(axis=1).std(ddof=1) / np.sqrt(G)))


# the end-to-end run of tests/test_gpu_free_energy.py and its CPU yardstick
E2E_ROUNDS, E2E_LADDERS, E2E_GROUPS, E2E_SIGMAS = 300, 128, 32, 6.0
_yardstick = {}


def harmonic_yardstick(seed=77):
    """The restatement on exact iid draws of the end-to-end ladder at the end-to-end n:
    dict(delta, iid_stderr [R - 1], iid_total_stderr, group_delta, stderr, total_stderr).  The
    pairs of an iid record share no draw, so the total's variance is the sum of theirs."""
    if seed not in _yardstick:
        R = len(HARMONIC_K)
        rec = harmonic_iid_record(E2E_ROUNDS, E2E_LADDERS, seed)
        pooled = bar(rec, R, 0, 1)
        grouped = bar(rec, R, 0, E2E_GROUPS)
        var = 1.0 / pooled['info'][0] - 2.0 / pooled['n'][0]
        stderr, total_stderr = group_statistics(grouped['delta'])
        _yardstick[seed] = dict(delta=pooled['delta'][0], iid_stderr=np.sqrt(var),
                                iid_total_stderr=float(np.sqrt(var.sum())),
                                group_delta=grouped['delta'], stderr=stderr, total_stderr=total_stderr)
    return _yardstick[seed]


def harmonic_iid_record(T, n_ladders, seed, ks=HARMONIC_K, D=HARMONIC_D):
    """A [T x C] work record of rounds 0 .. T-1 whose draws are exact and independent:
    x = z / sqrt(k_r) afresh in every round and chain."""
    R = len(ks)
    C = R * n_ladders
    k = np.tile(np.asarray(ks, dtype=f64), n_ladders)
    rs = np.random.RandomState(seed)
    rec = np.empty((T, C))
    for t in range(T):
        x = rs.standard_normal((C, D)) / np.sqrt(k)[:, None]
        sq = (x * x).sum(axis=1)
        p = partner_or_minus_one(C, R, t & 1)
        lp_own = -0.5 * k * sq
        lp_sw = -0.5 * k * sq[np.where(p >= 0, p, np.arange(C))]
        rec[t] = work_row(lp_own, lp_sw, R, t & 1)
    return rec
