"""Host restatement of ``csrc/loo.hip``, written from the contract in ``include/binf_hip.h``
(section "Model comparison by predictive fit"); nothing here calls into the library.

``psis_column(a, ar)`` takes ONE observation's log-likelihoods, ascending, and returns what
``binf_psis_loo_f64`` returns for it, every sum in the contract's order.  The arithmetic is
injected: the same code runs in numpy doubles (``F64``), in the 80-bit ``np.longdouble``
(``F80``) and in ``mpmath`` at 50 digits (``MP``); each takes the DOUBLE inputs as exact.

``pointwise_terms`` / ``pointwise_exact`` / ``pointwise_bound`` do the same for
``binf_gauss_pointwise_loglik_f64``.  The builders at the end give the CPU and the GPU tests
the same records.

Why 80 bits appear at all.  The GPU tests hold the device to 32 x max(e_host, 2^-53 |value|)
of the 50-digit value, e_host being the largest |double restatement - exact| per output over
the columns of the SAME record.  mpmath affords a few columns per record; the 80-bit
arithmetic affords all of them, and its own distance from the exact value is 2^-11 of the
double one's (11 more bits in every rounding, the same operations), so
    e_host = max over every column of |F64 - F80|, and over the mpmath columns of |F64 - MP|
is the quantity the bar asks for to within a part in two thousand, taken over MORE columns.
A column without an mpmath value is then held against its double restatement:
    |device - F64| <= |device - exact| + |exact - F64| <= 32 E + E,   E = max(e_host, 2^-53 |value|).
"""
import math

import numpy as np

f64 = np.float64
U = 2.0 ** -53
Q = 2.0 ** -1074
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
CHUNK = 8192                       # LOO_CHUNK of csrc/loo.hip
MAX_S = 1 << 22
FIELDS = ('elpd_loo', 'khat', 'n_eff', 'lppd', 'p_waic')


# ---------------------------------------------------------------------------
# arithmetics
# ---------------------------------------------------------------------------
class NumpyArith(object):
    """numpy arithmetic in ``dtype``; non-finite results are left as they fall."""

    def __init__(self, dtype):
        self.dtype = dtype
        self.exp, self.log, self.log1p, self.expm1, self.sqrt = np.exp, np.log, np.log1p, np.expm1, np.sqrt
        self.inf = dtype(np.inf)

    def arr(self, v):
        return np.asarray(v, dtype=f64).astype(self.dtype)

    def num(self, v):
        return self.dtype(v)

    def zeros(self, n):
        return np.zeros(n, dtype=self.dtype)

    def isfinite(self, v):
        return bool(np.isfinite(v))

    def context(self):
        return np.errstate(all='ignore')


class MpArith(object):
    """mpmath at ``dps`` digits on numpy object arrays."""

    def __init__(self, dps=50):
        import mpmath
        self.mp, self.dps = mpmath, dps
        self.exp, self.log, self.log1p, self.expm1, self.sqrt = (
            np.frompyfunc(f, 1, 1) for f in (mpmath.exp, mpmath.log, mpmath.log1p, mpmath.expm1, mpmath.sqrt))
        self.inf = mpmath.inf

    def arr(self, v):
        return np.array([self.mp.mpf(float(x)) for x in np.asarray(v, dtype=f64).reshape(-1)], dtype=object)

    def num(self, v):
        return self.mp.mpf(v)

    def zeros(self, n):
        return np.array([self.mp.mpf(0)] * n, dtype=object)

    def isfinite(self, v):
        return bool(self.mp.isfinite(v))

    def context(self):
        return self.mp.workdps(self.dps)


F64 = NumpyArith(np.float64)
F80 = NumpyArith(np.longdouble)


def MP():
    return MpArith(50)


# ---------------------------------------------------------------------------
# the contract's integers and orders
# ---------------------------------------------------------------------------
def plan(S):
    """(M, m, q): tail length min(floor(S / 5), ceil(3 sqrt(S))), candidates 30 + floor(sqrt(M)),
    quartile index floor(M / 4 + 0.5), in integers."""
    S = int(S)
    c = math.isqrt(9 * S)
    if c * c < 9 * S:
        c += 1
    M = min(S // 5, c)
    return M, 30 + math.isqrt(M), (M + 2) // 4


def tail_len(S):
    return plan(S)[0]


def workspace_bytes(S, N):
    if S < 2 or S > MAX_S or N < 1 or N >= 2 ** 31:
        return 0
    return 8 * N * (8 + 4 * ((S + CHUNK - 1) // CHUNK))


def tree_sum(terms, W, ar):
    """W accumulators from 0.0, term e to accumulator e mod W in ascending order, the W joined by
    the balanced tree over neighbours."""
    n = len(terms)
    rows = max(1, (n + W - 1) // W)
    pad = ar.zeros(rows * W)
    pad[:n] = terms
    pad = pad.reshape(rows, W)
    acc = ar.zeros(W)
    for r in range(rows):
        acc = acc + pad[r]
    while len(acc) > 1:
        acc = acc[0::2] + acc[1::2]
    return acc[0]


def chunked_sum(terms, start, ar):
    """((start + chunk 0) + chunk 1) + ...: chunks of 8192 elements, each a 256-wide tree_sum."""
    s = start
    for lo in range(0, len(terms), CHUNK):
        s = s + tree_sum(terms[lo:lo + CHUNK], 256, ar)
    return s


def seq_sum(terms, ar):
    s = ar.num(0.0)
    for t in terms:
        s = s + t
    return s


def _nan_max(values, first):
    m = first
    for v in values:
        if v > m or v != v:
            m = v
    return m


def psis_column(a, ar=F64):
    """dict(elpd_loo, khat, n_eff, lppd, p_waic, tail_len) of the ascending column ``a`` (doubles),
    as include/binf_hip.h states it, in the arithmetic ``ar``.  Values are ``ar``'s numbers."""
    a = np.asarray(a, dtype=f64).reshape(-1)
    S = a.shape[0]
    M, m, q = plan(S)
    nan = float('nan')
    if not (np.isfinite(a[0]) and np.isfinite(a[-1])):
        return dict(elpd_loo=nan, khat=nan, n_eff=nan, lppd=nan, p_waic=nan, tail_len=M)
    with ar.context():
        A = ar.arr(a)
        a0, aL, dS, dM = A[0], A[S - 1], ar.num(S), ar.num(M)
        abar = tree_sum(A, 256, ar) / dS
        lc = a0 - A[M]
        ec = ar.exp(lc)
        x = ar.exp(a0 - A[M - np.arange(1, M + 1)]) - ec if M else ar.zeros(0)      # x[t - 1], t = 1 .. M
        smooth = M >= 5 and bool(x[M - 1] > 0) and ar.isfinite(x[M - 1])
        khat = ar.inf
        if smooth:
            d3, ixM = 3 * x[q - 1], 1 / x[M - 1]
            b, L = [], []
            for j in range(1, m + 1):
                bj = (1 - ar.sqrt(ar.num(m) / (ar.num(j) - ar.num(0.5)))) / d3 + ixM
                kj = tree_sum(ar.log1p(-bj * x), 64, ar) / dM
                b.append(bj)
                L.append(dM * (ar.log(-bj / kj) - kj - 1))
            w = [1 / seq_sum([ar.exp(Ll - Lj) for Ll in L], ar) for Lj in L]
            # A weight below the cut is dropped; one that falls on the other side of it in another
            # arithmetic moves bhat by about 1e-15 of itself: no special case.
            cut = 10.0 * 2.0 ** -52
            keep = [not (wj < cut) for wj in w]
            W = seq_sum([wj for wj, kp in zip(w, keep) if kp], ar)
            bhat = seq_sum([bj * (wj / W) for bj, wj, kp in zip(b, w, keep) if kp], ar)
            kp = tree_sum(ar.log1p(-bhat * x), 64, ar) / dM
            sigma = -kp / bhat
            khat = (dM * kp + 5) / (dM + 10)
            t = np.arange(1, M + 1)
            p = (ar.arr(t) - ar.num(0.5)) / dM
            qt = sigma * ar.expm1(-khat * ar.log1p(-p)) / khat
            lw = ar.log(qt + ec)
            lw = np.array([ar.num(0.0) if v > 0 else v for v in lw], dtype=lw.dtype)
            lwt = lw[::-1].copy()                      # lwt[j] = lw'_j, j = M - t
        else:
            lwt = a0 - A[:M]
        sh1 = _nan_max(lwt, lc)
        va = lwt + A[:M]
        sh2 = _nan_max(va, a0)
        e = ar.exp(lwt - sh1) if M else ar.zeros(0)
        T1, T1q = tree_sum(e, 256, ar), tree_sum(e * e, 256, ar)
        T2 = tree_sum(ar.exp(va - sh2), 256, ar) if M else ar.num(0.0)
        eb = ar.exp((a0 - A) - sh1)
        eb[:M] = ar.num(0.0)
        s1, s1q = chunked_sum(eb, T1, ar), chunked_sum(eb * eb, T1q, ar)
        s2 = T2 + ar.num(S - M) * ar.exp(a0 - sh2)
        s3 = chunked_sum(ar.exp(A - aL), ar.num(0.0), ar)
        d = A - abar
        s4 = chunked_sum(d * d, ar.num(0.0), ar)
        return dict(elpd_loo=(sh2 - sh1) + (ar.log(s2) - ar.log(s1)), khat=khat, n_eff=(s1 * s1) / s1q,
                    lppd=aL + (ar.log(s3) - ar.log(dS)), p_waic=s4 / ar.num(S - 1), tail_len=M)


def psis_record(ll, ar=F64, columns=None):
    """``psis_column`` of every column (or of ``columns``) of the record ``ll [S x N]``, sorted
    here: dict of float arrays [len(columns)] and the int array ``tail_len``."""
    ll = np.asarray(ll, dtype=f64)
    cols = range(ll.shape[1]) if columns is None else columns
    res = [psis_column(np.sort(ll[:, i]), ar) for i in cols]
    out = {k: np.array([float(r[k]) for r in res]) for k in FIELDS}
    out['tail_len'] = np.array([r['tail_len'] for r in res], dtype=np.int32)
    return out


def totals(x):
    """(sum, sum of squared deviations from sum / N) of ``x [N]`` in binf_pointwise_totals_f64's
    order."""
    x = np.asarray(x, dtype=f64)
    s = tree_sum(x, 256, F64)
    d = x - s / f64(x.shape[0])
    return float(s), float(tree_sum(d * d, 256, F64))


def se_of(ssq, n):
    return math.sqrt(n * ssq / (n - 1)) if n > 1 else float('nan')


# ---------------------------------------------------------------------------
# the pointwise record
# ---------------------------------------------------------------------------
def pointwise_terms(mock, precision, ys, half_log_2pi=HALF_LOG_2PI):
    """The record in doubles, numpy's evaluation of the contract's expression."""
    m, tau, y = (np.asarray(v, dtype=f64) for v in (mock, precision, ys))
    with np.errstate(all='ignore'):
        d = m - y[None, :]
        return (-0.5 * (d * d)) * tau[:, None] + (0.5 * np.log(tau))[:, None] - f64(half_log_2pi)


def pointwise_exact(m, y, tau, half_log_2pi=HALF_LOG_2PI, dps=50):
    """One element from the doubles ``m``, ``y``, ``tau > 0`` (finite), every operation exact:
    (value, a, h) as mpf, a = 0.5 (m - y)^2 tau and h = 0.5 log tau."""
    import mpmath
    with mpmath.workdps(dps):
        mpf = mpmath.mpf
        d = mpf(float(m)) - mpf(float(y))
        a = d * d * mpf(float(tau)) / 2
        h = mpmath.log(mpf(float(tau))) / 2
        return -a + h - mpf(float(half_log_2pi)), a, h


def pointwise_bound(a, h, tau, half_log_2pi=HALF_LOG_2PI):
    """The allowed |device - exact| of one element of binf_gauss_pointwise_loglik_f64, from its
    order of operations; ``a`` = 0.5 (m - y)^2 tau and ``h`` = 0.5 log tau (floats), u = 2^-53.

    ASSUMPTION (the project's standing one; predict_ref.density_bound): the device library's
    log is within ONE ulp of the exact one, and an ulp of v is at most 2 u |v|.

      d = fl(m - y)                one rounding:  (m - y)(1 + u)
      fl(d d)                      three factors (1 + u)
      -0.5 * .                     exact
      fl(. * tau)                  a fourth:      the quadratic part is off by 4 u a
      hlp = 0.5 * log~(tau)        an ulp of the log, the halving exact:  2 u |h|
      fl(-a~ + hlp)                rounds a value of at most a + |h|:     u (a + |h|)
      fl(. - c)                    rounds a value of at most a + |h| + c: u (a + |h| + c)
    Together u (6 a + 4 |h| + c).  Where d d or the product with tau lands in the subnormal
    range the lost part is at most one quantum q = 2^-1074 of each: q tau / 2 + q.  The factor
    1.01 covers the products of two such terms (first-order terms are below 2^-40 of the
    value's parts for any finite double input)."""
    return 1.01 * (U * (6.0 * float(a) + 4.0 * abs(float(h)) + abs(half_log_2pi)) + Q * (0.5 * float(tau) + 1.0))


# ---------------------------------------------------------------------------
# records shared by the CPU and the GPU tests: ll [S x N], draws in random order
# ---------------------------------------------------------------------------
def _rs(name, S, N, seed):
    return np.random.RandomState((sum(map(ord, name)) * 7919 + S * 131 + N * 17 + seed * 104729) % (2 ** 31))


def gaussian_data(N, seed=0, outlier=4.5):
    """y_i ~ N(0.3, 1), the last point moved to ``outlier`` sigma above the mean of the others."""
    rs = _rs('gaussian_data', 0, N, seed)
    y = 0.3 + rs.standard_normal(N)
    if N > 1:
        y[N - 1] = y[:N - 1].mean() + outlier
    return y


def gaussian_model(S, N, seed=0):
    """The conjugate model y_i ~ N(mu, 1) with a flat prior: S exact posterior draws
    mu_s ~ N(ybar, 1 / N), ll[s, i] = log N(y_i | mu_s, 1); one point at 4.5 sigma."""
    y = gaussian_data(N, seed)
    rs = _rs('gaussian_model', S, N, seed)
    mu = y.mean() + rs.standard_normal(S) / math.sqrt(N)
    return -0.5 * (y[None, :] - mu[:, None]) ** 2 - HALF_LOG_2PI


def gaussian_exact_elpd(y):
    """elpd_i = log N(y_i | ybar_(-i), 1 + 1 / (N - 1)) of the conjugate model, closed form."""
    y = np.asarray(y, dtype=f64)
    N = y.shape[0]
    loo_mean = (y.sum() - y) / (N - 1)
    var = 1.0 + 1.0 / (N - 1)
    return -0.5 * (y - loo_mean) ** 2 / var - 0.5 * math.log(2.0 * math.pi * var)


def pareto_tail(S, N, seed=0, k=0.5):
    """ll = -k E, E ~ Exp(1): the importance ratios exp(-ll) are Pareto with shape k."""
    return -k * _rs('pareto_tail%g' % k, S, N, seed).exponential(size=(S, N))


def one_dominant(S, N, seed=0):
    """One draw per observation, at a random place, lies 30 below the others (sd 0.1): it carries
    nearly all the weight, and nothing underflows (e^-30)."""
    rs = _rs('one_dominant', S, N, seed)
    ll = -1.0 + 0.1 * rs.standard_normal((S, N))
    ll[rs.randint(S, size=N), np.arange(N)] -= 30.0
    return ll


def flat(S, N, seed=0):
    """Every draw of an observation has the same log-likelihood: x_M = 0, no smoothing."""
    return np.tile(-0.5 - _rs('flat', S, N, seed).uniform(size=N), (S, 1))


def near_flat_tail(S, N, seed=0):
    """The draws of an observation differ in the last bits: -(b_i + (4 r + r mod 3) 2^-52), r a
    permutation of 0 .. S-1, b_i = 1 + i / 128 -- every value an exact double in (-2, -1]; the
    exceedances are about 4 t 2^-52, multiples of 2^-53.  (The r mod 3 keeps them off an exact
    arithmetic progression, on which a candidate b_j of the fit can vanish identically --
    m / (j - 0.5) = 2.56 at M = 5 -- and its profile likelihood is 0 / 0.)"""
    rs = _rs('near_flat_tail', S, N, seed)
    out = np.empty((S, N))
    for i in range(N):
        r = rs.permutation(S)
        out[:, i] = -((1.0 + (i % 100) / 128.0) + (4.0 * r + r % 3) * 2.0 ** -52)
    return out


def wide(S, N, seed=0):
    """ll uniform over a span of 600: the body's weights fall to e^-600 and their squares
    underflow."""
    return -600.0 * _rs('wide', S, N, seed).uniform(size=(S, N))


BUILDERS = dict(gaussian_model=gaussian_model,
                pareto_tail_02=lambda S, N, seed=0: pareto_tail(S, N, seed, 0.2),
                pareto_tail_05=lambda S, N, seed=0: pareto_tail(S, N, seed, 0.5),
                pareto_tail_09=lambda S, N, seed=0: pareto_tail(S, N, seed, 0.9),
                one_dominant=one_dominant, flat=flat, near_flat_tail=near_flat_tail, wide=wide)


def host_error(ll, mp_columns=()):
    """The restatement's own error on the record ``ll [S x N]``: (f, e_host, exact) --
    ``f``: psis_record in doubles, every column; ``e_host``: per output the largest
    |F64 - F80| over every column and |F64 - MP| over ``mp_columns`` (module docstring);
    ``exact``: {column: psis_column in mpmath} for ``mp_columns``.  A pair of equal infinities
    (khat without a fit) or of NaNs counts as no error."""
    ll = np.asarray(ll, dtype=f64)
    f = psis_record(ll, F64)
    g = psis_record(ll, F80)
    assert np.finfo(np.longdouble).nmant >= 63, 'np.longdouble is not the 80-bit format here'
    exact = {int(i): psis_column(np.sort(ll[:, i]), MP()) for i in mp_columns}

    def gap(x, y):
        if x == y or (x != x and y != y):
            return 0.0
        return abs(x - y)
    e = {}
    for k in FIELDS:
        worst = max(gap(float(a), float(b)) for a, b in zip(f[k], g[k]))
        for i, ex in exact.items():
            worst = max(worst, gap(float(f[k][i]), float(ex[k])) if ex[k] == ex[k] else 0.0)
        e[k] = worst
    return f, e, exact
