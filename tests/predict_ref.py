"""The posterior-predictive density of ``csrc/predict.hip`` in exact arithmetic, and the bound
that its double-precision evaluations are held to.  Written from the contract in
``include/binf_hip.h``; nothing here calls into the library.

    p = exp(log(sum_s exp(f_s - M)) + M) / S,   M = max_s f_s,   t = sum_s exp(f_s - M)
    f_s = -0.5 (m_s - y)^2 tau_s + 0.5 log tau_s - half_log_2pi

``exact_density`` takes the DOUBLE inputs as they are and evaluates the expression with mpmath
at 60 digits; ``density_bound`` is the allowed |double evaluation - exact|, derived in its
docstring from the kernel's order of operations and from nothing that was measured.
``kernel_plan`` restates how the library cuts the samples into chunks (``predict_splits`` and
``chunk`` in ``csrc/predict.hip``), which fixes the depth of the kernel's sum.  The builders at
the end give the CPU and the GPU tests the same data.
"""
import math

import numpy as np

f64 = np.float64
U = 2.0 ** -53                     # unit roundoff of a double
Q = 2.0 ** -1074                   # the smallest subnormal
ZEROED = -745.2                    # np_exp (gauss_common.hpp) returns 0 below this exponent
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
XT, SL, JT = 16, 16, 8             # PRED_XT, PRED_SL, PRED_JT of csrc/predict.hip
DPS = 60


# ---------------------------------------------------------------------------
# the library's cut of the samples
# ---------------------------------------------------------------------------
def predict_splits(S, nx, ny):
    """``predict_splits`` of csrc/predict.hip for an [nx x ny] grid."""
    blocks = ((nx + XT - 1) // XT) * ((ny + JT - 1) // JT)
    ns = (1024 + blocks - 1) // blocks
    ns = min(ns, S // 256, 64)
    return 1 if ns < 2 else ns


def kernel_plan(S, nx, ny):
    """dict(ns, chunk, last, need, depth, joined): the number of sample chunks, the samples per
    chunk, the samples of the last chunk, the workspace bytes, and the additions on the
    longest path of the kernel's sum of exponentials:

      * a sample lane adds its share, at most ceil(chunk / 16) terms, in sequence,
      * 15 additions join the 16 sample lanes,
      * where the samples are cut (``joined``), ns - 1 additions join the chunks."""
    ns = predict_splits(S, nx, ny)
    chunk = (S + ns - 1) // ns if ns > 1 else S
    return dict(ns=ns, chunk=chunk, last=S - (ns - 1) * chunk, joined=ns > 1,
                need=0 if ns == 1 else ns * nx * ny * 16,
                depth=(chunk + SL - 1) // SL + (SL - 1) + (ns - 1))


# ---------------------------------------------------------------------------
# exact arithmetic
# ---------------------------------------------------------------------------
def terms_f64(mock_col, y, precision, half_log_2pi=HALF_LOG_2PI):
    """f_s in doubles, as numpy forms them (the restatement's integrand, oracle/ref_example.py)."""
    m, tau = np.asarray(mock_col, dtype=f64), np.asarray(precision, dtype=f64)
    with np.errstate(all='ignore'):
        return -0.5 * (m - f64(y)) ** 2 * tau + 0.5 * np.log(tau) - f64(half_log_2pi)


def exact_density(mock_col, y, precision, half_log_2pi=HALF_LOG_2PI):
    """The density at one point from the doubles ``mock_col`` [S], ``y``, ``precision`` [S],
    ``half_log_2pi``, every operation exact (mpmath, 60 digits).

    Returns dict(density, f, a, h, M, t, S, c): ``density`` an mpf (or a float NaN), ``M`` and
    ``t`` as mpf, and for the bound's weights, rounded to doubles, ``f`` [S] = f_s - M (-inf
    where a term is dropped), ``a`` = 0.5 (m - y)^2 tau and ``h`` = 0.5 log tau [S].

    Non-finite terms follow the contract of include/binf_hip.h, which is numpy's: which
    terms are NaN, -inf or +inf is read off the double evaluation (a NaN input, a negative
    precision, 0 * inf, inf - inf); a NaN term makes the density NaN, a +inf term as well
    (inf - inf under the maximum), terms of -inf drop out of the sum, and if every term
    is -inf the density is NaN (inf - inf again)."""
    import mpmath
    mock_col = np.asarray(mock_col, dtype=f64).reshape(-1)
    precision = np.asarray(precision, dtype=f64).reshape(-1)
    S = mock_col.shape[0]
    fd = terms_f64(mock_col, y, precision, half_log_2pi)
    nan = dict(density=float('nan'), f=fd, a=None, h=None, M=None, t=None, S=S)
    if np.any(np.isnan(fd)) or np.any(fd == np.inf) or not np.any(np.isfinite(fd)):
        return nan
    with mpmath.workdps(DPS):
        mpf = mpmath.mpf
        ym, c = mpf(float(y)), mpf(float(half_log_2pi))
        f = [None] * S
        a, h = np.zeros(S), np.zeros(S)
        logs = {}
        for s in range(S):
            if fd[s] == -np.inf:
                continue
            tau = float(precision[s])
            if tau not in logs:
                logs[tau] = mpmath.log(mpf(tau)) / 2
            d = mpf(float(mock_col[s])) - ym
            as_ = d * d * mpf(tau) / 2
            f[s] = -as_ + logs[tau] - c
            a[s], h[s] = float(as_), float(logs[tau])
        M = max(v for v in f if v is not None)
        t = mpmath.fsum(mpmath.exp(v - M) for v in f if v is not None)
        density = mpmath.exp(mpmath.log(t) + M) / S
        ff = np.array([-np.inf if v is None else float(v - M) for v in f])
        return dict(density=density, f=ff, a=a, h=h, M=M, t=t, S=S, c=float(half_log_2pi))


def density_bound(ex, depth, joined=False):
    """The allowed |p~ - p| (an mpf) between a double evaluation p~ of the density in the
    kernel's order and the exact value p of ``ex = exact_density(...)``, for a sum of
    exponentials whose longest path has ``depth`` additions (``kernel_plan`` for the kernel; S
    covers any order).  ``joined``: the sum went through the chunked path.

    u = 2^-53.  Every step is first order in u; the 1.01 at the end covers the products of two
    such terms (smc_ref.py does the same), and the bound refuses to be used (inf) where the
    first-order sum exceeds 2^-10, so that those products stay below 1 % of it.

    ASSUMPTION (the project's standing one, csrc/smc.hip): the device library's exp and log,
    and np_exp, which is the library's exp written out, return a value within ONE ULP of the
    exact one.  An ulp of v is at most 2 u |v|.  numpy's exp / log are held to the same.

    1. A term.  d = fl(m - y) = (m - y)(1 + u);  fl(d d) carries three factors (1 + u);  the
       halving is exact;  fl(. * tau) a fourth:  the quadratic part a = 0.5 (m - y)^2 tau is
       off by 4 u a.  h = 0.5 log tau: one ulp of the log, 2 u |h|.  fl(-a + h) rounds a value
       of at most a + |h|:  u (a + |h|).  fl(. - c) with c = half_log_2pi rounds a value of at
       most a + |h| + c.  Together
           |f~_s - f_s| <= e_s = u (6 a_s + 4 |h_s| + c).
       Where d d or the product with tau underflows, the lost part is at most one subnormal
       quantum q = 2^-1074 of each: q tau / 2 + q more in e_s.
    2. Its exponential.  x = fl(f~_s - M~) = (f~_s - M~)(1 + u) and exp within an ulp give
           E_s = exp(f_s - M~) (1 + r_s),   r_s = e_s + u |f_s - M| + 2 u.
       M~, the largest computed term, is chosen without rounding and cancels in the end:
       exp(log(t~) + M~) = sum_s exp(f_s)(1 + ...), whichever term M~ is.  |f~_s - M~| differs
       from |f_s - M| by at most e_s + e_max, second order once multiplied by u.
       In the chunked path the term is E_s = exp(f~_s - M~_z) * exp(M~_z - M~): the two
       exponents add up to the same f~_s - M~ (both are <= 0, so do their roundings), the second
       exponential brings another ulp, 2 u, and the product one rounding, u: 3 u more.
    3. The sum.  All E_s >= 0, so the additions along a path of ``depth`` roundings move the
       sum by at most depth * u of itself.  With w_s = exp(f_s - M) / t, the share of term s,
           |t~ - t| / t <= sum_s w_s r_s + depth u (+ 3 u joined).
       A term that contributes nothing (w_s = 0) loosens nothing, whatever its e_s.
       A term with f~_s - M~ < -745.2 is zeroed by np_exp: its whole share w_s is lost, which is
       what r_s = 1 says (taken for every term below -744.2, a unit of room for the distance
       between f~_s - M~ and f_s - M; such a share is below e^-744); and an exponential that lands in the subnormal range is off by up to
       q absolutely, q / t each -- S q / t in all (t >= 1).  Both are far below u; they are in the
       bound so that it holds where only such terms exist besides the largest.
    4. lse = fl(log~(t~) + M~):  the log within an ulp, 2 u |log t|;  the addition rounds
       |log t + M| by u.  An absolute error in lse is a relative one in exp(lse).
    5. exp~(lse) within an ulp, 2 u;  the division by S, u.
    6. The last two operations may each land in the subnormal range: q absolutely for each.

           bound = 1.01 p (sum_s w_s r_s + (depth + [3]) u + S q / t
                           + 2 u |log t| + u |log t + M| + 3 u)  +  2 q."""
    import mpmath
    S = ex['S']
    with mpmath.workdps(DPS), np.errstate(over='ignore'):
        fin = ex['f'] > -np.inf                      # f holds f_s - M
        rel = ex['f'][fin]
        w = np.exp(rel) / float(ex['t'])
        tau = np.exp(np.minimum(2.0 * ex['h'][fin], 709.7))              # h = 0.5 log tau
        e = U * (6.0 * ex['a'][fin] + 4.0 * np.abs(ex['h'][fin]) + abs(ex['c'])) + Q * (0.5 * tau + 1.0)
        r = np.where(rel < ZEROED + 1.0, 1.0, e + U * np.abs(rel) + 2.0 * U)
        with np.errstate(invalid='ignore'):
            first = float(np.sum(np.where(w > 0.0, w * np.minimum(r, 1e300), 0.0)))
        logt = float(mpmath.log(ex['t']))
        lse = float(mpmath.log(ex['t']) + ex['M'])
        first += (depth + (3 if joined else 0)) * U + S * Q / float(ex['t'])
        first += 2.0 * U * abs(logt) + U * abs(lse) + 3.0 * U
        if not first <= 2.0 ** -10:
            return mpmath.inf
        return mpmath.mpf(1.01) * ex['density'] * mpmath.mpf(first) + 2 * mpmath.mpf(Q)


def grid_bound(mock, precision, ys, depth, joined=False, half_log_2pi=HALF_LOG_2PI):
    """``density_bound`` for every point of a grid at once, in doubles: (p, bound, bound_mean),
    each [nx x ny].  For FINITE data whose densities are normal numbers: the weights and the
    density itself are the double evaluation here, which moves the bound in its second
    order only (tests/test_predict.py holds the two to 1e-9 of each other).  ``bound_mean`` is the allowed
    |numpy - exact| of the plain mean of the S Gaussian densities
    sqrt(tau / 2 pi) exp(-0.5 tau d^2): 4 u a in the exponent as in step 1, an ulp of exp, two
    roundings and a square root in the factor, one product, at most S additions, one
    division -- 1.01 p (sum_s w_s 4 u a_s + (S + 8) u)."""
    mock, tau, ys = (np.asarray(v, dtype=f64) for v in (mock, precision, ys))
    S = mock.shape[0]
    with np.errstate(over='ignore', under='ignore'):
        d = mock[:, :, None] - ys[None]
        a = 0.5 * d * d * tau[:, None, None]
        h = (0.5 * np.log(tau))[:, None, None]
        f = -a + h - half_log_2pi
        M = f.max(0)
        rel = f - M
        w = np.exp(rel)
        t = w.sum(0)
        w = w / t
        e = U * (6.0 * a + 4.0 * np.abs(h) + abs(half_log_2pi)) + Q * (0.5 * tau[:, None, None] + 1.0)
        r = np.where(rel < ZEROED + 1.0, 1.0, e + U * np.abs(rel) + 2.0 * U)
        first = (w * r).sum(0) + (depth + (3 if joined else 0)) * U + S * Q / t
        first = first + 2.0 * U * np.abs(np.log(t)) + U * np.abs(np.log(t) + M) + 3.0 * U
        p = np.exp(np.log(t) + M) / S
        bound = np.where(first <= 2.0 ** -10, 1.01 * p * first + 2.0 * Q, np.inf)
        return p, bound, 1.01 * p * ((w * (4.0 * U * a)).sum(0) + (S + 8) * U)


def edge_points(mock, precision, ys, half_log_2pi=HALF_LOG_2PI):
    """dict(zero, subnormal, normal) -> one (i, j) of each kind the grid has, by the vectorised
    double evaluation of the density (the restatement's expression; it only CHOOSES points)."""
    mock, tau, ys = (np.asarray(v, dtype=f64) for v in (mock, precision, ys))
    with np.errstate(all='ignore'):
        f = -0.5 * (mock[:, :, None] - ys[None]) ** 2 * tau[:, None, None] + (0.5 * np.log(tau))[:, None, None] - half_log_2pi
        M = f.max(0)
        p = np.exp(np.log(np.exp(f - M).sum(0)) + M) / mock.shape[0]
    kinds = dict(zero=p == 0.0, subnormal=(p > 0.0) & (p < 2.0 ** -1022), normal=p >= 2.0 ** -1022)
    return {k: tuple(int(v) for v in np.argwhere(m)[0]) for k, m in kinds.items() if m.any()}


def mean_of_densities(mock, precision, ys):
    """The mean over the samples of the Gaussian densities, no log_sum_exp: [nx x ny]."""
    mock, tau, ys = (np.asarray(v, dtype=f64) for v in (mock, precision, ys))
    dens = np.sqrt(tau / (2 * np.pi))[:, None, None] * np.exp(-0.5 * tau[:, None, None] * (mock[:, :, None] - ys[None]) ** 2)
    return dens.mean(0)


def error_over_bound(got, ex, depth, joined=False):
    """|got - exact| / bound as a float (inf for a NaN ``got``)."""
    import mpmath
    if got != got:
        return float('inf')
    with mpmath.workdps(DPS):
        return float(abs(mpmath.mpf(float(got)) - ex['density']) / density_bound(ex, depth, joined))


def below_half_quantum(ex):
    """True where the exact density is below 2^-1074 / 2: a double evaluation may only return 0
    or the smallest subnormal there."""
    import mpmath
    with mpmath.workdps(DPS):
        return bool(ex['density'] < mpmath.mpf(Q) / 2)


# ---------------------------------------------------------------------------
# inputs shared by the CPU and the GPU tests: (mock [S x nx], precision [S], ys [nx x ny])
# ---------------------------------------------------------------------------
def _rs(name, S, nx, ny, seed):
    return np.random.RandomState((sum(map(ord, name)) * 7919 + S * 131 + nx * 17 + ny + seed * 104729) % (2 ** 31))


def mild(S, nx, ny, seed=0):
    """The data of tests/test_gpu_predict.py: cubic polynomials with standard_normal * 0.3
    coefficients at uniform x, gamma(4, 0.5) precisions, standard_normal * 2 y."""
    rs = _rs('mild', S, nx, ny, seed)
    c = rs.standard_normal((S, 4)) * 0.3
    xs = rs.uniform(-1, 1, size=nx)
    mock = ((c[:, 0, None] * xs + c[:, 1, None]) * xs + c[:, 2, None]) * xs + c[:, 3, None]
    return mock, rs.gamma(4.0, 0.5, size=S), rs.standard_normal((nx, ny)) * 2


def far_tail(S, nx, ny, seed=0):
    """Every quadratic term far out: |mock| <= 0.05, precisions in [0.97, 1.03], and y so that
    0.5 y^2 walks over [620, 790] from point to point (a low-discrepancy walk, so that a grid
    of any size meets the whole range): the terms lie in about [-815, -600], the density from
    1e-262 through the subnormals (2^-1074 = e^-744.4) to exactly 0."""
    rs = _rs('far_tail', S, nx, ny, seed)
    mock = rs.uniform(-0.05, 0.05, size=(S, nx))
    tau = rs.uniform(0.97, 1.03, size=S)
    k = np.arange(nx * ny, dtype=f64)
    a0 = 620.0 + 170.0 * np.mod(k * 0.6180339887498949 + 0.37 * seed + 0.11 * (S % 7), 1.0)
    # the subnormal window is narrow (e^-744.4 .. e^-708.4 / S): every fourth point sits in it
    a0[3::4] = 738.0 + 8.0 * np.mod(k[3::4] * 0.6180339887498949 + 0.29 * seed, 1.0)
    ys = np.sqrt(2.0 * a0).reshape(nx, ny) * np.where(rs.uniform(size=(nx, ny)) < 0.5, -1.0, 1.0)
    return mock, tau, ys


def wide_precision(S, nx, ny, seed=0):
    """Precisions 10 ** uniform(-300, 300), one subnormal (2^-1070) and one near DBL_MAX
    (1.7e308) where S allows: 0.5 log(precision) in [-371, 355] dominates f.  Most y are a unit
    away from the mock values (the term with precision ~ 1 / d^2 carries the point); every third
    point sits EXACTLY on one sample's mock value, so that a term with a huge precision and
    d = 0 carries it: densities up to 1e153."""
    rs = _rs('wide_precision', S, nx, ny, seed)
    tau = 10.0 ** rs.uniform(-300.0, 300.0, size=S)
    if S >= 2:
        tau[rs.randint(S)] = 2.0 ** -1070
    if S >= 3:
        free = np.nonzero(tau != 2.0 ** -1070)[0]
        tau[free[rs.randint(free.size)]] = 1.7e308
    mock = rs.standard_normal((S, nx))
    ys = rs.standard_normal((nx, ny)) * 2
    flat = np.arange(nx * ny)
    for k in flat[::3]:
        i, j = divmod(int(k), ny)
        ys[i, j] = mock[rs.randint(S), i]
    return mock, tau, ys


def one_dominant(S, nx, ny, carrier=0, seed=0):
    """Sample ``carrier`` carries every point; every other term lies more than 745.2 below it, so
    the device's np_exp returns exactly 0 for it.  All precisions are 1; mock[carrier, i] is a
    base b_i, ys[i, j] = b_i + (0.01 .. 1), the other samples sit 41 .. 43 away from b_i: their
    quadratic part is at least 0.5 * 40^2 = 800 against at most 0.5 for the carrier."""
    rs = _rs('one_dominant', S, nx, ny, seed)
    carrier = carrier % S
    base = rs.standard_normal(nx)
    mock = base[None, :] + rs.uniform(41.0, 43.0, size=(S, nx)) * np.where(rs.uniform(size=(S, nx)) < 0.5, -1.0, 1.0)
    mock[carrier] = base
    ys = base[:, None] + rs.uniform(0.01, 1.0, size=(nx, ny))
    return mock, np.ones(S), ys


def near_equal_chunk_maxima(S, nx, ny, seed=0, chunk=None):
    """The largest terms of the sample chunks differ by an ulp or two.  ``chunk``: the kernel's
    (``kernel_plan``), or a quarter of the samples where the kernel does not cut them.  All
    precisions are 1.  One sample per chunk, at a random place in it, has mock = b_i moved by
    0, 2 or 4 ulps (z mod 3); y = b_i + (0.01 .. 0.1), so these are the largest terms, about
    -0.92, and differ by d * ulp(b) -- a fraction of an ulp of f, whose rounding then makes
    the computed maxima equal or an ulp or two apart.  The other samples sit 0.5 .. 3 away."""
    rs = _rs('near_equal', S, nx, ny, seed)
    if chunk is None:
        plan = kernel_plan(S, nx, ny)
        chunk = plan['chunk'] if plan['joined'] else max(1, (S + 3) // 4)
    base = 1.0 + rs.uniform(0.0, 0.9, size=nx)
    mock = base[None, :] + rs.uniform(0.5, 3.0, size=(S, nx)) * np.where(rs.uniform(size=(S, nx)) < 0.5, -1.0, 1.0)
    for z, lo in enumerate(range(0, S, chunk)):
        top = lo + rs.randint(min(chunk, S - lo))
        mock[top] = base - 2.0 * (z % 3) * np.spacing(base)
    ys = base[:, None] + rs.uniform(0.01, 0.1, size=(nx, ny))
    return mock, np.ones(S), ys


BUILDERS = dict(mild=mild, far_tail=far_tail, wide_precision=wide_precision, one_dominant=one_dominant,
                near_equal_chunk_maxima=near_equal_chunk_maxima)


def one_dominant_carriers(S):
    """The carriers the issue of this module names: each sample lane 0..15, the first and the last
    sample (as indices < S, without repeats)."""
    out = []
    for c in list(range(SL)) + [0, S - 1]:
        if c % S not in out:
            out.append(c % S)
    return out


def nonfinite_cases(nx, ny, S=20, seed=0):
    """(label, mock, precision, ys) on ``mild`` data with one thing planted.  The poisoned x-point
    is nx - 1 and the poisoned y-value ny - 1 (the last partial tiles, where the kernel's
    clamped reads of dead threads land), the poisoned sample S - 1 (the last lane round, the
    last chunk):

      nan_mock       mock[S-1, nx-1] = NaN            row nx - 1 is NaN, nothing else
      nan_y          ys[nx-1, ny-1] = NaN             that point is NaN, nothing else
      inf_precision  precision[S-1] = +inf            every point NaN (-inf + inf; 0 * inf at d = 0)
      neg_precision  precision[S-1] = -1              every point NaN (log of a negative)
      pinf_mock, ninf_mock  mock[S-1, nx-1] = +-inf   a term of -inf: dropped from row nx - 1
      zero_precision_some   every other precision 0   terms of -inf: dropped
      zero_precision_all    every precision 0         every point NaN (inf - inf)"""
    out = []
    for label in ('nan_mock', 'nan_y', 'inf_precision', 'neg_precision', 'pinf_mock', 'ninf_mock',
                  'zero_precision_some', 'zero_precision_all'):
        mock, tau, ys = mild(S, nx, ny, seed)
        if label == 'nan_mock':
            mock[S - 1, nx - 1] = np.nan
        elif label == 'nan_y':
            ys[nx - 1, ny - 1] = np.nan
        elif label == 'inf_precision':
            tau[S - 1] = np.inf
        elif label == 'neg_precision':
            tau[S - 1] = -1.0
        elif label == 'pinf_mock':
            mock[S - 1, nx - 1] = np.inf
        elif label == 'ninf_mock':
            mock[S - 1, nx - 1] = -np.inf
        elif label == 'zero_precision_some':
            tau[0::2] = 0.0
        else:
            tau[:] = 0.0
        out.append((label, mock, tau, ys))
    return out


def nonfinite_nan_mask(label, nx, ny):
    """Where the density of ``nonfinite_cases`` is NaN, by the rules above."""
    mask = np.zeros((nx, ny), dtype=bool)
    if label == 'nan_mock':
        mask[nx - 1] = True
    elif label == 'nan_y':
        mask[nx - 1, ny - 1] = True
    elif label in ('inf_precision', 'neg_precision', 'zero_precision_all'):
        mask[:] = True
    return mask


def poisoned_points(label, nx, ny):
    """The poisoned point and its neighbours in both directions."""
    return [(i, j) for i in (nx - 1, max(nx - 2, 0)) for j in (ny - 1, max(ny - 2, 0), 0)]


def sample_points(nx, ny, n=10):
    """At most ``n`` (i, j): the four corners (the last partial tiles among them), the first point
    past a full tile in each direction, and an even walk over the rest."""
    pts = [(0, 0), (nx - 1, ny - 1), (0, ny - 1), (nx - 1, 0), (min(XT, nx - 1), min(JT, ny - 1))]
    stride = max(1, (nx * ny) // max(1, n - len(pts)))
    pts += [divmod(k, ny) for k in range(stride // 2, nx * ny, stride)]
    seen = []
    for p in pts:
        if p not in seen:
            seen.append(p)
    return seen[:n]
