"""Ladders, cases, bounds and assertion functions that hold the polynomial log-prob kernels
(csrc/poly.hip, csrc/rowsum.hpp, the Gaussian epilogue they share with the pair-distance
likelihood) to numpy and to exact arithmetic over the whole range of a double.

The assertion functions take a *backend*: an object with the methods of ``NumpyRoutes`` below,
arrays in, arrays out.  tests/test_gpu_poly_range.py hands them the device through the C ABI;
tests/test_poly_range.py hands them numpy itself (they must pass) and mutated restatements of
the kernels (they must fail): the same functions, so what the CPU file shows of their power
holds for the device run.

Comparison rule ("bit for bit", ``same_bits``): the NaN masks are equal and the int64 views are
equal wherever the values are not NaN.  The sign of zero counts; sign and payload of a NaN do not.

Input classes (``case`` / ``forward_case``, fixed seeds):
  F  finite: coefficients, xs and ys from the ladder's small and moderate entries and N(0, 1);
     every reference mock datum and chi^2 is finite, at least half of the chi^2 values are
     nonzero and pairwise distinct (``class_f_holds``).  ``small_ys=True`` draws ys from the
     entries below 2^-500 and makes every third chain tiny, so that those chains' chi^2 are
     small multiples of 2^-1074, odd ones among them.  The weights of d * d / w are positive
     and finite (``F_WEIGHTS`` and exp(N(0, 1))): the weighted chi^2 is held to the same
     condition, so the weighted route is compared on numbers, not on NaN masks; class O and
     ``check_weight_edges`` (one zero, subnormal, negative, infinite or NaN weight in a class F
     case) carry the weights at which d * d / w leaves the finite range.
  O  overflow: inputs from the whole ladder, ys with +-inf so that inf - inf occurs.  Every
     third chain is constant (only c0 nonzero): its mock data stay finite and its chi^2 is +inf
     without a NaN.  Horner on finite coefficients and a finite x overflows to +-inf but cannot
     give NaN (a value only becomes infinite through a product by |x| > 1, after which neither
     inf * 0 nor inf - inf can follow), so chain 1 has an infinite leading coefficient: -inf and
     +inf by the sign of x, NaN at x = 0.  For K >= 2, N >= 7, C >= 9 the reference mock data hold
     each of +inf, -inf and NaN, the infinities also in chains whose inputs are all finite, and
     the reference chi^2 holds +inf and NaN (``class_o_holds``; one coefficient cannot overflow).
  X  a class F case with one non-finite entry (``spoil``): the checks demand that everything the
     entry does not reach keeps its class F bits, so a result that is NaN everywhere fails.

The epilogue's bound (``logp_bound``).  With u = 2^-53, TINY = 2^-1074, chi2 the value the
epilogue multiplies, A = chi2 tau / 2, B = (N / 2) |ln tau|, E = -A + (N / 2) ln tau:
  * -0.5 chi2 is exact unless chi2 is an odd multiple of TINY (then it loses TINY / 2);
  * the product by tau rounds once: u A, or TINY / 2 where it is subnormal;
  * the device log may be one ulp off: 2u |ln tau|, through the factor N / 2 (exact): 2u B;
  * (N 0.5) log rounds once: u B (it cannot underflow: |ln tau| >= 2^-53 unless tau = 1, N/2 >= 0.5);
  * the sum rounds once: u |lp| (a subnormal sum is exact);
  -> u (A + 3 B + |E|) (1 + 8u), the factor paying for the second-order terms, plus the
  underflow allowance TINY (tau / 2 + 1): the halving's TINY / 2 multiplied by tau (1 + u), and
  the product's own TINY / 2.  Measured against chi2_f = -2 lp(tau = 1), which IS twice the
  halved value the epilogue multiplies, the halving term is not needed; measured against the
  chi2 that was summed it is, and a flat allowance fails: numpy itself on chi2 = 3 TINY,
  tau = 1e300 sits 2.5e-24 from E (tests/test_poly_range.py shows both).
The Gamma prior's bound (``gamma_bound``): s = shape - 1 as the double the kernel is handed,
E = s ln tau - tau rate: one ulp of log through s (2u |s ln tau|), one rounding each for
s log (u |s ln tau|), tau rate (u |tau rate|, or TINY / 2 subnormal) and the difference (u |E|):
u (3 |s ln tau| + |tau rate| + |E|) (1 + 8u) + TINY.

Where the result is not a finite number in double arithmetic -- tau is +-0, negative, inf or NaN,
chi^2 is not finite, or the product by tau overflows -- the roundings above are exact or
irrelevant and the device must return numpy's own value under the comparison rule."""
import math

import numpy as np

U = 2.0 ** -53
TINY = 2.0 ** -1074
MAXD = float(np.finfo(np.float64).max)
INF, NAN = float('inf'), float('nan')
POLYVAL = np.polynomial.polynomial.polyval

LADDER = np.array([0.0, -0.0, TINY, -TINY, 2.0 ** -1030, -2.0 ** -1030, 2.0 ** -537, -2.0 ** -537,
                   1.0, -1.0, 1.0 + 2.0 ** -52, -(1.0 - 2.0 ** -53), 0.3, -1.7,
                   2.0 ** 511, -2.0 ** 511, 2.0 ** 512, -2.0 ** 512, MAXD, -MAXD])
SMALL = LADDER[:8]                 # the square underflows: to 0, or to one quantum for 2^-537
MODERATE = LADDER[:14]             # |x| <= 1.7: no power up to 63 overflows
NONFINITE = np.array([INF, -INF, NAN])
EDGES = np.concatenate([LADDER, NONFINITE])

KMAXES = (4, 8, 16, 24, 33, 36, 48, 64)                 # BINF_KMAX_DISPATCH
K_LIST = (1, 2, 4, 5, 8, 9, 16, 17, 24, 25, 33, 34, 36, 37, 48, 49, 64)
CHI_K = (1, 5, 16, 33, 64)
# every route of the reduction at the smallest length that reaches it: the leaf with and without
# tail; H = 1, 2, 3 (the last length in the wave kernel); the block kernel; height 7; two chunks
N_LIST = (0, 1, 7, 8, 9, 129, 300, 600, 1025, 7689, 8193)
C_LIST = (1, 9, 70)                # at H = 0 a wave holds 8 rows: 9 spills one into the next
SHARED_N = (7, 129, 300, 600, 1025)
BAD_ROWS = (0, 3, 8)
FORWARD_N = len(LADDER) + 3
STRIDE_SHAPE = (4, 65536 + 300, 2)  # K, N, C: the grid-stride loops turn once N > 256 * 256

LOGP_ROUTES = ('gauss_err_logp', 'poly_gauss_logp', 'poly_gauss_logp_memo', 'poly_gauss_logp_memo reuse')
CHI2_ROUTES = ('row_sumsq_diff', 'row_sumsq_diff weights')
GAMMA_PARAMS = ((1.0, 0.2), (3.5, 3.5), (0.3, 7.0), (1.0, 0.0))
UPDATE_RATES = (0.0, 1.0, -1.0)

TAU_NAMED = (1.0 - 2.0 ** -53, 1.0 + 2.0 ** -52, 0.5, 2.5, math.e, TINY, 2.0 ** -1040, 2.0 ** -1022,
             1e-300, 1e300, MAXD)
TAU_BAD = (0.0, -0.0, -1.0, -TINY, INF, -INF, NAN)


def tau_random(n=200, seed=5):
    """n precisions log-uniform in [e^-700, e^700]."""
    return np.exp(np.random.RandomState(seed).uniform(-700.0, 700.0, size=n))


def tau_sets(C):
    """The precisions of the epilogue test: every named, bad and random value as a scalar (a
    launch each: the ``fin.tau`` branch) and in a per-chain vector (the ``tau_chain`` branch; all
    of them dealt over ceil(n / C) vectors, the last filled up from the front)."""
    rnd = tau_random()
    scalars = list(TAU_NAMED) + list(TAU_BAD) + list(rnd)
    pool = np.concatenate([TAU_NAMED, TAU_BAD, rnd])
    vectors = []
    for a in range(0, len(pool), C):
        v = pool[a:a + C]
        if len(v) < C:
            v = np.concatenate([v, pool[:C - len(v)]]) if len(pool) >= C else np.resize(pool, C)
        vectors.append(np.ascontiguousarray(v))
    return scalars, vectors


# ---------------------------------------------------------------------------
# the comparison rule
# ---------------------------------------------------------------------------
def same_bits(got, want):
    got = np.ascontiguousarray(got, dtype=np.float64)
    want = np.ascontiguousarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(got.view(np.int64)[~gn], want.view(np.int64)[~wn]))


def assert_same_bits(got, want, what):
    if not same_bits(got, want):
        got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
        if got.shape != want.shape:
            raise AssertionError('%s: shape %s, expected %s' % (what, got.shape, want.shape))
        nan = np.isnan(got) & np.isnan(want)
        bad = np.argwhere(~nan & ((np.isnan(got) != np.isnan(want)) | (got.view(np.int64) != want.view(np.int64))))
        i = tuple(bad[0])
        raise AssertionError('%s: %d of %d entries differ, first at %s: got %r, expected %r'
                             % (what, len(bad), got.size, i, float(got[i]), float(want[i])))


# ---------------------------------------------------------------------------
# references: numpy as the reference application writes it
# ---------------------------------------------------------------------------
def ref_forward(theta, xs):
    """[C x N]: numpy.polynomial.polynomial.polyval(xs, theta[c]) per chain."""
    with np.errstate(all='ignore'):
        return np.stack([POLYVAL(xs, theta[c]) for c in range(theta.shape[0])]).reshape(theta.shape[0], len(xs))


def ref_chi2(mock, ys, weights=None):
    with np.errstate(all='ignore'):
        d = mock - ys
        sq = d * d if weights is None else d * d / weights
        return np.array([np.sum(row) for row in sq])


def ref_logp(chi2, tau, N):
    """The Gaussian error model's log-prob as likelihood.py writes it, on a chi^2 already summed."""
    with np.errstate(all='ignore'):
        return -0.5 * chi2 * tau + N * 0.5 * np.log(tau)


def ref_err_grad(mock, ys, tau):
    with np.errstate(all='ignore'):
        return (mock - ys) * (tau[:, None] if np.ndim(tau) else tau)


def ref_gamma_logp(tau, shape, rate):
    with np.errstate(all='ignore'):
        return (shape - 1.0) * np.log(tau) - tau * rate


def ref_gamma_update(g, lp, rate):
    with np.errstate(all='ignore'):
        return g / (-lp + rate)


def ref_pairdist_chi2(x, ys):
    """chi^2 of all pair distances of [C x 3n] coordinates (summation order: this module's own;
    the epilogue test takes chi^2 from the backend's tau = 1 call, never from here)."""
    C, n = x.shape[0], x.shape[1] // 3
    I, J = np.triu_indices(n, 1)
    with np.errstate(all='ignore'):
        r = x.reshape(C, n, 3)
        d = np.sqrt(np.sum((r[:, I] - r[:, J]) ** 2, axis=2))
        return np.sum((d - ys) ** 2, axis=1)


class NumpyRoutes(object):
    """The backend interface, answered by the references themselves."""

    def forward(self, theta, xs):
        return ref_forward(theta, xs)

    def err_grad(self, mock, ys, tau):
        return ref_err_grad(mock, ys, tau)

    def chi2_of(self, route, case):
        """Raw chi^2 per chain as ``route`` sums it (kept for the last case: the epilogue test asks
        for the same sums at every precision)."""
        key = (id(case['mock']), id(case['ys']))
        if getattr(self, '_kept', (None, None))[0] != key:
            self._kept = (key, ref_chi2(case['mock'], case['ys']), case)
        return self._kept[1]

    def log_of(self, tau):
        with np.errstate(all='ignore'):
            return np.log(tau)

    def finish(self, chi2, tau, N):
        with np.errstate(all='ignore'):
            return -0.5 * chi2 * tau + N * 0.5 * self.log_of(tau)

    def logp_routes(self, case, tau):
        """{route: lp [C]} for LOGP_ROUTES; ``tau`` a float or a [C] array."""
        N = len(case['xs'])
        return dict((r, self.finish(self.chi2_of(r, case), tau, N)) for r in LOGP_ROUTES)

    def chi2_routes(self, case):
        """{route: chi^2 [C]} for CHI2_ROUTES on case['mock'], case['ys'], case['weights']."""
        return {'row_sumsq_diff': ref_chi2(case['mock'], case['ys']),
                'row_sumsq_diff weights': ref_chi2(case['mock'], case['ys'], case['weights'])}

    def pairdist_logp(self, x, ys, tau):
        return self.finish(ref_pairdist_chi2(x, ys), tau, len(ys))

    def gamma_logp(self, tau, shape, rate):
        return ref_gamma_logp(tau, shape, rate)

    def gamma_update(self, g, lp, rate):
        return ref_gamma_update(g, lp, rate)


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------
def _mix(rs, pool, shape, share=0.5):
    """A share of the entries from ``pool``, the rest N(0, 1)."""
    v = rs.choice(pool, size=shape)
    z = rs.standard_normal(shape)
    return np.where(rs.uniform(size=shape) < share, v, z)


# class F weights: positive and mild, so that every datum's d * d / w is seen in the sum's bits
F_WEIGHTS = np.array([1.0, 1.0 + 2.0 ** -52, 1.0 - 2.0 ** -53, 0.3, 1.7, 2.0 ** -10, 2.0 ** 10])
# one weight of a class F case replaced by each of these (``check_weight_edges``)
WEIGHT_EDGES = np.array([0.0, -0.0, TINY, -TINY, 2.0 ** -1030, -1.7, MAXD, -MAXD, INF, -INF, NAN])


def _finish_case(theta, xs, ys, rs, cls='O'):
    """Weights of d * d / w.  Class F: positive and finite, half from F_WEIGHTS, half exp(N(0, 1)),
    so that the weighted chi^2 is a finite number; class O: the whole ladder, zero, subnormal and
    negative weights included (d * d / 0, +inf meeting -inf)."""
    if cls == 'F':
        w = np.where(rs.uniform(size=len(xs)) < 0.5, rs.choice(F_WEIGHTS, size=len(xs)),
                     np.exp(rs.standard_normal(len(xs))))
    else:
        w = rs.choice(LADDER, size=len(xs))
    case = {'theta': np.ascontiguousarray(theta), 'xs': np.ascontiguousarray(xs),
            'ys': np.ascontiguousarray(ys), 'weights': np.ascontiguousarray(w)}
    case['mock'] = ref_forward(case['theta'], case['xs'])
    return case


def case(cls, K, N, C, seed=0, small_ys=False):
    rs = np.random.RandomState(1000003 * seed + 10007 * K + 13 * N + C + (500 if cls == 'O' else 0))
    if cls == 'F':
        theta, xs = _mix(rs, MODERATE, (C, K), 0.3), _mix(rs, MODERATE, N)
        ys = rs.choice(SMALL, size=N) if small_ys else _mix(rs, MODERATE, N)
        if small_ys:
            # tiny chains: mock = c0 = +-2^-537 or +-2^-536, squared residuals 0, 1, 4 or 9 quanta.
            # A chain at 2^-536 gets an odd quantum only from a y = +-2^-537: an odd number of those
            if N >= 1 and np.sum(np.abs(ys) == 2.0 ** -537) % 2 == 0:
                ys[0] = TINY if abs(ys[0]) == 2.0 ** -537 else 2.0 ** -537
            for c in range(0, C, 3):
                theta[c] = 0.0
                theta[c, 0] = (2.0 ** -537, -2.0 ** -537, 2.0 ** -536, -2.0 ** -536)[(c // 3) % 4]
    elif cls == 'O':
        theta, xs = _mix(rs, LADDER, (C, K)), _mix(rs, LADDER, N)
        ys = _mix(rs, np.concatenate([LADDER, [INF, -INF]]), N)
        fixed = (INF, -INF, 0.3)
        ys[:len(fixed)] = fixed[:N]
        fixed = (1.0, -1.7, 2.0 ** 512, -MAXD, 0.0, -2.0 ** 511, 2.0 ** -537)
        xs[:len(fixed)] = fixed[:N]
        for c in range(2, C, 3):                    # constant chains: finite mock data
            theta[c] = 0.0
            theta[c, 0] = rs.choice(LADDER)
        if C >= 2 and K >= 2:                       # mock data +inf, -inf by the sign of x, NaN at x = 0
            theta[1] = rs.standard_normal(K)
            theta[1, -1] = INF
    else:
        raise ValueError(cls)
    return _finish_case(theta, xs, ys, rs, cls)


def forward_case(cls, K, C=9, seed=0):
    """N = len(LADDER) + 3 with xs from the ladder (class F: its moderate entries, the rest
    N(0, 1)); the last chain all -0.0, the one before all +0.0: the sign of a zero result."""
    rs = np.random.RandomState(77 + 131 * K + seed + (500 if cls == 'O' else 0))
    pool = MODERATE if cls == 'F' else LADDER
    xs = np.concatenate([pool, rs.standard_normal(FORWARD_N - len(pool))])
    theta = _mix(rs, pool, (C, K))
    if cls == 'O' and C >= 2 and K >= 2:
        theta[1] = rs.standard_normal(K)
        theta[1, -1] = INF
    if C >= 4:
        theta[C - 1] = -0.0
        theta[C - 2] = 0.0
    ys = _mix(rs, pool, FORWARD_N)
    return _finish_case(theta, xs, ys, rs, cls)


def stride_case():
    K, N, C = STRIDE_SHAPE
    rs = np.random.RandomState(65536)
    xs = np.resize(np.concatenate([MODERATE, rs.standard_normal(83)]), N)
    return _finish_case(_mix(rs, MODERATE, (C, K)), xs, np.resize(_mix(rs, EDGES, 1021), N), rs, 'F')


def spoil(case_f, what, index, value):
    """Class X: ``case_f`` with one entry of a chain's coefficient row (what = 'theta', index =
    (row, k)), of xs or of ys (index = n) replaced by ``value``."""
    c = dict((k, v.copy()) for k, v in case_f.items())
    c[what][index] = value
    c['mock'] = ref_forward(c['theta'], c['xs'])
    return c


def class_f_holds(case_f):
    """Mock data, chi^2 and weighted chi^2 finite; at least half of the chi^2 values, and of the
    weighted ones, nonzero and pairwise distinct."""
    ok = bool(np.all(np.isfinite(case_f['mock'])) and np.all(np.isfinite(case_f['weights']))
              and np.all(case_f['weights'] > 0.0))
    for w in (None, case_f['weights']):
        chi2 = ref_chi2(case_f['mock'], case_f['ys'], w)
        nz = chi2[chi2 != 0.0]
        ok = ok and bool(np.all(np.isfinite(chi2)) and 2 * len(np.unique(nz)) >= len(chi2))
    return ok


def class_o_holds(case_o):
    mock, chi2 = case_o['mock'], ref_chi2(case_o['mock'], case_o['ys'])
    finite_in = np.all(np.isfinite(case_o['theta']), axis=1)
    return bool(np.any(mock == INF) and np.any(mock == -INF) and np.any(np.isnan(mock))
                and np.any(mock[finite_in] == INF) and np.any(mock[finite_in] == -INF)
                and np.any(chi2 == INF) and np.any(np.isnan(chi2)))


def err_grad_case(C):
    """mock x ys over all pairs of LADDER u NONFINITE (chain c rolls the mock values by c), and the
    precisions: every edge as a scalar, and per chain (C of them from a fixed permutation)."""
    n = len(EDGES)
    ys = np.tile(EDGES, n)
    mock = np.stack([np.repeat(np.roll(EDGES, c), n) for c in range(C)])
    perm = np.random.RandomState(9).permutation(n)
    vectors = [np.ascontiguousarray(EDGES[np.roll(perm, s)[:C]]) for s in (0, 8, 16)]
    return mock, ys, list(EDGES), vectors


def gamma_taus(C):
    """C = 1: every edge on its own; otherwise the edges, then log-uniform fill."""
    if C == 1:
        return [np.array([t]) for t in EDGES]
    rs = np.random.RandomState(C)
    return [np.concatenate([EDGES, np.exp(rs.uniform(-700.0, 700.0, size=C - len(EDGES)))])]


def update_pairs():
    n = len(EDGES)
    return np.repeat(EDGES, n), np.tile(EDGES, n)


def pairdist_case(cls, C=9, seed=0):
    """5 beads, all 10 pairs."""
    rs = np.random.RandomState(31 + seed + (500 if cls == 'O' else 0))
    pool = MODERATE if cls == 'F' else LADDER
    x = _mix(rs, pool, (C, 15))
    ys = np.abs(_mix(rs, pool, 10))
    I, J = np.triu_indices(5, 1)
    return {'x': np.ascontiguousarray(x), 'ys': np.ascontiguousarray(ys),
            'pair_i': I.astype(np.int32), 'pair_j': J.astype(np.int32)}


# ---------------------------------------------------------------------------
# bounds, in mpmath at 50 digits (per-chain scalars only)
# ---------------------------------------------------------------------------
_mp = None


def mp():
    global _mp
    if _mp is None:
        import mpmath
        _mp = mpmath.mp.clone()
        _mp.dps = 50
    return _mp


_exact_cache = {}
_ln_cache = {}


def exact_logp(chi2, tau, N):
    """(E, bound) as mpmath numbers for finite chi2 >= 0 and finite tau > 0."""
    key = (float(chi2), float(tau), int(N))
    hit = _exact_cache.get(key)
    if hit is None:
        M = mp()
        t = M.mpf(key[1])
        A = M.mpf(key[0]) * t / 2
        ln = _ln_cache.get(key[1])
        if ln is None:
            if len(_ln_cache) > 100000:
                _ln_cache.clear()
            ln = _ln_cache[key[1]] = M.log(t)
        B = M.mpf(key[2]) / 2 * abs(ln)
        E = -A + M.mpf(key[2]) / 2 * ln
        bound = M.mpf(U) * (A + 3 * B + abs(E)) * (1 + 8 * M.mpf(U)) + M.mpf(TINY) * (t / 2 + 1)
        if len(_exact_cache) > 400000:
            _exact_cache.clear()
        hit = _exact_cache[key] = (E, bound)
    return hit


def logp_bound(chi2, tau, N):
    return exact_logp(chi2, tau, N)[1]


def exact_gamma(tau, shape, rate):
    """(E, bound) for finite tau > 0; s = shape - 1 as the double the kernel is handed."""
    M = mp()
    t, s, r = M.mpf(float(tau)), M.mpf(float(shape) - 1.0), M.mpf(float(rate))
    sl, tr = abs(s * M.log(t)), abs(t * r)
    E = s * M.log(t) - t * r
    return E, M.mpf(U) * (3 * sl + tr + abs(E)) * (1 + 8 * M.mpf(U)) + M.mpf(TINY)


def gamma_bound(tau, shape, rate):
    return exact_gamma(tau, shape, rate)[1]


def fraction(got, E, bound):
    """|got - E| / bound as a float (got finite)."""
    M = mp()
    return float(abs(M.mpf(float(got)) - E) / bound)


def epilogue_fractions(got, chi2, tau, N, what):
    """One route's log-probs against the rule of the module docstring: numpy's own value, bit
    for bit, where the result is not finite in double arithmetic; inside ``logp_bound`` of exact
    arithmetic elsewhere.  Returns (worst fraction, chains held to the bound)."""
    got, chi2 = np.asarray(got, dtype=np.float64), np.asarray(chi2, dtype=np.float64)
    tau = np.broadcast_to(np.asarray(tau, dtype=np.float64), got.shape)
    with np.errstate(all='ignore'):
        prod = -0.5 * chi2 * tau
    bounded = (tau > 0.0) & np.isfinite(tau) & np.isfinite(chi2) & np.isfinite(prod)
    own = ref_logp(chi2, tau, N)
    assert_same_bits(got[~bounded], own[~bounded], what + ': not finite in double arithmetic')
    worst = 0.0
    for c in np.flatnonzero(bounded):
        if not np.isfinite(got[c]):
            raise AssertionError('%s: chain %d: %r where exact arithmetic is finite (chi2 %r, tau %r)'
                                 % (what, c, float(got[c]), float(chi2[c]), float(tau[c])))
        E, bound = exact_logp(chi2[c], tau[c], N)
        f = fraction(got[c], E, bound)
        if not f <= 1.0:
            raise AssertionError('%s: chain %d: chi2 %r tau %r N %d: %r is %.3g of the bound from exact %s'
                                 % (what, c, float(chi2[c]), float(tau[c]), N, float(got[c]), f, mp().nstr(E, 20)))
        worst = max(worst, f)
    return worst, int(bounded.sum())


# ---------------------------------------------------------------------------
# the assertion functions
# ---------------------------------------------------------------------------
def check_forward(be, cs, what=''):
    """(a) poly_forward equals POLYVAL bit for bit."""
    assert_same_bits(be.forward(cs['theta'], cs['xs']), cs['mock'], 'poly_forward %s' % what)


def check_forward_spoiled(be, case_f, what=''):
    """(a), class X: a non-finite coefficient stays in its chain (rows 0, 3 and the last; first,
    middle and last coefficient), a non-finite xs[n] makes column n NaN in every chain and leaves
    every other column its class F bits; numpy's bits throughout."""
    C, K = case_f['theta'].shape
    N = len(case_f['xs'])
    got_f = be.forward(case_f['theta'], case_f['xs'])
    assert_same_bits(got_f, case_f['mock'], 'poly_forward F %s' % what)
    assert np.all(np.isfinite(got_f))
    for value in NONFINITE:
        for row in sorted(set((0, min(3, C - 1), C - 1))):
            for k in sorted(set((0, K // 2, K - 1))):
                x = spoil(case_f, 'theta', (row, k), value)
                got = be.forward(x['theta'], x['xs'])
                at = 'poly_forward X %s theta[%d, %d] = %r' % (what, row, k, value)
                assert_same_bits(got, x['mock'], at)
                others = np.arange(C) != row
                assert_same_bits(got[others], got_f[others], at + ', other chains')
                assert not np.all(np.isfinite(got[row])), at
        for n in sorted(set((0, N // 2, N - 1))):
            x = spoil(case_f, 'xs', n, value)
            got = be.forward(x['theta'], x['xs'])
            at = 'poly_forward X %s xs[%d] = %r' % (what, n, value)
            assert_same_bits(got, x['mock'], at)
            others = np.arange(N) != n
            assert np.all(np.isnan(got[:, n])), at
            assert_same_bits(got[:, others], got_f[:, others], at + ', other columns')


def check_err_grad(be, mock, ys, tau, what=''):
    """(b) gauss_err_grad equals (mock - ys) * tau bit for bit."""
    assert_same_bits(be.err_grad(mock, ys, tau), ref_err_grad(mock, ys, tau), 'gauss_err_grad %s' % what)


def check_chi2_unit(be, cs, what='', poly_only=False):
    """(c) every route at tau = 1 equals numpy's expression bit for bit."""
    N = len(cs['xs'])
    with np.errstate(all='ignore'):
        want = np.array([-0.5 * np.sum((cs['mock'][c] - cs['ys']) ** 2) * 1.0 + N * 0.5 * np.log(1.0)
                         for c in range(cs['mock'].shape[0])])
    got = be.logp_routes(cs, 1.0)
    for r in LOGP_ROUTES:
        if poly_only and r == 'gauss_err_logp':
            continue
        assert_same_bits(got[r], want, '%s at tau = 1 %s' % (r, what))
    if not poly_only:
        got = be.chi2_routes(cs)
        assert_same_bits(got['row_sumsq_diff'], ref_chi2(cs['mock'], cs['ys']), 'row_sumsq_diff %s' % what)
        assert_same_bits(got['row_sumsq_diff weights'], ref_chi2(cs['mock'], cs['ys'], cs['weights']),
                         'row_sumsq_diff weights %s' % what)
    return got


def check_weight_edges(be, case_f, what=''):
    """Class F with ONE weight replaced by a zero, a subnormal, a negative, the largest double, an
    infinity or NaN: d * d / w of that datum alone leaves the finite range, the weighted sum is
    numpy's -- +-inf, NaN (0 / 0, or a NaN weight) or the finite sum -- bit for bit."""
    N = len(case_f['xs'])
    for j, value in enumerate(WEIGHT_EDGES):
        x = spoil(case_f, 'weights', (j * 5 + N // 2) % N, value)
        got = be.chi2_routes(x)['row_sumsq_diff weights']
        assert_same_bits(got, ref_chi2(x['mock'], x['ys'], x['weights']),
                         'row_sumsq_diff weights %s: one weight = %r' % (what, value))


def check_containment(be, case_f, what=''):
    """(d) a non-finite chain (rows 0, 3, 8; NaN, inf, -inf in one coefficient) or a chain with a
    non-finite mock datum leaves the other rows of every route their class F bits, and is itself
    what numpy says."""
    C, K = case_f['theta'].shape
    base = dict(be.logp_routes(case_f, 1.0))
    base.update(be.chi2_routes(case_f))
    for r in LOGP_ROUTES:
        assert np.all(np.isfinite(base[r])), (r, what)
    N = len(case_f['xs'])
    for j, row in enumerate(BAD_ROWS):
        value = NONFINITE[(j + 2) % 3]              # NaN, inf, -inf
        x = spoil(case_f, 'theta', (row, (j * K) // 3), value)
        assert not np.all(np.isfinite(x['mock'][row]))
        got = dict(be.logp_routes(x, 1.0))
        got.update(be.chi2_routes(x))
        others = np.arange(C) != row
        want = ref_logp(ref_chi2(x['mock'], x['ys']), 1.0, N)
        for r in LOGP_ROUTES + CHI2_ROUTES:
            at = '%s %s: chain %d spoiled with %r' % (r, what, row, value)
            assert_same_bits(got[r][others], base[r][others], at + ', other chains')
            if r in LOGP_ROUTES:
                assert_same_bits(got[r], want, at)
            else:
                assert np.all(np.isfinite(base[r])), at
                assert_same_bits(got[r], ref_chi2(x['mock'], x['ys'], x['weights'] if 'weights' in r else None), at)
            assert not np.isfinite(got[r][row]), at


def check_bad_datum(be, case_f, what=''):
    """Class X with a bad xs[n] (every log-prob NaN) and a bad ys[n] (numpy's NaN / -inf)."""
    N = len(case_f['xs'])
    for value in NONFINITE:
        for field in ('xs', 'ys'):
            x = spoil(case_f, field, N // 2, value)
            got = be.logp_routes(x, 1.0)
            want = ref_logp(ref_chi2(x['mock'], x['ys']), 1.0, N)
            for r in LOGP_ROUTES:
                at = '%s %s: %s[%d] = %r' % (r, what, field, N // 2, value)
                assert_same_bits(got[r], want, at)
                if field == 'xs':
                    assert np.all(np.isnan(got[r])), at


def check_epilogue(be, cs, what='', scalars=None, vectors=None):
    """(e) every log-prob route at general tau, scalar and per chain, against exact arithmetic on
    chi2_f = -2 lp(tau = 1) of the route's own tau = 1 call.  Returns {route: worst fraction}."""
    C = cs['theta'].shape[0]
    N = len(cs['xs'])
    if scalars is None:
        scalars, vectors = tau_sets(C)
    unit = be.logp_routes(cs, 1.0)
    chi2_f = dict((r, -2.0 * unit[r]) for r in LOGP_ROUTES)
    worst = dict((r, 0.0) for r in LOGP_ROUTES)
    held = 0
    for tau in list(scalars) + list(vectors):
        got = be.logp_routes(cs, tau)
        for r in LOGP_ROUTES:
            f, n = epilogue_fractions(got[r], chi2_f[r], tau, N, '%s %s tau %s' % (r, what, 'per chain' if np.ndim(tau) else repr(tau)))
            worst[r] = max(worst[r], f)
            held += n
    return worst, held


def check_epilogue_pairdist(be, pc, what=''):
    C = pc['x'].shape[0]
    scalars, vectors = tau_sets(C)
    chi2_f = -2.0 * be.pairdist_logp(pc['x'], pc['ys'], 1.0)
    worst, held = 0.0, 0
    for tau in list(scalars) + list(vectors):
        got = be.pairdist_logp(pc['x'], pc['ys'], tau)
        f, n = epilogue_fractions(got, chi2_f, tau, len(pc['ys']), 'pairdist_gauss_logp %s tau %s'
                                  % (what, 'per chain' if np.ndim(tau) else repr(tau)))
        worst, held = max(worst, f), held + n
    return worst, held


def check_gamma_logp(be, tau, shape, rate, what=''):
    """(f) gamma_logp inside ``gamma_bound`` of exact arithmetic where tau is finite and positive
    and tau * rate does not overflow; numpy's own value elsewhere.  Returns the worst fraction."""
    tau = np.asarray(tau, dtype=np.float64)
    got = be.gamma_logp(tau, shape, rate)
    own = ref_gamma_logp(tau, shape, rate)
    with np.errstate(all='ignore'):
        bounded = (tau > 0.0) & np.isfinite(tau) & np.isfinite(tau * rate)
    at = 'gamma_logp %s shape %r rate %r' % (what, shape, rate)
    assert_same_bits(got[~bounded], own[~bounded], at + ': not finite in double arithmetic')
    worst = 0.0
    for c in np.flatnonzero(bounded):
        assert np.isfinite(got[c]), (at, c, tau[c])
        E, bound = exact_gamma(tau[c], shape, rate)
        f = fraction(got[c], E, bound)
        if not f <= 1.0:
            raise AssertionError('%s: tau %r: %r is %.3g of the bound from exact %s'
                                 % (at, float(tau[c]), float(got[c]), f, mp().nstr(E, 20)))
        worst = max(worst, f)
    return worst


def check_gamma_update(be, g, lp, rate, what=''):
    """(g) gamma_precision_update equals g / (-lp + rate) bit for bit."""
    assert_same_bits(be.gamma_update(g, lp, rate), ref_gamma_update(g, lp, rate),
                     'gamma_precision_update %s rate %r' % (what, rate))


# ---------------------------------------------------------------------------
# restatements of the kernels, for the CPU file: as written, and mutated
# ---------------------------------------------------------------------------
def kmax_of(K):
    return [m for m in KMAXES if K <= m][0]


def horner_padded(theta, xs, fold=False, pad_next=False):
    """Horner<KMAX> of csrc/poly.hip for every chain: coefficients above K - 1 are zero, the
    recurrence runs over all KMAX.  ``fold``: x * 0.0 folded to 0.0.  ``pad_next``: the padding
    reads on into the next chain's coefficients (the last chain's clamp at the end of the array)."""
    C, K = theta.shape
    KM = kmax_of(K)
    flat = theta.reshape(-1)
    out = np.empty((C, len(xs)))
    with np.errstate(all='ignore'):
        for c in range(C):
            if pad_next:
                idx = np.minimum(c * K + np.arange(KM), flat.size - 1)
                co = flat[idx]
            else:
                co = np.concatenate([theta[c], np.zeros(KM - K)])
            v = co[KM - 1] + (np.zeros(len(xs)) if fold else xs * 0.0)
            for i in range(KM - 2, -1, -1):
                v = co[i] + v * xs
            out[c] = v
    return out


class KernelRestated(NumpyRoutes):
    """numpy, with the forward model as the kernel evaluates it (padded Horner)."""

    def forward(self, theta, xs):
        return horner_padded(theta, xs)


class FoldedHorner(NumpyRoutes):
    def forward(self, theta, xs):
        return horner_padded(theta, xs, fold=True)


class PadsWithNextChain(NumpyRoutes):
    def forward(self, theta, xs):
        return horner_padded(theta, xs, pad_next=True)


class SloppyLog(NumpyRoutes):
    """A log good to 1e-13, relative."""

    def log_of(self, tau):
        with np.errstate(all='ignore'):
            return np.log(tau) * (1.0 + 1e-13)


class OneDatumShort(NumpyRoutes):
    """(N - 1) / 2 in place of N / 2."""

    def finish(self, chi2, tau, N):
        with np.errstate(all='ignore'):
            return -0.5 * chi2 * tau + (N - 1) * 0.5 * np.log(tau)


class LeakyReduction(NumpyRoutes):
    """A row whose sum is not finite moves the last bit of the row after it."""

    @staticmethod
    def _leak(chi2):
        chi2 = chi2.copy()
        for c in np.flatnonzero(~np.isfinite(chi2)):
            n = (c + 1) % len(chi2)
            if np.isfinite(chi2[n]):
                chi2[n] = np.nextafter(chi2[n], INF)
        return chi2

    def chi2_of(self, route, case):
        return self._leak(ref_chi2(case['mock'], case['ys']))

    def chi2_routes(self, case):
        return dict((k, self._leak(v)) for k, v in NumpyRoutes.chi2_routes(self, case).items())


class WeightedTailDropped(NumpyRoutes):
    """A weighted reduction that forgets the leaf's tail (the last N % 8 elements)."""

    def chi2_routes(self, case):
        r = NumpyRoutes.chi2_routes(self, case)
        n = len(case['ys']) - len(case['ys']) % 8
        r['row_sumsq_diff weights'] = ref_chi2(case['mock'][:, :n], case['ys'][:n], case['weights'][:n])
        return r


class WrongWeight(NumpyRoutes):
    """d[i] * d[i] / w[i - 1]."""

    def chi2_routes(self, case):
        r = NumpyRoutes.chi2_routes(self, case)
        r['row_sumsq_diff weights'] = ref_chi2(case['mock'], case['ys'], np.roll(case['weights'], 1))
        return r


class WeightedOtherOrder(NumpyRoutes):
    """The weighted terms added up one after the other instead of pairwise."""

    def chi2_routes(self, case):
        r = NumpyRoutes.chi2_routes(self, case)
        with np.errstate(all='ignore'):
            d = case['mock'] - case['ys']
            r['row_sumsq_diff weights'] = np.array([float(np.cumsum(row)[-1]) if len(row) else 0.0
                                                    for row in d * d / case['weights']])
        return r
