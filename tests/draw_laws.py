"""Host helpers of the law tests of the device draw streams (``tests/test_draw_laws.py`` on
the CPU, ``tests/test_gpu_draw_laws.py`` on the device).  numpy, scipy and mpmath only (the
whole-stream statistics are written in torch so that they can run where a 2^26 array lies);
nothing here calls into the library.

``tests/draw_streams.py`` restates every stream and the device equals it bit for bit; both
were written from the same reading of the papers.  Here every stream is held to its LAW:
statistics with known null laws, intervals from closed forms, the committed ziggurat table
and scipy / mpmath quantiles, nothing from device output or from the restatement's samples.

Statistics (each a dict like ``stationarity``'s: name, kind, value, lo, hi)
---------------------------------------------------------------------------
dkw       sup |F_n - F| of a probability-integral transform against U(0, 1), threshold
          ``sqrt(log(2 / alpha) / (2 n))`` (``stationarity.dkw``); valid for every n.
count     a region count in its EXACT binomial interval (``scipy.stats.binom.ppf / isf`` at
          alpha / 2 each side).
hoeffding a sum of independent indicators with DIFFERENT known probabilities (the slow elements
          that end inside their first candidate's wedge interval s [X_{i+1}, X_i]: probability
          ``q_i = a_i + (1 - a_i) (Phi(X_i) - Phi(X_{i+1}))``): mean +- ``sqrt(n log(2 / alpha) / 2)``,
          Hoeffding's bound, valid for every n like DKW.  The pooled PIT is blunt against a wedge
          test that always accepts (the value stays uniform in a narrow interval); this is not.
exact     a count that is 0 under the null with certainty (a value outside [0, 1), a gamma
          draw that is not positive, a tail value whose sign is not its candidate's).
indep     two PIT-uniform arrays v, w: ``(v - w) mod 1`` and ``(v + w) mod 1`` are both U(0, 1)
          when v and w are independent (one uniform summand suffices), a DKW each.  w = v puts
          the difference at 0, w = 1 - v the sum.  The pairs are always DISJOINT (elements
          2g / 2g+1, not e / e+1 for every e), so that the transformed sample is i.i.d. as
          the DKW bound requires.

The conditional law of a slow ziggurat element
----------------------------------------------
An element whose FIRST candidate (layer i, sign s: from the generator's words alone,
``Draws.first_layer / first_sign / first_slow``) failed the fast test ends as follows.

layer i >= 1   the candidate x = s |x| is uniform on s [X_{i+1}, X_i]; the wedge test accepts
               it with probability ``a_i`` = (area under f - f(X_i) there) / (rectangle
               (X_i - X_{i+1}) (f(X_{i+1}) - f(X_i))), and an accepted x has the density
               ``~ f(x) - f(X_i)``, CDF ``W_{i,s}``.  A rejected candidate is replaced by a
               fresh run of the whole algorithm, N(0, 1).  So the final value has the CDF
               ``a_i W_{i,s}(x) + (1 - a_i) Phi(x)``.
layer 0        the value is s |X| with ``P(|X| <= x) = 1 - sf(x) / sf(R)``, x >= R.

That mixture formula and the table together are checked without any sample: summed over the
layers it must give Phi (``algorithm_law``).  The PIT of every slow element is U(0, 1).

The closed forms are float64: with ``Q = ndtr(-x)`` (upper tails: the smaller numbers),

    A_i(t) = sqrt(2 pi) (Q(X_{i+1}) - Q(t)) - f(X_i) (t - X_{i+1}),   W = A_i(t) / A_i(X_i).

Cancellation.  Both terms of A_i are about a rectangle's area while their difference is a
wedge's.  With ndtr within ``NDTR_ULP`` = 4 ulp (hypothesis; ``EPS`` = 2^-52 relative), exp
within 1 ulp and every other operation correctly rounded,

    |dA_i(t)| <= EPS [ (NDTR_ULP + 1) sqrt(2 pi) (Q(X_{i+1}) + Q(t)) + 3 f(X_i) (t - X_{i+1}) ],

which ``cancellation_bound`` evaluates at t = X_i for every layer: at most 7.4e-10 of a wedge's
area (layer 765; the wedges of the middle layers are the smallest, about 1e-7, against
rectangles of 5e-4: 1e-11 holds only for the outermost layers).  The PIT carries
a_i (dA(t) + W dA(X_i)) / A_i <= 2 x that, 1.5e-9 -- against a smallest DKW threshold of 4.2e-4.
``tests/test_draw_laws.py`` measures the error against ``mpmath.quad`` (1.4e-10).

``CASES`` is THE table of settings (the analogue of ``stationarity.ROUTES``): stream, seed,
offset, shape, n and the mutants that apply.  The CPU power table and the device tests both read
it, so a device test cannot drift to a setting whose power was never shown.  Levels: every test
function has the total level ``ALPHA`` = 1e-9, split evenly (Bonferroni) over its cases and over
each case's ``nstat`` statistics (``alpha_of``).

Mutants (``defect=`` of tests/draw_streams.py) and what sees them: see the power table in
tests/test_draw_laws.py's docstring.  ``tail_sign`` is not among them: the law is symmetric, so
it is no law mutant -- no statistic of the values alone sees it; only what is conditional on the
candidate's sign does (the ``exact`` sign check, and the tail's PIT, taken on the candidate's side).
"""
import math

import numpy as np
import mpmath
from scipy import special, stats

import draw_streams as ds
from stationarity import ALPHA, MARGIN, dkw, dkw_threshold, z_of, unit_interval, inside, describe  # noqa: F401

f64 = np.float64
EPS = ds.EPS
NDTR_ULP = 4.0
SQ2PI = math.sqrt(2.0 * math.pi)
R = ds.TAIL_R

_X = ds.ZX
_F = np.exp(-0.5 * _X * _X)
_Q = special.ndtr(-_X)
_DX = _X[:-1] - _X[1:]                                      # [i] = X_i - X_{i+1}
AREA = SQ2PI * (_Q[1:] - _Q[:-1]) - _F[:-1] * _DX           # [i] = A_i(X_i), i >= 1
RECT = _DX * (_F[1:] - _F[:-1])
WEDGE_SHARE = AREA / RECT                                   # a_i, i >= 1
WEDGE_SHARE[0] = 0.0                                        # layer 0 has the tail instead
# a candidate is slow unless |u| < X_{i+1} / X_i, the layer uniform over the 1024
P_SLOW = float(np.mean(1.0 - ds.ZR))
P_TAIL = float(stats.norm.sf(R))                            # one side


def cancellation_bound():
    """max over the layers of |dA_i(X_i)| / A_i(X_i) as derived in the module docstring, and
    the layer where it is attained."""
    i = np.arange(1, 1024)
    dA = EPS * ((NDTR_ULP + 1.0) * SQ2PI * (_Q[i + 1] + _Q[i]) + 3.0 * _F[i] * _DX[i])
    rel = dA / AREA[i]
    return float(rel.max()), int(i[np.argmax(rel)])


# ---------------------------------------------------------------------------
# probability-integral transforms
# ---------------------------------------------------------------------------
def zig_slow_pit(z, layer, sign):
    """The PIT of slow ziggurat elements: final values ``z``, first candidate's ``layer`` and
    ``sign`` (-1 / +1)."""
    z = np.asarray(z, dtype=f64)
    i = np.asarray(layer, dtype=np.int64)
    s = np.asarray(sign, dtype=f64)
    t = s * z
    lo, hi = _X[i + 1], _X[i]
    tc = np.clip(t, lo, hi)
    wp = np.clip((SQ2PI * (_Q[i + 1] - special.ndtr(-tc)) - _F[i] * (tc - lo)) / AREA[i], 0.0, 1.0)
    w = np.where(s > 0, wp, 1.0 - wp)
    a = WEDGE_SHARE[i]
    wedge = a * w + (1.0 - a) * special.ndtr(z)
    g = np.where(t >= R, 1.0 - special.ndtr(-np.maximum(t, R)) / special.ndtr(-R), 0.0)
    return np.where(i == 0, np.where(s > 0, g, 1.0 - g), wedge)


def zig_slow_pit_mp(z, layer, sign, dps=30):
    """The same by ``mpmath.quad`` of the densities (one point)."""
    with mpmath.workdps(dps):
        z, s = mpmath.mpf(float(z)), int(sign)
        t = s * z
        if layer == 0:
            r = mpmath.mpf(R)
            g = 1 - mpmath.ncdf(-t) / mpmath.ncdf(-r) if t >= r else mpmath.mpf(0)
            return g if s > 0 else 1 - g
        lo, hi = mpmath.mpf(float(_X[layer + 1])), mpmath.mpf(float(_X[layer]))
        fh = mpmath.exp(-hi * hi / 2)

        def dens(x):
            return mpmath.exp(-x * x / 2) - fh
        area = mpmath.quad(dens, [lo, hi])
        tc = min(max(t, lo), hi)
        wp = mpmath.quad(dens, [lo, tc]) / area
        w = wp if s > 0 else 1 - wp
        a = area / ((hi - lo) * (mpmath.exp(-lo * lo / 2) - fh))
        return a * w + (1 - a) * mpmath.ncdf(z)


def algorithm_law(xs, dps=50):
    """The law of the ziggurat AS WRITTEN, from the committed table, in mpmath; no sample.
    Per point x >= 0 the parts of [0, x] in area units -- layer i >= 1: the fast part
    ``min(x, X_{i+1}) (f(X_{i+1}) - f(X_i))`` and the wedge part ``slow_i a_i W_i(x)`` x rectangle
    (the mixture formula of the module docstring); layer 0: ``min(x, R) f(R)`` and the tail
    ``T (1 - sf(x) / sf(R))``, T the density's area beyond R.  Returns, per x,

      identity   |sum of the parts / sqrt(2 pi) + 1/2 - Phi(x)|: the parts telescope to the area
                 under f whatever the edges are, so this is arithmetic (the mixture formula, a_i,
                 W_i, the tail law, monotone edges down to X_1024 = 0, X_1 = R);
      law        |F(x) - Phi(x)| of the algorithm's own output: each layer is chosen with
                 probability 1/1024, so its parts are divided by its OWN area v_i = X_i (f(X_{i+1})
                 - f(X_i)) (v_0 = X_0 f(R)), and the sum by its total (the acceptance mass).
                 The table holds doubles, so the v_i agree to their rounding only
                 (``draw_streams.check_tables``: area_spread) and F - Phi is of that order, not 0."""
    with mpmath.workdps(dps):
        X = [mpmath.mpf(float(v)) for v in _X]
        F = [mpmath.exp(-x * x / 2) for x in X]
        P = [mpmath.ncdf(x) for x in X]
        s2 = mpmath.sqrt(2 * mpmath.pi)
        half = mpmath.mpf(1) / 2
        r, sfr = X[1], mpmath.ncdf(-X[1])
        T = s2 * sfr
        lay = []                                           # (lo, hi, df, f(X_i), Phi(lo), rectangle, a_i, area, v_i)
        for i in range(1, 1024):
            lo, hi, df = X[i + 1], X[i], F[i + 1] - F[i]
            area = s2 * (P[i] - P[i + 1]) - F[i] * (hi - lo)
            rect = (hi - lo) * df
            lay.append((lo, hi, df, F[i], P[i + 1], rect, area / rect, area, X[i] * df))

        def parts(x, phi):
            """x = None: the whole half line."""
            ident = alg = mpmath.mpf(0)
            for lo, hi, df, fi, plo, rect, a, area, v in lay:
                if x is None or x >= hi:
                    part = lo * df + rect * a              # W = 1
                elif x <= lo:
                    part = x * df                          # W = 0
                else:
                    part = lo * df + rect * a * ((s2 * (phi - plo) - fi * (x - lo)) / area)
                ident += part
                alg += part / v
            inside = r if x is None or x >= r else x
            tail = mpmath.mpf(1) if x is None else ((1 - mpmath.ncdf(-x) / sfr) if x > r else mpmath.mpf(0))
            ident += inside * F[1] + T * tail
            alg += inside / X[0] + (1 - r / X[0]) * tail   # layer 0 as drawn: fast iff |u| X_0 < R
            return ident, alg
        mass = parts(None, None)[1]
        res = []
        for x in xs:
            x = mpmath.mpf(float(x))
            phi = mpmath.ncdf(x)
            ident, alg = parts(x, phi)
            res.append((float(abs(ident / s2 + half - phi)), float(abs(alg / mass / 2 + half - phi))))
        return res, float(mass / 1024)


TEMME_FROM = 1e6


def gamma_pit(shape, g):
    """The regularised lower incomplete gamma function P(shape, g).  ``scipy.special.gammainc``
    below ``TEMME_FROM``; from there on the first term of Temme's uniform expansion,

        P(a, x) = erfc(-eta sqrt(a / 2)) / 2 - exp(-a eta^2 / 2) / sqrt(2 pi a) (c_0(eta) + O(1 / a)),
        eta^2 / 2 = mu - log(1 + mu),  mu = (x - a) / a,  c_0 = 1 / mu - 1 / eta  (-1/3 + eta / 12 - ... at 0),

    whose next term is below 1 / (12 a sqrt(2 pi a)) < 4e-11 there -- because scipy 1.15's
    gammainc is wrong in the lower tail at very large shape: at a = 1e8 and x = a - 4.66 sqrt(a) it
    returns 9.79e-7 where the value is 1.5575e-6 (an error of 5.8e-7, above the bar of
    tests/test_draw_laws.py, which is how it was found).  Both branches are held to an mpmath
    quadrature there."""
    a, x = float(shape), np.asarray(g, dtype=f64)
    if a < TEMME_FROM:
        return special.gammainc(a, x)
    with np.errstate(divide='ignore', invalid='ignore'):
        mu = np.maximum((x - a) / a, -1.0)
        h = mu - np.log1p(mu)
        eta = np.sign(mu) * np.sqrt(2.0 * h)
        c0 = np.where(np.abs(mu) < 1e-3, -1.0 / 3.0 + eta / 12.0 - 2.0 * eta * eta / 135.0, 1.0 / mu - 1.0 / eta)
        out = 0.5 * special.erfc(-eta * math.sqrt(0.5 * a)) - np.exp(-a * h) / math.sqrt(2.0 * math.pi * a) * c0
    return np.clip(np.where(x > 0.0, out, 0.0), 0.0, 1.0)


def gamma_cdf_mp(shape, x, dps=40):
    """P(shape, x) in mpmath: its own series below shape 100, above it a quadrature of the density
    from 60 standard deviations below the mean (what lies further out is below 1e-700), cut every
    4 standard deviations."""
    with mpmath.workdps(dps):
        a, x = mpmath.mpf(float(shape)), mpmath.mpf(float(x))
        if a < 100:
            return float(mpmath.gammainc(a, 0, x, regularized=True))
        sd, lg = mpmath.sqrt(a), mpmath.loggamma(a)
        cuts = [max(mpmath.mpf(0), a - 60 * sd)]
        if x <= cuts[0]:
            return 0.0
        while cuts[-1] + 4 * sd < x:
            cuts.append(cuts[-1] + 4 * sd)
        cuts.append(x)
        return float(mpmath.quad(lambda t: mpmath.exp((a - 1) * mpmath.log(t) - t - lg) if t > 0 else mpmath.mpf(0), cuts))


def box_muller_pits(z):
    """(radius, angle) statistics of the pairs (z[2g], z[2g+1]): ``exp(-(a^2 + b^2) / 2)`` and
    ``atan2(b, a) / 2 pi mod 1``, each U(0, 1) and the two independent."""
    z = np.asarray(z, dtype=f64).reshape(-1)
    a, b = z[0::2], z[1::2]
    return np.exp(-0.5 * (a * a + b * b)), np.mod(np.arctan2(b, a) / (2.0 * np.pi), 1.0)


# ---------------------------------------------------------------------------
# statistics
# ---------------------------------------------------------------------------
def binomial(count, n, p, alpha, name):
    lo, hi = float(stats.binom.ppf(0.5 * alpha, n, p)), float(stats.binom.isf(0.5 * alpha, n, p))
    return dict(name=name, kind='count', value=float(count), lo=lo, hi=hi, mean=n * p)


def hoeffding(count, probs, alpha, name):
    n, m = probs.size, float(np.sum(probs))
    t = math.sqrt(0.5 * n * math.log(2.0 / alpha))
    return dict(name=name, kind='count', value=float(count), lo=m - t, hi=m + t, mean=m)


def exact(count, name):
    return dict(name=name, kind='exact', value=float(count), lo=0.0, hi=0.0)


def independence(v, w, alpha, name):
    """Two checks; v and w PIT-uniform arrays of equal size, the pairs (v_k, w_k) disjoint."""
    v, w = np.asarray(v, dtype=f64).reshape(-1), np.asarray(w, dtype=f64).reshape(-1)
    assert v.size == w.size
    return [unit_interval(np.mod(v - w, 1.0), alpha, name + ': (v - w) mod 1'),
            unit_interval(np.mod(v + w, 1.0), alpha, name + ': (v + w) mod 1')]


def margin_of(c):
    """How far outside its interval a statistic lies, in units of the interval's half width on
    that side (1 = on the edge); an ``exact`` check that fails is decided outright."""
    if c['kind'] == 'exact':
        return float('inf') if c['value'] != 0.0 else 0.0
    if c['kind'] == 'count':
        m = c['mean']
        return (c['value'] - m) / max(c['hi'] - m, 0.5) if c['value'] >= m else (m - c['value']) / max(m - c['lo'], 0.5)
    return c['value'] / c['hi']


def margin(checks):
    return max(margin_of(c) for c in checks)


# ---------------------------------------------------------------------------
# THE table of settings
# ---------------------------------------------------------------------------
SEED = (1 << 40) + 777001
ZIG_MUTANTS = ('wedge_flip', 'wedge_always', 'tail_positive')
GAMMA_SHAPES = (0.05, 0.5, 0.999, 1.0, 1.5, 2.5, 11.0, 8193.0, 1e8)
_GAMMA_MUTANTS = {0.05: ('no_boost',), 0.5: ('no_boost', 'c_from_alpha'), 0.999: ('no_boost',),
                  1.0: ('c_from_alpha', 'd_half'), 1.5: (), 2.5: ('d_half',), 11.0: ('d_half',),
                  8193.0: (), 1e8: ()}

CASES = {
    # rng_fill('normal_zig'): the slow paths against their conditional law
    'zig_slow': dict(test='zig_slow', stream='zig', seed=ds.SEED, offset=ds.ZIG_OFF, e0=0, n=1 << 22, nstat=5,
                     mutants=ZIG_MUTANTS, out_of_scope=('tail_first_attempt',)),
    # ... and the whole stream, on the device (and two neighbours: offset + 1, seed + 1)
    'zig_whole': dict(test='zig_whole', stream='zig_whole', seed=SEED + 1, offset=(1 << 47) + 11, e0=0, n=1 << 26,
                      nstat=13, mutants=('tail_positive',), out_of_scope=()),
    # hmc_gauss_rng_draws: 2 transitions x 4096 chains x 128
    'fused': dict(test='lanes', stream='fused', seed=SEED + 2, offset=(1 << 40) + 5, n=2, C=4096, D=128,
                  chain_offset=3, nstat=18, mutants=ZIG_MUTANTS, out_of_scope=('tail_first_attempt',)),
    # hmc_gauss_big_rng_draws: 2 calls (offset, offset + 1) x 80 chains x (8192 + 777)
    'big': dict(test='lanes', stream='big', seed=SEED + 3, offset=(1 << 40) + 9, n=2, C=80, D=8192 + 777,
                chain_offset=5, nstat=18, mutants=ZIG_MUTANTS, out_of_scope=('tail_first_attempt',)),
    'box_muller': dict(test='box_muller', stream='box_muller', seed=SEED + 4, offset=(1 << 63) + 7, e0=0,
                       n=1 << 22, nstat=6, mutants=('cos_twice',), out_of_scope=()),
    'uniform': dict(test='uniform', stream='uniform', seed=SEED + 5, offset=(1 << 33) + 3, e0=0, n=1 << 22,
                    nstat=6, mutants=(), out_of_scope=()),
    # rng_fill_normal_zig_uniform: both outputs of one launch, odd element offsets
    'zig_uniform': dict(test='zig_uniform', stream='zig_uniform', seed=SEED + 6, offset=ds.ZIG_OFF - 77,
                        offset_u=ds.ZIG_OFF - 76, e0=12345, e0_u=777, n=(1 << 20) + 1, n_u=(1 << 14) + 1,
                        nstat=8, mutants=('wedge_flip', 'wedge_always'), out_of_scope=()),
}
for _k, _sh in enumerate(GAMMA_SHAPES):
    # the second stream at offset + 128: DeviceRNG.gamma advances by 128
    CASES['gamma_%g' % _sh] = dict(test='gamma', stream='gamma', shape=_sh, seed=SEED + 16 + _k,
                                   offset=(1 << 40) + 1000 * _k, e0=0, n=1 << 22, nstat=6,
                                   mutants=_GAMMA_MUTANTS[_sh], out_of_scope=())


def cases_of(test):
    return sorted(n for n, c in CASES.items() if c['test'] == test)


def alpha_of(name):
    """The level of ONE statistic of case ``name``."""
    c = CASES[name]
    return ALPHA / len(cases_of(c['test'])) / c['nstat']


def smallest_dkw_threshold():
    """Over every DKW any case can run (the whole sample is the largest one of a case)."""
    out = []
    for name, c in CASES.items():
        n = c['n'] * c['C'] * c['D'] if 'C' in c else c['n']
        out.append(dkw_threshold(n, alpha_of(name)))
    return min(out)


def _done(name, checks):
    assert len(checks) == CASES[name]['nstat'], (name, len(checks))
    return checks


# ---------------------------------------------------------------------------
# evaluation: the same functions read the restatement's arrays (CPU power table) and the
# device's.  ``d`` is the restatement's Draws: only its first_* fields are used, and they come from
# the generator's words alone.  (A mutant's own Draws classify a mutant run: in the lane streams a
# changed decision shifts the words the lane's later elements are made of.)
# ---------------------------------------------------------------------------
def slow_checks(z, d, alpha):
    """5 checks on the elements whose first candidate is slow."""
    z = np.asarray(z, dtype=f64).reshape(-1)
    slow = d.first_slow.reshape(-1)
    layer, sign = d.first_layer.reshape(-1)[slow], d.first_sign.reshape(-1)[slow]
    zs = z[slow]
    pit = zig_slow_pit(zs, layer, sign)
    tail = layer == 0
    i = layer[~tail].astype(np.int64)
    q = WEDGE_SHARE[i] + (1.0 - WEDGE_SHARE[i]) * (_Q[i + 1] - _Q[i])
    t = sign[~tail] * zs[~tail]
    stayed = np.sum((t >= _X[i + 1]) & (t <= _X[i]))
    return [hoeffding(stayed, q, alpha, 'stayed in the candidate\'s wedge'),
            unit_interval(pit, alpha, 'slow-path PIT (%d)' % pit.size),
            unit_interval(pit[tail], alpha, 'tail PIT (%d)' % int(tail.sum())),
            binomial(slow.sum(), z.size, P_SLOW, alpha, 'slow first candidates'),
            exact(np.sum(np.sign(zs[tail]) != sign[tail]), 'tail signs against candidates')]


def phi_dkw(z, alpha, name='DKW of Phi(z)'):
    return unit_interval(special.ndtr(np.asarray(z, dtype=f64).reshape(-1)), alpha, name)


def evaluate_zig_slow(name, z, d):
    return _done(name, slow_checks(z, d, alpha_of(name)))


def evaluate_lanes(name, p, u, d):
    """p [2, C, D] (transitions, or two calls of the long-chain generator), u [2, C]."""
    a = alpha_of(name)
    p, u = np.asarray(p, dtype=f64), np.asarray(u, dtype=f64)
    v = special.ndtr(p)
    D = p.shape[2]
    D2, D16, C2 = D - D % 2, D - D % 16, p.shape[1] - p.shape[1] % 2
    lane = v[:, :, :D16].reshape(p.shape[0], p.shape[1], -1, 16)
    out = slow_checks(p, d, a) + [phi_dkw(p, a)]
    out += independence(v[:, :, 0:D2:2], v[:, :, 1:D2:2], a, 'lanes j / j+1')
    out += independence(lane[..., :8], lane[..., 8:], a, 'draws t / t+1 of a lane')
    out += independence(v[:, 0:C2:2], v[:, 1:C2:2], a, 'chains c / c+1')
    out += independence(v[0], v[1], a, 'transitions t / t+1')
    out += independence(u, v[:, :, 0], a, 'uniform / first momentum')
    out += [unit_interval(u, a, 'DKW of the acceptance uniforms'),
            exact(np.sum(~((u >= 0.0) & (u < 1.0))), 'uniforms outside [0, 1)')]
    return _done(name, out)


def evaluate_box_muller(name, z):
    a = alpha_of(name)
    rad, ang = box_muller_pits(z)
    return _done(name, [phi_dkw(z, a), unit_interval(rad, a, 'radius: exp(-r^2 / 2)'),
                        unit_interval(ang, a, 'angle / 2 pi')] + independence(rad, ang, a, 'radius / angle')
                 + [exact(np.sum(~np.isfinite(z)), 'not finite')])


def evaluate_uniform(name, u, u_off, u_seed):
    a = alpha_of(name)
    return _done(name, [unit_interval(u, a, 'DKW'), exact(np.sum(~((u >= 0.0) & (u < 1.0))), 'outside [0, 1)')]
                 + independence(u, u_off, a, 'offsets o / o+1') + independence(u, u_seed, a, 'seeds s / s+1'))


def evaluate_gamma(name, g, g_off):
    a, shape = alpha_of(name), CASES[name]['shape']
    g = np.asarray(g, dtype=f64)
    v, w = gamma_pit(shape, g), gamma_pit(shape, g_off)
    return _done(name, [unit_interval(v, a, 'DKW of gammainc(%g, g)' % shape),
                        exact(np.sum(~(g > 0.0)), 'not positive')]
                 + independence(v[0::2], v[1::2], a, 'elements e / e+1')
                 + independence(v, w, a, 'offsets o / o+128'))


def evaluate_zig_uniform(name, p, u, d):
    a = alpha_of(name)
    return _done(name, slow_checks(p, d, a) + [phi_dkw(p, a), unit_interval(u, a, 'DKW of the uniforms'),
                                                exact(np.sum(~((u >= 0.0) & (u < 1.0))), 'uniforms outside [0, 1)')])


# -- the whole stream: torch, so that it runs where the array lies -----------------------
def _dkw_uniform_t(v, alpha, name):
    import torch
    v = v.reshape(-1)
    # (numpy's sort is ten times faster than torch's on the host, where the power table runs)
    v = torch.from_numpy(np.sort(v.numpy())) if v.device.type == 'cpu' else torch.sort(v).values
    n = v.numel()
    i = torch.arange(1, n + 1, dtype=torch.float64, device=v.device)
    d = float(torch.maximum((i / n - v).max(), (v - (i - 1.0) / n).max()))
    return dict(name=name, kind='dkw', value=d, lo=0.0, hi=dkw_threshold(n, alpha))


def _independence_t(v, w, alpha, name):
    import torch
    return [_dkw_uniform_t(torch.remainder(v - w, 1.0), alpha, name + ': (v - w) mod 1'),
            _dkw_uniform_t(torch.remainder(v + w, 1.0), alpha, name + ': (v + w) mod 1')]


def evaluate_zig_whole(name, z, z_off=None, z_seed=None):
    """z and its two neighbours (offset + 1, seed + 1): float64 torch tensors [n].  Without the
    neighbours (the CPU power table's mutant rows, which change z alone): the statistics of z
    alone, at the same level."""
    import torch
    a, n = alpha_of(name), z.numel()
    v = torch.special.ndtr(z)
    out = [_dkw_uniform_t(v, a, 'DKW of Phi(z)')]
    for cnt, p, label in ((int((z > R).sum()), P_TAIL, 'z > R'), (int((z < -R).sum()), P_TAIL, 'z < -R'),
                          (int((z.abs() > 5.0).sum()), 2.0 * float(stats.norm.sf(5.0)), '|z| > 5'),
                          (int((z > 0.0).sum()), 0.5, 'z > 0')):
        out.append(binomial(cnt, n, p, a, 'count of ' + label))
    if z_off is None:
        return out
    v_off, v_seed = torch.special.ndtr(z_off), torch.special.ndtr(z_seed)
    out += _independence_t(v[0::2], v[1::2], a, 'elements 2g / 2g+1')
    quad = v.reshape(-1, 4)
    out += _independence_t(quad[:, :2], quad[:, 2:], a, 'elements e / e+2')
    out += _independence_t(v, v_off, a, 'offsets o / o+1')
    out += _independence_t(v, v_seed, a, 'seeds s / s+1')
    return _done(name, out)


# ---------------------------------------------------------------------------
# the restatement at a case's settings
# ---------------------------------------------------------------------------
def _stack(a, b):
    d = ds.Draws(np.stack([a.ref, b.ref]))
    for f in ('first_layer', 'first_sign', 'first_slow', 'path'):
        setattr(d, f, np.stack([getattr(a, f), getattr(b, f)]))
    return d


def _zig_chunks(seed, offset, n, defect=None, chunk=1 << 22):
    out = np.empty(n)
    for e0 in range(0, n, chunk):
        out[e0:e0 + chunk] = ds.zig_stream(seed, offset, e0, min(chunk, n - e0), defect=defect).ref
    return out


_sound = {}


def host_arrays(name, mutant=None):
    """What the case's evaluator takes, from the restatement: ``(args, d)`` with d the Draws
    whose first_* fields classify (None where the evaluator takes none).  Only the stream under
    test carries the mutant; its neighbours (offset + 1, ...) are the sound ones."""
    c = CASES[name]
    s = c['stream']
    if s == 'zig':
        d = ds.zig_stream(c['seed'], c['offset'], c['e0'], c['n'], defect=mutant)
        return (d.ref,), d
    if s == 'zig_whole':
        import torch
        if mutant is not None:                   # the statistics of z alone (evaluate_zig_whole)
            return (torch.from_numpy(_zig_chunks(c['seed'], c['offset'], c['n'], mutant)),), None
        return tuple(torch.from_numpy(_zig_chunks(c['seed'] + ks, c['offset'] + ko, c['n']))
                     for ks, ko in ((0, 0), (0, 1), (1, 0))), None
    if s == 'fused':
        p, u = ds.fused_streams(c['n'], c['C'], c['D'], c['seed'], c['offset'], c['chain_offset'], defect=mutant)
        return (p.ref, u.ref), p
    if s == 'big':
        a = [ds.big_streams(c['C'], c['D'], c['seed'], c['offset'] + k, c['chain_offset'], defect=mutant)
             for k in range(c['n'])]
        return (np.stack([a[0][0].ref, a[1][0].ref]), np.stack([a[0][1].ref, a[1][1].ref])), _stack(a[0][0], a[1][0])
    if s == 'box_muller':
        return (ds.box_muller_stream(c['seed'], c['offset'], c['e0'], c['n'], defect=mutant).ref,), None
    if s == 'uniform':
        return tuple(ds.uniform_stream(c['seed'] + ks, c['offset'] + ko, c['e0'], c['n']).ref
                     for ks, ko in ((0, 0), (0, 1), (1, 0))), None
    if s == 'gamma':
        if name not in _sound:
            _sound[name] = ds.gamma_stream(c['shape'], c['seed'], c['offset'] + 128, c['e0'], c['n']).ref
        return (ds.gamma_stream(c['shape'], c['seed'], c['offset'], c['e0'], c['n'], defect=mutant).ref,
                _sound[name]), None
    if s == 'zig_uniform':
        d = ds.zig_stream(c['seed'], c['offset'], c['e0'], c['n'], defect=mutant)
        return (d.ref, ds.uniform_stream(c['seed'], c['offset_u'], c['e0_u'], c['n_u']).ref), d
    raise KeyError(s)


EVALUATORS = {'zig': evaluate_zig_slow, 'zig_whole': evaluate_zig_whole, 'fused': evaluate_lanes,
              'big': evaluate_lanes, 'box_muller': evaluate_box_muller, 'uniform': evaluate_uniform,
              'gamma': evaluate_gamma, 'zig_uniform': evaluate_zig_uniform}


def evaluate(name, args, d=None):
    f = EVALUATORS[CASES[name]['stream']]
    return f(name, *args) if d is None else f(name, *(tuple(args) + (d,)))
