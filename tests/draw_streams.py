"""Host restatement of every device draw stream, with derived decision margins and
value bounds.  Written from the papers (Salmon et al. SC'11; Blackman & Vigna 2018;
Marsaglia & Tsang 2000 twice; Doornik 2005) and from the comments of
``philox_draws.hpp`` / ``xoshiro.hpp`` / ``hmc_gauss_kernel.hpp`` / ``hmc_gauss_big.hip``.
Nothing here calls into the library; the only thing read from the source tree is the
committed ziggurat table (data), which :func:`check_tables` verifies in mpmath.

Streams
-------
stand-alone (Philox4x32-10, element e of stream (seed, offset), GLOBAL index e):
  :func:`uniform_stream`, :func:`box_muller_stream`, :func:`zig_stream`,
  :func:`gamma_stream`.
fused (xoshiro128++ per lane, seeded from the Philox block under key tag 0x58534f52):
  :func:`fused_streams` (persistent kernel), :func:`big_streams` (long chains).

Every function returns a :class:`Draws`: reference values, an absolute bound per
element, the path the element took and whether any accept decision on that path was
marginal.  :func:`compare` holds a device array against it.

Accuracy hypothesis
-------------------
ROCm's accuracy table is not assumed to be at hand; the hypothesis is: device ``exp``
and ``log`` err by at most 1 ulp, ``sincospi`` by at most 2 ulp, ``pow`` by at most
2 ulp; ``sqrt``, ``/``, ``*``, ``+`` are correctly rounded and the library is compiled
without contraction, so the written expression fixes every other rounding.  An error of
n ulp of a result r is at most ``n * EPS * |r|`` with ``EPS = 2**-52``; all bounds
below are stated in that unit ("ulp" = EPS relative), ``u = EPS / 2`` is one rounding.

Decisions (float64, each with the error of its two sides; none measured)
-----------------------------------------------------------------------
fast test   Philox: ``|u| < RATIO[layer]`` compares two exact doubles.  xoshiro:
            ``|u X[layer]| < X[layer+1]`` compares one correctly rounded product with
            a table entry.  Both are reproduced exactly: error 0, never marginal.
wedge test  ``f1 + U (f0 - f1) < 1`` with ``f = exp(a)``, ``a = -0.5 (X^2 - x^2)``:
            ``|da| <= u/2 (X^2 + x^2 + 2|a|)`` (two squares, one difference),
            ``|df| <= f (|da| + EPS)`` (1-ulp exp), and the three roundings of the
            combination add ``u (2 U |f0 - f1| + |lhs|)``.
tail test   ``-2 y >= x x`` with ``y = log(1 - ub)``, ``x = log(1 - ua) / R``: the left
            side carries 1 ulp, the right ``2 (1 + 1/2) + 1/2 = 3.5`` ulp.
gamma t<=0  ``t = 1 + c x``: ``|dt| <= EPS (4.5 |c x| + 0.5 |t|)`` (x: 4 ulp, below).
gamma       ``log(1 - u1) < x^2/2 + d - d v + d log v``: left 1 ulp; right, with
squeeze     ``rt = |dt| / |t|``: ``8.5 EPS x^2/2 + (3 rt + 1.5 EPS) d v +
            d (3 rt + EPS + 1.5 EPS |log v|) + 1.5 EPS S`` where
            ``S = |x^2/2| + d + d v + d |log v|`` is the cancellation scale of the
            three additions.
A decision is MARGINAL when its two sides differ by no more than twice that error
(once for the device, once for this float64 evaluation); it is then re-decided in
mpmath at 50 digits, the element is flagged and left out of value comparison.

Values
------
uniform, fast-path, wedge-accepted and redrawn normals are exact products: bound 0.
tail        ``z = R - x``: x carries 1.5 ulp (log, division), the subtraction one
            rounding: ``EPS (1.5 |x| + 0.5 |z|)``, times 2; reference: mpmath.
Box-Muller  ``sqrt(-2 log(1 - u1)) cospi(2 u2)``: 1 ulp (log) halves under the root,
            plus its rounding = 1; sincospi 2; the product 1/2: <= 4 ulp.
gamma       ``d v`` with ``v = t^3``: ``3 rt + 1.5 ulp``; shape < 1 adds pow (2 ulp) and
            a product (1/2 ulp); results in the subnormal range are held to the same
            count of subnormal spacings.  ``c`` and ``d`` come from correctly rounded
            operations only and are reproduced exactly.
References for the inexact values are computed in 80-bit long double from the same
uniforms (error 2**-11 ulp; one rounding to double, 1/2 ulp, is added to each bound).
"""
import math
import os
import re

import numpy as np

EPS = 2.0 ** -52
M32 = 0xffffffff
M64 = (1 << 64) - 1
XO_TAG = 0x58534f52
BIG_U_STREAM = 1 << 62
NPY_BUFSIZE = 8192
PW_BLOCK = 128
SUBNORMAL = 2.0 ** -1074

FAST, WEDGE, REDRAWN, TAIL = 0, 1, 2, 3
PATHS = ('fast', 'wedge', 'redrawn', 'tail')

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, 'the high-precision references need an 80-bit long double'


class Draws(object):
    """ref [..] float64, bound [..] absolute, path [..] int8, marginal [..] bool.  The
    ziggurat streams add the element's FIRST candidate, read from the generator's words
    alone: first_layer [..] int16, first_sign [..] int8 (-1 / +1), first_slow [..] bool (it
    failed the fast test) -- what tests/draw_laws.py classifies elements by."""

    def __init__(self, ref, bound=None, path=None, marginal=None, **info):
        self.ref = ref
        self.first_layer = self.first_sign = self.first_slow = None
        self.bound = np.zeros(ref.shape) if bound is None else bound
        self.path = np.zeros(ref.shape, dtype=np.int8) if path is None else path
        self.marginal = np.zeros(ref.shape, dtype=bool) if marginal is None else marginal
        self.info = info

    def counts(self):
        return dict((name, int(np.sum(self.path == k))) for k, name in enumerate(PATHS))


# ---------------------------------------------------------------------------
# Philox4x32-10
# ---------------------------------------------------------------------------
_PM0, _PM1, _PW0, _PW1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(ctr, key):
    c0, c1, c2, c3 = [int(c) & M32 for c in ctr]
    k0, k1 = [int(k) & M32 for k in key]
    for _ in range(10):
        p0, p1 = _PM0 * c0, _PM1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + _PW0) & M32, (k1 + _PW1) & M32
    return [c0, c1, c2, c3]


def philox_v(c0, c1, c2, c3, k0, k1):
    """Vectorised over the counter words (uint64 arrays holding 32-bit values)."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3)])
    k0, k1 = int(k0) & M32, int(k1) & M32
    m, s = np.uint64(M32), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(_PM0) * c0, np.uint64(_PM1) * c2
        c0, c1, c2, c3 = (p1 >> s) ^ c1 ^ np.uint64(k0), p1 & m, (p0 >> s) ^ c3 ^ np.uint64(k1), p0 & m
        k0, k1 = (k0 + _PW0) & M32, (k1 + _PW1) & M32
    return c0, c1, c2, c3


def u53(a, b):
    """53-bit uniform in [0, 1) from two 32-bit words (exact in float64)."""
    if isinstance(a, np.ndarray):
        return ((a >> np.uint64(5)).astype(np.float64) * 67108864.0
                + (b >> np.uint64(6)).astype(np.float64)) * (1.0 / 9007199254740992.0)
    return ((a >> 5) * 67108864.0 + (b >> 6)) * (1.0 / 9007199254740992.0)


def _block_v(i, seed, offset, tag=None):
    """Philox block of counter i (int64 array) under (seed, offset); tag: the ziggurat's
    attempt tag in the top 16 bits of the offset."""
    i = np.asarray(i, dtype=np.uint64)
    c3 = (offset >> 32) & M32
    if tag is not None:
        c3 = (c3 & 0xffff) | (tag << 16)
    return philox_v(i & np.uint64(M32), i >> np.uint64(32), offset & M32, c3, seed & M32, (seed >> 32) & M32)


def _block_s(i, seed, offset, tag=None):
    c3 = (offset >> 32) & M32
    if tag is not None:
        c3 = (c3 & 0xffff) | (tag << 16)
    return philox4x32_10([i & M32, (i >> 32) & M32, offset & M32, c3], [seed & M32, (seed >> 32) & M32])


def _pairs(e0, n):
    """Blocks g0 .. that the window [e0, e0 + n) touches, and the window's slice of
    the interleaved pair outputs."""
    g0 = e0 >> 1
    npairs = ((e0 + n + 1) >> 1) - g0
    return np.arange(g0, g0 + npairs, dtype=np.int64), slice(e0 - 2 * g0, e0 - 2 * g0 + n)


def _interleave(a, b):
    out = np.empty(2 * a.size, dtype=a.dtype)
    out[0::2], out[1::2] = a, b
    return out


# ---------------------------------------------------------------------------
# uniform and Box-Muller
# ---------------------------------------------------------------------------
def uniform_stream(seed, offset, e0, n):
    g, win = _pairs(e0, n)
    r = _block_v(g, seed, offset)
    return Draws(_interleave(u53(r[0], r[1]), u53(r[2], r[3]))[win])


def _sincospi_hp(a):
    """(sin(pi a), cos(pi a)) in long double for doubles a in [0, 2): the reduction
    r = a - q / 2, q = rint(2 a), is exact, so zeros come out as exact zeros."""
    a = np.asarray(a, dtype=np.float64)
    q = np.rint(2.0 * a)
    r = (a - 0.5 * q).astype(LD)
    pi = LD(3.141592653589793238462643383279502884)
    s, c = np.sin(pi * r), np.cos(pi * r)
    s = np.where(r == 0, LD(0), s)
    q = q.astype(np.int64) & 3
    sin = np.where(q == 0, s, np.where(q == 1, c, np.where(q == 2, -s, -c)))
    cos = np.where(q == 0, c, np.where(q == 1, -s, np.where(q == 2, -c, s)))
    return sin, cos


def _box_muller_hp(u1, u2):
    r = np.sqrt(LD(-2) * np.log(LD(1) - u1.astype(LD)))
    s, c = _sincospi_hp(2.0 * u2)
    return r * c, r * s


BM_ULP = 4.0


def box_muller_stream(seed, offset, e0, n, defect=None):
    """defect 'cos_twice': the pair's second element repeats the cosine."""
    assert defect is None or defect in BOX_MULLER_DEFECTS, defect
    g, win = _pairs(e0, n)
    r = _block_v(g, seed, offset)
    a, b = _box_muller_hp(u53(r[0], r[1]), u53(r[2], r[3]))
    if defect == 'cos_twice':
        b = a
    ref = _interleave(a, b)[win].astype(np.float64)
    return Draws(ref, (BM_ULP + 0.5) * EPS * np.abs(ref))


# ---------------------------------------------------------------------------
# the ziggurat table and its decisions
# ---------------------------------------------------------------------------
def _read_tables():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                        'binf_amd', 'csrc', 'zig_tables.hpp')
    text = open(path).read()

    def arr(name, n):
        body = re.search(r'%s\[%d\] = \{(.*?)\};' % (name, n), text, re.S).group(1)
        return np.array([float.fromhex(t) for t in body.replace(',', ' ').split()])
    tail_r = float.fromhex(re.search(r'ZIG_TAIL_R = (\S+);', text).group(1))
    bits = int(re.search(r'ZIG_BITS = (\d+);', text).group(1))
    return arr('ZIG_X', 1025), arr('ZIG_RATIO', 1024), tail_r, bits


ZX, ZR, TAIL_R, ZIG_BITS = _read_tables()
_ZXL, _ZRL = [float(v) for v in ZX], [float(v) for v in ZR]
assert ZIG_BITS == 10 and ZX.shape == (1025,) and ZR.shape == (1024,)


def check_tables():
    """The committed table in mpmath: returns the figures the CPU test asserts on."""
    import mpmath as mp
    mp.mp.dps = 50
    X = [mp.mpf(float(v)) for v in ZX]

    def f(x):
        return mp.exp(-x * x / 2)
    tail = mp.sqrt(mp.pi / 2) * mp.erfc(X[1] / mp.sqrt(2))
    base = X[1] * f(X[1]) + tail                       # the base strip plus the tail
    areas = [X[i] * (f(X[i + 1]) - f(X[i])) for i in range(1, 1024)]
    v = sum(areas) / len(areas)
    return dict(
        area_spread=float(max(abs(a - v) for a in areas) / v),
        base_vs_layers=float(abs(base - v) / v),
        x0_vs_base=float(abs(X[0] * f(X[1]) - base) / base),      # X[0] = V / f(R)
        monotone=bool(np.all(np.diff(ZX) < 0) and ZX[1024] == 0.0),
        ratio_exact=bool(np.array_equal(ZR, ZX[1:] / ZX[:-1])),
        tail_r=bool(TAIL_R == ZX[1]))


# The injected defects of the ziggurat streams (``defect=``).  Law mutants -- the stream's
# distribution is no longer N(0, 1): 'wedge_flip' (the wedge test inverted), 'wedge_always'
# (the wedge test always accepts), 'tail_positive' (every tail value positive),
# 'tail_first_attempt' (the tail's first attempt always stands: an exponential law).
# 'tail_sign' (the tail's sign inverted) is NOT a law mutant: the law is symmetric and the
# sign bit is independent of everything else, so only the element-wise comparison and what
# tests/draw_laws.py conditions on the candidate's sign see it.
ZIG_DEFECTS = ('wedge_flip', 'wedge_always', 'tail_positive', 'tail_first_attempt', 'tail_sign')
GAMMA_DEFECTS = ('gamma_offset', 'no_boost', 'c_from_alpha', 'd_half')
BOX_MULLER_DEFECTS = ('cos_twice',)


def _wedge_defect(acc, defect):
    if defect == 'wedge_flip':
        return not acc
    return True if defect == 'wedge_always' else acc


class _Stats(object):
    def __init__(self):
        self.marginal_decisions = 0
        self.wedge_trace = None          # list of (x, layer, U, accepted) when asked for


def _mp_wedge(x, layer, U):
    import mpmath as mp
    mp.mp.dps = 50
    x, xi, xi1, U = mp.mpf(x), mp.mpf(_ZXL[layer]), mp.mpf(_ZXL[layer + 1]), mp.mpf(U)
    f0, f1 = mp.exp(-(xi * xi - x * x) / 2), mp.exp(-(xi1 * xi1 - x * x) / 2)
    return bool(f1 + U * (f0 - f1) < 1)


def wedge_decide(x, layer, U, stats):
    """(accept, marginal) of the ZIGNOR wedge test as the kernels write it."""
    xi, xi1 = _ZXL[layer], _ZXL[layer + 1]
    x2 = x * x
    a0, a1 = -0.5 * (xi * xi - x2), -0.5 * (xi1 * xi1 - x2)
    f0, f1 = math.exp(a0), math.exp(a1)
    lhs = f1 + U * (f0 - f1)
    u = 0.5 * EPS
    da0 = 0.5 * u * (xi * xi + x2 + 2.0 * abs(a0))
    da1 = 0.5 * u * (xi1 * xi1 + x2 + 2.0 * abs(a1))
    err = (1.0 - U) * f1 * (da1 + EPS) + U * f0 * (da0 + EPS) + u * (2.0 * U * abs(f0 - f1) + abs(lhs))
    acc, marg = lhs < 1.0, abs(lhs - 1.0) <= 2.0 * err
    if marg:
        stats.marginal_decisions += 1
        acc = _mp_wedge(x, layer, U)
    if stats.wedge_trace is not None:
        stats.wedge_trace.append((x, layer, U, acc))
    return acc, marg


def tail_draw(uniforms, neg, stats, defect=None):
    """Marsaglia's tail beyond R from successive (ua, ub): (value, bound, marginal).
    ``uniforms(t)`` gives attempt t's pair; at most 64 attempts, the last one stands."""
    neg = (neg != (defect == 'tail_sign')) and defect != 'tail_positive'
    import mpmath as mp
    marginal, x, ua = False, 0.0, 0.0
    for t in range(64):
        ua, ub = uniforms(t)
        x = math.log(1.0 - ua) / TAIL_R
        lhs, rhs = -2.0 * math.log(1.0 - ub), x * x
        acc = lhs >= rhs
        if abs(lhs - rhs) <= 2.0 * EPS * (abs(lhs) + 3.5 * rhs):
            mp.mp.dps = 50
            stats.marginal_decisions += 1
            marginal = True
            acc = bool(-2 * mp.log(1 - mp.mpf(ub)) >= (mp.log(1 - mp.mpf(ua)) / mp.mpf(TAIL_R)) ** 2)
        if acc or defect == 'tail_first_attempt':
            break
    mp.mp.dps = 50
    xm = mp.log(1 - mp.mpf(ua)) / mp.mpf(TAIL_R)
    z = float(mp.mpf(TAIL_R) - xm)
    bound = 2.0 * EPS * (1.5 * abs(x) + 0.5 * z)
    return (-z if neg else z), bound, marginal


# ---------------------------------------------------------------------------
# the Philox ZIGNOR stream
# ---------------------------------------------------------------------------
def _zig_split(lo, hi):
    """layer from the low 10 bits, u in [-1, 1) from the 53 bits above (scalars)."""
    uu = ((hi >> 1) * 4194304.0 + (lo >> ZIG_BITS)) * (1.0 / 9007199254740992.0)
    return lo & 1023, 2.0 * uu - 1.0


def _zig_slow(lo, hi, i, which, seed, offset, stats, defect):
    """The candidate (lo, hi) of block i failed the fast test: (value, bound, path, marginal)."""
    marginal, k = False, 1
    while True:
        layer, u = _zig_split(lo, hi)
        if abs(u) < _ZRL[layer]:
            return u * _ZXL[layer], 0.0, REDRAWN, marginal
        if layer == 0:
            def uniforms(t):
                r = _block_s(i, seed, offset, 0x8000 | (t << 1) | which)
                return u53(r[0], r[1]), u53(r[2], r[3])
            z, bound, m = tail_draw(uniforms, u < 0.0, stats, defect)
            return z, bound, TAIL, marginal or m
        r = _block_s(i, seed, offset, (k << 1) | which)
        x = u * _ZXL[layer]
        acc, m = wedge_decide(x, layer, u53(r[2], r[3]), stats)
        marginal = marginal or m
        acc = _wedge_defect(acc, defect)
        if acc or k >= 63:
            return x, 0.0, (WEDGE if k == 1 else REDRAWN), marginal
        lo, hi, k = r[0], r[1], k + 1


def zig_stream(seed, offset, e0, n, defect=None, trace=False):
    assert 0 <= offset < 1 << 48, 'the attempt tags live in the top 16 bits of the offset'
    g, win = _pairs(e0, n)
    r = _block_v(g, seed, offset, 0)
    lo = _interleave(r[0], r[2])[win]
    hi = _interleave(r[1], r[3])[win]
    layer = (lo & np.uint64(1023)).astype(np.int64)
    uu = ((hi >> np.uint64(1)).astype(np.float64) * 4194304.0
          + (lo >> np.uint64(ZIG_BITS)).astype(np.float64)) * (1.0 / 9007199254740992.0)
    u = 2.0 * uu - 1.0
    assert defect is None or defect in ZIG_DEFECTS, defect
    d = Draws(u * ZX[layer])
    d.first_layer, d.first_sign = layer.astype(np.int16), np.where(u < 0.0, -1, 1).astype(np.int8)
    d.first_slow = ~(np.abs(u) < ZR[layer])
    stats = _Stats()
    if trace:
        stats.wedge_trace = []
    for l in np.nonzero(d.first_slow)[0]:
        e = e0 + int(l)
        d.ref[l], d.bound[l], d.path[l], d.marginal[l] = _zig_slow(
            int(lo[l]), int(hi[l]), e >> 1, e & 1, seed, offset, stats, defect)
    d.info.update(marginal_decisions=stats.marginal_decisions, wedge_trace=stats.wedge_trace)
    return d


# ---------------------------------------------------------------------------
# the gamma stream (Marsaglia & Tsang 2000)
# ---------------------------------------------------------------------------
POW_ULP = 2.0


def _mp_gamma_decide(u1n, u2n, u1, c, d):
    """(t > 0, accept) of one attempt at 50 digits, from the attempt's uniforms."""
    import mpmath as mp
    mp.mp.dps = 50
    x = mp.sqrt(-2 * mp.log(1 - mp.mpf(u1n))) * mp.cospi(2 * mp.mpf(u2n))
    t = 1 + mp.mpf(c) * x
    if t <= 0:
        return False, False
    v, d = t ** 3, mp.mpf(d)
    return True, bool(mp.log(1 - mp.mpf(u1)) < x * x / 2 + d - d * v + d * mp.log(v))


def gamma_stream(shape, seed, offset, e0, n, small=True, defect=None):
    """Element e: attempt k draws its normal from counter e under offset + 2k and its
    two uniforms under offset + 2k + 1; t <= 0 retries; at most 64 attempts, then d.
    Defects: 'gamma_offset' (the uniforms from the normal's own offset), 'no_boost'
    (shape < 1 without the factor U^(1/shape): the law of shape + 1), 'c_from_alpha'
    (c = 1 / sqrt(9 alpha): the normal envelope no longer dominates), 'd_half'
    (d = alpha - 1/2: the law of shape alpha - 1/6)."""
    assert defect is None or defect in GAMMA_DEFECTS, defect
    shape = float(shape)
    alpha = shape + 1.0 if shape < 1.0 else shape
    d = alpha - (0.5 if defect == 'd_half' else 1.0 / 3.0)
    c = 1.0 / math.sqrt(9.0 * (alpha if defect == 'c_from_alpha' else d))
    small = small and defect != 'no_boost'
    e = np.arange(e0, e0 + n, dtype=np.int64)
    out = Draws(np.full(n, d))
    attempts = np.full(n, 64, dtype=np.int64)
    before_pow, pow_base = np.full(n, d), np.ones(n)             # g = before_pow * pow_base**(1/shape)
    pending = np.arange(n)
    t_retries = marginal_decisions = 0
    with np.errstate(divide='ignore', invalid='ignore', over='ignore', under='ignore'):
        for k in range(64):
            if pending.size == 0:
                break
            rn = _block_v(e[pending], seed, (offset + 2 * k) & M64)
            ru = _block_v(e[pending], seed, (offset + (2 * k if defect == 'gamma_offset' else 2 * k + 1)) & M64)
            u1n, u2n = u53(rn[0], rn[1]), u53(rn[2], rn[3])
            u1, u2 = u53(ru[0], ru[1]), u53(ru[2], ru[3])
            xh = _box_muller_hp(u1n, u2n)[0]
            x = xh.astype(np.float64)
            cx = c * x
            t = 1.0 + cx
            dt = EPS * (BM_ULP + 0.5) * np.abs(cx) + 0.5 * EPS * np.abs(t)
            tpos = t > 0.0
            tmarg = np.abs(t) <= 2.0 * dt
            tt = np.where(tpos, t, 1.0)
            v = tt * tt * tt
            logv = np.log(v)
            lhs = np.log(1.0 - u1)
            A = 0.5 * x * x
            rhs = A + d - d * v + d * logv
            rt = dt / np.abs(tt)
            S = np.abs(A) + d + d * v + d * np.abs(logv)
            err = (EPS * np.abs(lhs) + 8.5 * EPS * A + (3.0 * rt + 1.5 * EPS) * d * v
                   + d * (3.0 * rt + EPS + 1.5 * EPS * np.abs(logv)) + 1.5 * EPS * S)
            acc = tpos & (lhs < rhs)
            marg = tmarg | (tpos & (np.abs(lhs - rhs) <= 2.0 * err))
            for l in np.nonzero(marg)[0]:
                marginal_decisions += 1
                tp, a = _mp_gamma_decide(u1n[l], u2n[l], u1[l], c, d)
                tpos[l], acc[l] = tp, a
                out.marginal[pending[l]] = True
            t_retries += int(np.sum(~tpos))
            # the accepted values, in long double from the same uniforms
            th = LD(1) + LD(c) * xh[acc]
            gh = LD(d) * th * th * th
            rel = 3.0 * rt[acc] + 1.5 * EPS
            before_pow[pending[acc]] = gh.astype(np.float64)
            if small and shape < 1.0:
                pow_base[pending[acc]] = 1.0 - u2[acc]
                gh = gh * np.power(LD(1) - u2[acc].astype(LD), LD(1.0 / shape))
                rel = rel + (POW_ULP + 0.5) * EPS
            idx = pending[acc]
            ref = gh.astype(np.float64)
            out.ref[idx] = ref
            nulp = (rel + 0.5 * EPS) / EPS
            out.bound[idx] = nulp * np.maximum(EPS * np.abs(ref), SUBNORMAL)
            attempts[idx] = k
            pending = pending[~acc]
    out.path[:] = np.where(attempts == 0, FAST, REDRAWN)          # first attempt / a later one
    out.info.update(attempts=attempts, t_retries=t_retries, marginal_decisions=marginal_decisions,
                    exhausted=int(pending.size), c=c, d=d,
                    before_pow=before_pow, pow_base=pow_base)
    return out


# ---------------------------------------------------------------------------
# xoshiro128++ and the fused generator
# ---------------------------------------------------------------------------
def _rotl(x, k):
    return ((x << k) | (x >> (32 - k))) & M32


class Xo128(object):
    """One stream, Python ints."""

    def __init__(self, s):
        self.s = [int(v) for v in s]

    @classmethod
    def seeded(cls, stream, seed, offset):
        r = philox4x32_10([stream & M32, (stream >> 32) & M32, offset & M32, (offset >> 32) & M32],
                          [seed & M32, ((seed >> 32) & M32) ^ XO_TAG])
        if not any(r):
            r[0] = 1
        return cls(r)

    def next(self):
        s = self.s
        r = (_rotl((s[0] + s[3]) & M32, 7) + s[0]) & M32
        t = (s[1] << 9) & M32
        s[2] ^= s[0]
        s[3] ^= s[1]
        s[1] ^= s[2]
        s[0] ^= s[3]
        s[2] ^= t
        s[3] = _rotl(s[3], 11)
        return r

    def uniform53(self):
        a = self.next()
        return u53(a, self.next())

    def candidate(self):
        """(x, layer, final): layer = top 10 bits of the first output, u = 2 d - 3 with
        d in [1, 2) built from the other 52 bits."""
        hi = self.next()
        lo = self.next()
        layer = hi >> 22
        u = 2.0 * (1.0 + (((hi & 0xfffff) << 32) | lo) * EPS) - 3.0
        x = u * _ZXL[layer]
        return x, layer, abs(x) < _ZXL[layer + 1]


class XoV(object):
    """Many streams, uint32 arrays."""

    def __init__(self, stream, seed, offset):
        stream = np.asarray(stream, dtype=np.uint64)
        r = philox_v(stream & np.uint64(M32), stream >> np.uint64(32), offset & M32, (offset >> 32) & M32,
                     seed & M32, ((seed >> 32) & M32) ^ XO_TAG)
        self.s = [v.astype(np.uint32) for v in r]
        zero = (self.s[0] | self.s[1] | self.s[2] | self.s[3]) == 0
        self.s[0][zero] = 1

    @staticmethod
    def _rotl(x, k):
        return (x << np.uint32(k)) | (x >> np.uint32(32 - k))

    def next(self, mask=None):
        """The next output of every stream; only streams under `mask` advance."""
        s0, s1, s2, s3 = self.s
        r = self._rotl(s0 + s3, 7) + s0
        t = s1 << np.uint32(9)
        n2 = s2 ^ s0
        n3 = s3 ^ s1
        n1 = s1 ^ n2
        n0 = s0 ^ n3
        n2 = n2 ^ t
        n3 = self._rotl(n3, 11)
        new = [n0, n1, n2, n3]
        self.s = new if mask is None else [np.where(mask, a, b) for a, b in zip(new, self.s)]
        return r

    def uniform53(self):
        a = self.next().astype(np.uint64)
        return u53(a, self.next().astype(np.uint64))


def _xo_resolve(x, layer, g, stats, defect):
    """A candidate that failed the fast test: wedge test (tail for the base layer); a
    rejection draws fresh candidates from the lane's own stream.  64 rounds at most."""
    marginal, path = False, WEDGE
    for _ in range(64):
        if layer == 0:
            def uniforms(t):
                a = g.uniform53()
                return a, g.uniform53()
            z, bound, m = tail_draw(uniforms, x < 0.0, stats, defect)
            return z, bound, TAIL, marginal or m
        acc, m = wedge_decide(x, layer, g.uniform53(), stats)
        marginal = marginal or m
        acc = _wedge_defect(acc, defect)
        if acc:
            return x, 0.0, path, marginal
        path = REDRAWN
        x, layer, ok = g.candidate()
        if ok:
            return x, 0.0, path, marginal
    return x, 0.0, path, marginal


def _lane_draws(n):
    d = Draws(np.zeros(n))
    d.first_layer, d.first_sign = np.zeros(n, dtype=np.int16), np.zeros(n, dtype=np.int8)
    d.first_slow = np.zeros(n, dtype=bool)
    return d


def _lane_normals(gen, idx, gs, out, stats, defect):
    """The lanes' momentum draws: idx [lanes, T] is the flat output index of slot t
    (-1: not drawn, consumes nothing).  Per group of `gs` slots: the wanted candidates
    first, then this lane's rejections in index order."""
    nl, T = idx.shape
    for g0 in range(0, T, gs):
        fails = []
        for i in range(g0, g0 + gs):
            want = idx[:, i] >= 0
            if not want.any():
                continue
            hi = gen.next(want).astype(np.uint64)
            lo = gen.next(want).astype(np.uint64)
            layer = (hi >> np.uint64(22)).astype(np.int64)
            dd = 1.0 + (((hi & np.uint64(0xfffff)) << np.uint64(32)) | lo).astype(np.float64) * EPS
            x = (2.0 * dd - 3.0) * ZX[layer]
            ok = np.abs(x) < ZX[layer + 1]
            w = np.nonzero(want)[0]
            out.ref[idx[w, i]] = x[w]
            out.first_layer[idx[w, i]] = layer[w]
            out.first_sign[idx[w, i]] = np.where(dd[w] < 1.5, -1, 1)
            out.first_slow[idx[w, i]] = ~ok[w]
            for l in np.nonzero(want & ~ok)[0]:
                fails.append((int(l), i, float(x[l]), int(layer[l])))
        fails.sort()                                            # by lane, then by slot
        pos = 0
        while pos < len(fails):
            l = fails[pos][0]
            g = Xo128([s[l] for s in gen.s])
            while pos < len(fails) and fails[pos][0] == l:
                _, i, x, layer = fails[pos]
                o = idx[l, i]
                out.ref[o], out.bound[o], out.path[o], out.marginal[o] = _xo_resolve(x, layer, g, stats, defect)
                pos += 1
            for k in range(4):
                gen.s[k][l] = g.s[k]


_FIELDS = ('ref', 'bound', 'path', 'marginal', 'first_layer', 'first_sign', 'first_slow')


def tree_height(n):
    if n <= PW_BLOCK:
        return 0
    n2 = n // 2
    n2 -= n2 % 8
    return 1 + max(tree_height(n2), tree_height(n - n2))


def leaves(n, H):
    """numpy's pairwise-summation leaves of a length-n vector under a tree of height
    H: (lowest path, offset, length); a leaf above depth H is listed once."""
    out = []
    for path in range(1 << H):
        off, m, depth = 0, n, 0
        for dd in range(H):
            if m <= PW_BLOCK:
                break
            n2 = m // 2
            n2 -= n2 % 8
            if (path >> (H - 1 - dd)) & 1:
                off, m = off + n2, m - n2
            else:
                m = n2
            depth += 1
        if path & ((1 << (H - depth)) - 1) == 0:
            out.append((path, off, m))
    return out


def fused_layout(D):
    """(H, slots per lane, group size) of the persistent kernel for chains of D."""
    H = tree_height(D)
    tneed = max((ln + 7) // 8 for _, _, ln in leaves(D, H))
    T = 16 if H > 3 else min(t for t in (1, 2, 4, 8, 12, 16) if t >= tneed)
    return H, T, (8 if T % 8 == 0 else (4 if T % 4 == 0 else T))


def fused_streams(n, C, D, seed, offset, chain_offset=0, defect=None, trace=False):
    """(p [n, C, D], u [n, C]) of hmc_gauss_rng_draws: lane (chain, leaf, j) owns the
    elements off + 8 t + j of its leaf and the stream
    (chain + chain_offset) * (8 << H) + 8 * (lowest path of the leaf) + j, reseeded
    for transition s at offset + s; the uniform follows the last group, from the
    chain's first lane."""
    assert D <= 8192
    H, T, gs = fused_layout(D)
    lv = leaves(D, H)
    paths = np.array([p for p, _, _ in lv], dtype=np.int64)
    offs = np.array([o for _, o, _ in lv], dtype=np.int64)
    lens = np.array([ln for _, _, ln in lv], dtype=np.int64)
    j = np.arange(8, dtype=np.int64)
    lane_stream = (paths[:, None] * 8 + j[None, :]).ravel()                  # [leaves * 8]
    t = np.arange(T, dtype=np.int64)
    within = 8 * t[None, None, :] + j[None, :, None]                         # [1, 8, T]
    local = np.where(within < lens[:, None, None], offs[:, None, None] + within, -1).reshape(-1, T)
    chains = np.arange(C, dtype=np.int64)
    stream = ((chains[:, None] + chain_offset) * (8 << H) + lane_stream[None, :]).ravel()
    assert defect is None or defect in ZIG_DEFECTS, defect
    p = _lane_draws(n * C * D)
    stats = _Stats()
    if trace:
        stats.wedge_trace = []
    u = np.empty((n, C))
    for s in range(n):
        idx = np.where(local[None, :, :] >= 0,
                       s * C * D + chains[:, None, None] * D + local[None, :, :], -1).reshape(-1, T)
        gen = XoV(stream, seed, (offset + s) & M64)
        _lane_normals(gen, idx, gs, p, stats, defect)
        u[s] = gen.uniform53().reshape(C, -1)[:, 0]               # path 0, j = 0
    for name in _FIELDS:
        setattr(p, name, getattr(p, name).reshape(n, C, D))
    p.info.update(marginal_decisions=stats.marginal_decisions, wedge_trace=stats.wedge_trace)
    return p, Draws(u)


def big_streams(C, D, seed, offset, chain_offset=0, defect=None):
    """(p [C, D], u [C]) of hmc_gauss_big_rng_draws: chunks of 8192 elements; the lane
    (group, j) of a (chain, chunk) owns the stream
    (((chain + chain_offset) * nchunks + chunk) * 32 + group) * 8 + j and serves the
    leaves group, group + 32, ... in that order, each in two halves of 8 slots; a
    leaf reached by several paths is drawn once, by its lowest path.  The chain's
    uniform is the first of stream BIG_U_STREAM + chain + chain_offset."""
    nchunks = (D + NPY_BUFSIZE - 1) // NPY_BUFSIZE
    assert defect is None or defect in ZIG_DEFECTS, defect
    p = _lane_draws(C * D)
    stats = _Stats()
    chains = np.arange(C, dtype=np.int64)
    for chunk in range(nchunks):
        m = min(NPY_BUFSIZE, D - chunk * NPY_BUFSIZE)
        H = tree_height(m)
        rounds = ((1 << H) + 31) // 32
        local = np.full((32, 8, rounds * 16), -1, dtype=np.int64)
        for path, off, ln in leaves(m, H):
            for jj in range(8):
                for t in range(16):
                    if 8 * t + jj < ln:
                        local[path % 32, jj, (path // 32) * 16 + t] = chunk * NPY_BUFSIZE + off + 8 * t + jj
        local = local.reshape(256, -1)
        lane = np.arange(256, dtype=np.int64)                    # group * 8 + j
        stream = (((chains[:, None] + chain_offset) * nchunks + chunk) * 256 + lane[None, :]).ravel()
        idx = np.where(local[None] >= 0, chains[:, None, None] * D + local[None], -1).reshape(C * 256, -1)
        gen = XoV(stream, seed, offset)
        _lane_normals(gen, idx, 8, p, stats, defect)
    for name in _FIELDS:
        setattr(p, name, getattr(p, name).reshape(C, D))
    p.info['marginal_decisions'] = stats.marginal_decisions
    u = XoV(BIG_U_STREAM + chains + chain_offset, seed, offset).uniform53()
    return p, Draws(u)


# ---------------------------------------------------------------------------
# holding a device array against a restatement
# ---------------------------------------------------------------------------
def compare(got, d):
    """Report of `got` against the Draws d: elements compared per path, marginal
    elements (left out), mismatches (indices), and the largest error of the inexact
    elements in ulp (EPS relative)."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == d.ref.shape, (got.shape, d.ref.shape)
    live = ~d.marginal
    diff = np.abs(got - d.ref)
    bad = live & ~(diff <= d.bound)                              # NaN fails
    inexact = live & (d.bound > 0) & (d.ref != 0)
    with np.errstate(divide='ignore', invalid='ignore'):
        ulp = np.where(inexact, diff / np.maximum(EPS * np.abs(d.ref), SUBNORMAL), 0.0)
        ratio = np.where(live & (d.bound > 0), diff / np.where(d.bound > 0, d.bound, 1.0), 0.0)
    rep = dict(max_of_bound=float(ratio.max()) if ratio.size else 0.0, compared=dict((name, int(np.sum(live & (d.path == k)))) for k, name in enumerate(PATHS)),
               marginal=int(np.sum(d.marginal)), mismatches=np.argwhere(bad),
               max_ulp=float(ulp.max()) if ulp.size else 0.0)
    rep['n'] = sum(rep['compared'].values())
    return rep


def describe(rep, got=None, d=None, limit=5):
    s = ('compared %(compared)s, marginal %(marginal)d, max err %(max_ulp).3f ulp '
         '(%(max_of_bound).3f of its bound)' % rep)
    s += ', %d mismatches' % len(rep['mismatches'])
    if got is not None:
        for ix in rep['mismatches'][:limit]:
            ix = tuple(ix)
            s += '\n  %s: got %r want %r +- %.3g (%s)' % (ix, float(np.asarray(got)[ix]), float(d.ref[ix]),
                                                         float(d.bound[ix]), PATHS[d.path[ix]])
    return s


# ---------------------------------------------------------------------------
# The cases of tests/test_gpu_draw_streams.py.  Seeds and offsets use the high words
# (seed >= 2**40, ziggurat offsets next to 2**48 - 1); tests/test_draw_streams.py
# asserts that none of them meets a marginal decision in the restatement.
# ---------------------------------------------------------------------------
SEED = (1 << 40) + 12345
ZIG_OFF = (1 << 48) - 1
# (seed, offset, elem_offset, n, output view shifted by one double)
ZIG_CASES = [(SEED, ZIG_OFF, 0, 1 << 22, False),
             (SEED + 1, ZIG_OFF - 1, 12345, 100001, False),        # odd window start, odd n
             (SEED + 2, ZIG_OFF - 2, (1 << 33) + 2, 4099, False),  # counter high word, 16-byte stores
             (SEED + 3, ZIG_OFF - 3, (1 << 33) + 1, 1, False),
             (SEED + 4, ZIG_OFF - 4, 0, 65537, True),              # 8-byte aligned: scalar stores
             (SEED + 5, ZIG_OFF - 5, 6, 2, False)]
FLAT_CASES = [(SEED, (1 << 63) + 5, 0, 1 << 20, False),
              (SEED + 1, (1 << 33) + 1, 12345, 100001, False),
              (SEED + 2, 3, (1 << 33) + 2, 4099, True),
              (SEED + 3, 4, (1 << 33) + 1, 1, False)]
GAMMA_SHAPES = (0.5, 1.0, 2.5, 11.0, 8193.0, 1e8)
# (shape, seed, offset, elem_offset, n)
GAMMA_CASES = [(sh, SEED + 16 * k, (1 << 40) + 2 * k, (12345, (1 << 33) + 1, 0)[k % 3], 200000 + (k & 1))
               for k, sh in enumerate(GAMMA_SHAPES)]
# (transitions, C, D, seed, offset, chain_offset)
FUSED_CASES = [(1, 60000, 8, SEED, 7, 0),
               (2, 4096, 64, SEED + 1, (1 << 40) + 3, 0),
               (1, 3000, 33, SEED + 2, 9, 11),
               (1, 1200, 200, SEED + 3, 9, 1 << 40),
               (2, 256, 1024, SEED + 4, (1 << 63) + 1, 5),
               (1, 150, 2048, SEED + 5, 2, 7)]
# (C, D, seed, offset, chain_offset): one full chunk and a ragged one
BIG_CASES = [(40, 8192 + 777, SEED + 6, (1 << 40) + 1, 3)]


# ---------------------------------------------------------------------------
# do the bounds see a defect?
# ---------------------------------------------------------------------------
def self_test(verbose=False):
    """Each injected defect must produce mismatches; the sound stream must not.
    Returns {defect: number of mismatches}."""
    seen = {}

    def note(name, rep):
        seen[name] = len(rep['mismatches'])
        if verbose:
            print('%-28s %s' % (name, describe(rep)))

    seed, off, n = (1 << 40) + 99, (1 << 48) - 1, 1 << 19
    z = zig_stream(seed, off, 0, n)
    note('zig: sound', compare(z.ref, z))
    for path in (FAST, TAIL):
        got = z.ref.copy()
        i = np.nonzero(z.path == path)[0][0]
        got[i] = got[i] * (1.0 + 64 * EPS)
        note('zig: %s value + 64 ulp' % PATHS[path], compare(got, z))
    note('zig: wedge flipped', compare(zig_stream(seed, off, 0, n, defect='wedge_flip').ref, z))
    note('zig: tail sign flipped', compare(zig_stream(seed, off, 0, n, defect='tail_sign').ref, z))
    b = box_muller_stream(seed, 3, 0, 4096)
    note('box-muller: sound', compare(b.ref, b))
    note('box-muller: + 64 ulp', compare(b.ref * (1.0 + 64 * EPS), b))
    for shape in (0.5, 2.5):
        g = gamma_stream(shape, seed, 7, 0, 1 << 15)
        note('gamma %g: sound' % shape, compare(g.ref, g))
        note('gamma %g: + 64 ulp' % shape, compare(g.ref * (1.0 + 64 * EPS), g))
        note('gamma %g: wrong offset' % shape,
             compare(gamma_stream(shape, seed, 7, 0, 1 << 15, defect='gamma_offset').ref, g))
    p, u = fused_streams(1, 4096, 64, seed, 5)
    note('fused: sound', compare(p.ref, p))
    note('fused: wedge flipped', compare(fused_streams(1, 4096, 64, seed, 5, defect='wedge_flip')[0].ref, p))
    note('fused: tail sign flipped', compare(fused_streams(1, 4096, 64, seed, 5, defect='tail_sign')[0].ref, p))
    for name, m in seen.items():
        assert (m == 0) == name.endswith('sound'), (name, m)
    return seen


if __name__ == '__main__':
    self_test(verbose=True)
