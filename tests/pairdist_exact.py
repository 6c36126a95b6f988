"""Exact-arithmetic references for the pair-distance restraint model (BASELINE
config C5), independent of oracle/ref_distance.py: standard library and numpy
only (``math.isqrt``, ``fractions``, ``decimal`` at 50 digits with exact
``Decimal(float)`` conversion).

What it provides:

* ``cr_sqrt(s)``: the correctly rounded square root of a double, from an integer
  square root of the scaled argument.
* ``hard_cases()``: squared distances whose square root lies within a few
  2^-50 result ulps of a rounding midpoint -- the inputs on which a sqrt
  iteration that is only *nearly* correct rounds the wrong way.  For a small
  c = 1 (mod 8) an odd M with M^2 = c (mod 2^55) is Hensel-lifted; for M in
  [2^53, 2^54) the double s = (M^2 - c) 2^-106 lies in [1, 4) and its root
  M 2^-53 - c 2^-106 / (M 2^-53 + sqrt(s)) sits below the midpoint M 2^-53 (an
  odd multiple of half a result ulp, the result ulp being 2^-52) by less than
  c 2^-55 ulps; s = (M^2 + c) 2^-106 mirrors it above.  Multiplying s by
  2^(2k) moves the case to another binade without changing the relative picture.
* ``edge_values()``: the 2^-767 cut of the kernels' sqrt and its neighbours,
  subnormals, 0, values near DBL_MAX.
* ``realise(s)``: a difference vector (a, b, 0) whose squared length, evaluated
  in fp64 as the kernels do it -- ``(a*a + b*b) + 0*0``, every operation rounded,
  no FMA -- is exactly s.
* ``force_rows(x, ymat, tau, rows)``: the restraint force
  tau sum_j (d - y)(x_i - x_j)/d of the chosen beads in 50-digit decimal, with
  d and x_i - x_j exact functions of the fp64 coordinates (NaN where d = 0, as
  the model's definition gives); ``force_scales`` the two magnitudes the force
  bound of the GPU tests is made of.
"""
import decimal
import math
from fractions import Fraction

import numpy as np

CTX = decimal.Context(prec=50, Emin=-999999, Emax=999999)
U = 2.0 ** -53
D0 = decimal.Decimal(0)


def dec(v):
    """exact decimal of a double (Decimal(float) is exact; the context rounds only results)"""
    return decimal.Decimal(float(v))


# ---------------------------------------------------------------------------
# correctly rounded sqrt
# ---------------------------------------------------------------------------
def cr_sqrt(s):
    """sqrt(s) rounded to nearest even, from math.isqrt of an exact scaled integer."""
    s = float(s)
    if s != s or s < 0.0:
        return float('nan')
    if s == 0.0 or s == float('inf'):
        return s
    num, den = s.as_integer_ratio()          # den a power of two
    e = den.bit_length() - 1                 # s = num 2^-e
    # A = s 2^(2t) an integer of at least 112 bits: its isqrt carries >= 56 bits
    t = max(0, (112 - num.bit_length() + e + 1) // 2 + 1)
    if 2 * t < e:
        t = (e + 1) // 2
    A = num << (2 * t - e)
    q = math.isqrt(A)                        # sqrt(s) = sqrt(A) 2^-t, sqrt(A) in [q, q + 1)
    exact = q * q == A
    shift = q.bit_length() - 53
    keep, rem = q >> shift, q & ((1 << shift) - 1)
    half = 1 << (shift - 1)
    if rem > half or (rem == half and (not exact or keep & 1)):
        keep += 1
    return math.ldexp(keep, shift - t)


# ---------------------------------------------------------------------------
# hard-to-round squared distances
# ---------------------------------------------------------------------------
def _sqrt_mod_2k(c, k):
    """the odd roots of M^2 = c (mod 2^k), c = 1 (mod 8), by Hensel lifting"""
    c %= 1 << k
    assert c % 8 == 1
    m = 1
    for b in range(3, k):                    # m^2 = c (mod 2^b) -> mod 2^(b + 1)
        if (m * m - c) >> b & 1:
            m += 1 << (b - 1)
    mod = 1 << k
    roots = {m % mod, (-m) % mod, (m + (mod >> 1)) % mod, (-m + (mod >> 1)) % mod}
    assert all(r * r % mod == c % mod for r in roots)
    return sorted(roots)


class HardCase(object):
    """s = (M^2 - side c) 2^-106 2^(2k): sqrt(s) lies below (side = +1) or above
    (side = -1) the midpoint M 2^-53 2^k by less than c 2^-55 result ulps."""

    def __init__(self, M, c, side, k):
        self.M, self.c, self.side, self.k = M, c, side, k
        self.s = math.ldexp(float(M * M - side * c), -106 + 2 * k)

    def midpoint(self):
        return Fraction(self.M) * Fraction(2) ** (self.k - 53)

    def ulp(self):
        return Fraction(2) ** (self.k - 52)

    def expected(self):
        """the correctly rounded root: the representable neighbour on sqrt(s)'s side"""
        return math.ldexp(float((self.M - self.side) // 2), self.k - 52)


def hard_cases(cs=(1, 9, 17, 25, 33, 41, 49, 57, 65, 73), scales=(0, 5, -9, 200, -300)):
    """below a midpoint: M^2 = c (mod 2^55) for the given c = 1 (mod 8); above one (the
    mirrored form M^2 + c'): M^2 = -c' (mod 2^55), which needs c' = 7 (mod 8) -- c' = c + 6"""
    out = []
    for c0 in cs:
        for side in (1, -1):
            c = c0 if side > 0 else c0 + 6
            for M in _sqrt_mod_2k(side * c, 55):
                if not (1 << 53) <= M < (1 << 54):
                    continue
                for k in scales:
                    h = HardCase(M, c, side, k)
                    # (M^2 -+ c) 2^-106 must be a double: M^2 -+ c = 0 (mod 2^55), < 2^108
                    assert Fraction(h.s) == Fraction(M * M - side * c) * Fraction(2) ** (2 * k - 106)
                    out.append(h)
    return out


def check_near_midpoint(h):
    """integer / rational proof that sqrt(s) is on the stated side of the midpoint,
    closer than c 2^-55 ulps"""
    s = Fraction(h.s)
    mid = h.midpoint()
    gap = Fraction(h.c) * Fraction(2) ** -55 * h.ulp()
    if h.side > 0:      # below: (mid - gap)^2 < s < mid^2
        return (mid - gap) ** 2 < s < mid ** 2
    return mid ** 2 < s < (mid + gap) ** 2


# ---------------------------------------------------------------------------
# edge values of the squared distance
# ---------------------------------------------------------------------------
DBL_MAX = float.fromhex('0x1.fffffffffffffp+1023')
CUT = 2.0 ** -767                            # sqrt_rn's plain range starts here


def edge_values():
    """squared distances at the kernels' edges (every one realisable by realise())"""
    vals = [CUT, np.nextafter(CUT, 0.0), np.nextafter(CUT, 1.0),
            math.ldexp(1.5, -767), math.ldexp(1.0, -800), math.ldexp(1.0, -1000),
            5e-324, math.ldexp(3.0, -1074), math.ldexp(1.0, -1050), math.ldexp(1.0, -1023),
            np.nextafter(2.0 ** -1022, 0.0), 2.0 ** -1022,
            DBL_MAX, np.nextafter(DBL_MAX, 0.0), 2.0 ** 1023, math.ldexp(1.75, 1020),
            1.0, np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0), 4.0, np.nextafter(4.0, 0.0)]
    return [float(v) for v in vals]


# ---------------------------------------------------------------------------
# a chosen squared distance as a difference vector
# ---------------------------------------------------------------------------
def _round_bits(v, bits):
    if v == 0.0:
        return 0.0
    m, e = math.frexp(v)
    return math.ldexp(round(m * (1 << bits)), e - bits)


def fp_sq(a, b, e=0.0):
    """(a*a + b*b) + e*e in fp64, every operation rounded (Python floats: no FMA)"""
    return (a * a + b * b) + e * e


def realise(s, fracs=(0.6, 0.3, 0.45, 0.75, 0.9, 0.2), max_ulps=64):
    """(a, b) with fp_sq(a, b, 0.0) == s exactly; a has <= 26 significant bits, so
    a*a is exact wherever it is a normal number.  a takes a share `frac` of s; b is
    searched within max_ulps of the root of the rest (another share if none fits)."""
    s = float(s)
    if s == 0.0:
        return 0.0, 0.0
    for frac in fracs:
        a = _round_bits(math.sqrt(s * frac), 26) if s > 2.0 ** -900 else 0.0
        if a * a == float('inf'):
            a = 0.0
        r = float(Fraction(s) - Fraction(a * a)) if a else s
        b0 = math.sqrt(r) if r > 0 else 0.0
        cands = [b0]
        up = dn = b0
        for _ in range(max_ulps):
            up, dn = float(np.nextafter(up, math.inf)), float(np.nextafter(dn, 0.0))
            cands += [up, dn]
        for b in cands:
            if fp_sq(a, b) == s:
                return a, b
    raise ValueError('no b within %d ulps realises s=%r' % (max_ulps, s))


# ---------------------------------------------------------------------------
# exact force
# ---------------------------------------------------------------------------
def _dsqrt(v):
    return v.sqrt(CTX)


def exact_pair(xi, xj):
    """exact differences and 50-digit distance of two beads (sequences of 3 doubles)"""
    dv = [CTX.subtract(dec(xi[k]), dec(xj[k])) for k in range(3)]
    s = CTX.add(CTX.add(CTX.multiply(dv[0], dv[0]), CTX.multiply(dv[1], dv[1])), CTX.multiply(dv[2], dv[2]))
    return dv, _dsqrt(s)


def force_rows(x, ymat, tau, rows):
    """{bead i: [F_i0, F_i1, F_i2]} (Decimal, NaN where a partner coincides with i) of
    tau sum_{j != i} (d_ij - y_ij)(x_i - x_j)/d_ij; x [n, 3], ymat [n, n] doubles."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    n = x.shape[0]
    t = dec(tau)
    out = {}
    for i in rows:
        f = [D0, D0, D0]
        nan = False
        xi = x[i]
        for j in range(n):
            if j == i:
                continue
            dv, d = exact_pair(xi, x[j])
            if d == 0:
                nan = True
                continue
            w = CTX.divide(CTX.subtract(d, dec(ymat[i, j])), d)
            for k in range(3):
                f[k] = CTX.add(f[k], CTX.multiply(w, dv[k]))
        out[int(i)] = [decimal.Decimal('NaN')] * 3 if nan else [CTX.multiply(t, v) for v in f]
    return out


def force_scales(x, ymat, rows):
    """per row and axis: A = sum_j |y/d| |x_i - x_j| and W = sum_j |1 - y/d| |x_i - x_j| (fp64,
    to a few ulps -- they scale a bound, they are not checked)"""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    A, W = {}, {}
    for i in rows:
        dv = x[i][None, :] - x
        d = np.sqrt(np.sum(dv * dv, axis=1))
        m = np.arange(len(x)) != i
        with np.errstate(divide='ignore', invalid='ignore'):
            r = np.abs(ymat[i] / d)
        ad = np.abs(dv)
        A[int(i)] = (r[m, None] * ad[m]).sum(axis=0)
        W[int(i)] = (np.abs(1.0 - r[m])[:, None] * ad[m]).sum(axis=0)
    return A, W


def exact_distance(xi, xj):
    """the exact distance of two beads rounded once to a double"""
    return float(exact_pair(xi, xj)[1])


# ---------------------------------------------------------------------------
# exact leapfrog (binf/samplers/hmc.py:116-123) with the restraint force and an isotropic prior
# ---------------------------------------------------------------------------
def exact_grad(q, ymat, tau, prior):
    """gradient of the energy: restraint force + k (q - x0), all beads, Decimal [n][3]"""
    n = len(q)
    t = dec(tau)
    g = [[D0, D0, D0] for _ in range(n)]
    for i in range(n):
        for j in range(i + 1, n):
            dv = [CTX.subtract(q[i][k], q[j][k]) for k in range(3)]
            d = _dsqrt(CTX.add(CTX.add(CTX.multiply(dv[0], dv[0]), CTX.multiply(dv[1], dv[1])),
                               CTX.multiply(dv[2], dv[2])))
            w = CTX.multiply(t, CTX.divide(CTX.subtract(d, dec(ymat[i, j])), d))
            for k in range(3):
                v = CTX.multiply(w, dv[k])
                g[i][k] = CTX.add(g[i][k], v)
                g[j][k] = CTX.subtract(g[j][k], v)
    if prior is not None:
        pk, x0 = dec(prior[0]), dec(prior[1])
        for i in range(n):
            for k in range(3):
                g[i][k] = CTX.add(g[i][k], CTX.multiply(pk, CTX.subtract(q[i][k], x0)))
    return g


def exact_leapfrog(q0, p0, ymat, tau, prior, dt, L):
    """q, p after L leapfrog steps, Decimal [n][3] each; also the gradients met on the way"""
    q = [[dec(v) for v in row] for row in np.asarray(q0, dtype=np.float64).reshape(-1, 3)]
    p = [[dec(v) for v in row] for row in np.asarray(p0, dtype=np.float64).reshape(-1, 3)]
    h, dtd = CTX.multiply(dec(dt), decimal.Decimal('0.5')), dec(dt)
    grads = []

    def kick(step):
        g = exact_grad(q, ymat, tau, prior)
        grads.append(g)
        for i in range(len(p)):
            for k in range(3):
                p[i][k] = CTX.subtract(p[i][k], CTX.multiply(step, g[i][k]))

    def drift():
        for i in range(len(q)):
            for k in range(3):
                q[i][k] = CTX.add(q[i][k], CTX.multiply(dtd, p[i][k]))

    kick(h)
    for _ in range(L - 1):
        drift()
        kick(dtd)
    drift()
    kick(h)
    return q, p, grads


def to_f64(rows):
    return np.array([[float(v) for v in r] for r in rows], dtype=np.float64)
