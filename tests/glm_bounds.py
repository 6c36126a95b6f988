"""Derived error bounds for the generalised-linear kernels (``binf_glm_pointwise_f64``,
``binf_linear_glm_logp_f64``, ``binf_linear_glm_grad_f64``; csrc/glm_term.hpp, csrc/glm.hip),
and the exact values they are measured from.  Nothing here is a measured tolerance.  Host only.

Notation: ``u = 2**-53``, ``gamma_m = m u / (1 - m u)`` (linear_bounds.gamma),
``S_n = sum_k |theta_k| |A_kn|``, ``TINY = 2**-1074`` (one subnormal step: what a result that
underflows may lose whatever its size), and for a computed part ``x`` "8u" means
``8 u |x| + TINY``: the allowance ``linear_bounds`` gives the device's ``log`` and its epilogue,
used here for the device's ``exp`` and ``log1p`` too.  The ROCm toolchain installs no
device-library document that states an error for double ``exp`` or ``log1p`` (none that states a
larger one, then), so 8u stands; the largest measured fraction of the bound is in DESIGN.

linear predictor
    ``eta^_n = fl(mock^_n + offset_n)`` with ``|mock^_n - mock_n| <= gamma_K S_n`` (the mock
    datum's bound of linear_bounds: K products, K - 1 additions, any order, fused or not):
    ``|eta^_n - eta_n| <= delta_n = gamma_K S_n + u (|mock_n| + gamma_K S_n + |offset_n|)``.
    Without an offset the addition of 0.0 is exact; the same delta is kept (it is not smaller).

log-density term (``y`` successes of ``m`` trials; the constants are the caller's, below)
    The exact term is Lipschitz in eta: ``|d ll / d eta| = |y - m s(eta)| <= max(y, m - y)``
    (binomial), ``|y - e**eta| <= y + e**(eta + delta)`` on the interval (Poisson).  Then every
    operation of glm_term.hpp on ``eta^``, with H = |eta| + delta and X+ = x evaluated at
    eta + delta:
      binomial  t = exp(-|eta^|): 8u t, t <= 1;  L = log1p(t^): <= 8u t (the slope of log1p is
                at most 1) + 8u L, L <= log 2;  sp = fl(max(eta^, 0) + L^): + u sp+;
                a = fl(y eta^): u y H;  b = fl(m sp^): m (the above) + u m sp+;
                ll = fl(a - b): u (y H + m sp+).
                ``B_n = max(y, m - y) delta + 2 u y H + m (8u t + 8u L + 3 u sp+) + (2 m + 2) TINY``
                (the TINY of t and the TINY of L reach ll through the product by m: where t is
                subnormal, at |eta| > 708.39, they are all of its error -- the edge ladder at
                eta = -745.13 with m = 2**20 is where a flat 4 TINY, right for m = 1, fell short
                of numpy's own restatement; one TINY each for the two products)
      Poisson   e = exp(eta^): 8u e+;  a = fl(y eta^): u y H;  ll = fl(a - e^): u (y H + e+).
                ``B_n = (y + e+) delta + 2 u y H + 10 u e+ + 3 TINY``
    with t and L taken at their suprema on the interval (|eta| - delta, clipped at 0).

log-prob
    N computed terms summed in ANY order (lanes, pieces, joins; zero-initialised accumulators
    and the padding columns left out by a select add nothing): ``gamma_{N+1} sum_n |ll^_n|``, and
    one rounding for ``+ log_norm``: ``u (sum_n |ll^_n| + |log_norm|)``, with ``|ll^_n| <= y H +
    m sp+`` (``y H + e+``) ``+ B_n``:
        ``|lp^ - lp| <= sum_n B_n + (gamma_{N+1} + u) sum_n (mag_n + B_n) + u |log_norm|``.
    ``log_norm`` is an INPUT of the kernel (one double, computed once on the host): the exact
    value is that of the double it receives.  How far ``math.lgamma`` leaves that double from
    ``sum log C(m, y)`` is the model's business and is held by :func:`lgamma_bound` in the CPU
    tests.  The as-written path (forward kernel, element-wise record, ``binf_row_sum_f64``) obeys
    the same model with one more rounding per datum for ``+ lconst_n``; :func:`pointwise_bound`.

gradient term
    ``|d g / d eta| = m s (1 - s) <= m / 4`` (binomial), ``e**eta`` (Poisson).  Operations:
      binomial  t: 8u;  d = fl(1 + t^): relative (8u t + u (1 + t)) / (1 + t) <= 9u;  the
                quotient: u;  s is computed to 18u s (numerator 8u or exact, denominator 9u, the
                division u);  fl(m s^): u m s;  fl(. - y): u (m s + y).
                ``rho_n = m delta / 4 + 20 u m s+ + u y + (2 m + 1) TINY``,  s+ <= 1  (the TINY
                of t and of the quotient through the product by m, as above)
      Poisson   ``rho_n = e+ delta + 8 u e+ + u (e+ + y) + 2 TINY``
force
    as tests/grad_bounds.py with rho_n in place of the residual's error: an N-term dot product of
    the computed g^_n in SOME tree (tiles, splits, lane joins),
        ``|G^_i - G_i| <= sum_n |A_in| rho_n + gamma_N sum_n |A_in| (|g_n| + rho_n)``.

The exact values: eta from integer arithmetic on the doubles (``linear_bounds.Exact.mock``, the
offset added as an exact rational), carried through mpmath at 50 digits (glm_ref.exact_ll /
exact_g).  The bounds are evaluated in double precision; ``SLACK = 1 + 2**-30`` covers the
roundings of that evaluation and of rounding the exact eta to a double where a magnitude is
taken (relative u |eta| <= 2**-46 for the |eta| <= 100 of the generators).

For the chains that are NOT compared with exact arithmetic the bound is evaluated at numpy's
float64 eta~ with delta doubled: numpy's own mock datum obeys the same model, so the exact eta
lies within delta of eta~ and the device's within 2 delta.  numpy's result lies inside that
bound as the device's does: the assertion on a device value is ``|got - numpy| <= 2 bound``.

The inputs of the GPU tests, beside :func:`case`:
    :func:`force_cases`, with :func:`table_row` / :func:`chain_tiles` (the dispatch tables of
    glm.hip restated) -- every (KS, KV) x CT instantiation; :func:`dropped_visibility` is the CPU
    check that a row which loses a coefficient leaves the bound on the chains compared exactly.
    :func:`edge_ladder` / :func:`edge_case` -- each eta at which the term changes behaviour, put
    exactly into the kernels; :func:`edge_pointwise_check` and :func:`edge_chain_check` are the
    assertions, shared by the GPU tests (the device's values) and the CPU test (numpy's).  Two
    Poisson rules, and no other exception: (1) above eta = 700 the 17-term sum of e+ in
    :func:`logp_bound` is no double, so a chain with such an eta is held by the per-datum bound
    of the element-wise kernel alone (of the fused kernels only the signs are asserted there:
    their own sum of 17 such terms may overflow); (2) a datum beyond exp's overflow (eta > 709.78...) is
    ll = -inf and g = +inf exactly, its chain's log-prob -inf and its gradient an infinity of the
    design row's sign -- never NaN -- and the other chains of the launch keep their bits.
    ``ExactGLM(..., roundings=m)`` states another forward model's ``gamma_m S_n`` (Horner: 2 K).
"""
import math

import numpy as np

import glm_ref as R
import grad_bounds as GB
import linear_bounds as LB

U = LB.U
SLACK = LB.SLACK
gamma = LB.gamma
TINY = 2.0 ** -1074
LANCZOS_G = 6.024680040776729583740234375      # CPython's mathmodule.c


def eta_delta(S, mock_abs, offset_abs, K):
    """delta_n of the module docstring."""
    gs = gamma(K) * np.asarray(S, dtype=np.float64)
    return (gs + U * (np.asarray(mock_abs) + gs + offset_abs)) * SLACK


def _mags(family, eta, delta, y, m):
    """Magnitudes on the interval eta +- delta: dict of arrays."""
    eta = np.asarray(eta, dtype=np.float64)
    H = np.abs(eta) + delta
    with np.errstate(over='ignore', under='ignore'):
        if family == R.BINOMIAL_LOGIT:
            lo = np.maximum(np.abs(eta) - delta, 0.0)
            t = np.exp(-lo)
            L = np.log1p(t)
            up = eta + delta
            sp = np.maximum(up, 0.0) + np.log1p(np.exp(-np.abs(up)))
            return dict(H=H, t=t, L=L, sp=sp, mag=y * H + m * sp, g=np.maximum(m, y))
        e = np.exp(eta + delta)
        return dict(H=H, e=e, mag=y * H + e, g=e + y)


def term_bounds(family, eta, delta, y, m=None):
    """``(B, rho, mag, gabs)``: the bounds on one datum's ll and g, and upper limits of |ll|
    and |g|, elementwise.  ``eta``: the exact eta rounded to doubles, or numpy's with a delta
    that covers the distance."""
    y = np.asarray(y, dtype=np.float64)
    m = np.ones_like(y) if m is None else np.asarray(m, dtype=np.float64)
    q = _mags(family, eta, delta, y, m)
    if family == R.BINOMIAL_LOGIT:
        B = np.maximum(y, m - y) * delta + 2 * U * y * q['H'] + \
            m * (8 * U * q['t'] + 8 * U * q['L'] + 3 * U * q['sp']) + (2 * m + 2) * TINY
        rho = m * delta / 4 + 20 * U * m + U * y + (2 * m + 1) * TINY
    else:
        with np.errstate(invalid='ignore'):         # an overflowed e with delta = 0: no bound
            B = (y + q['e']) * delta + 2 * U * y * q['H'] + 10 * U * q['e'] + 3 * TINY
            rho = q['e'] * delta + 8 * U * q['e'] + U * (q['e'] + y) + 2 * TINY
    return B * SLACK, rho * SLACK, q['mag'] * SLACK, q['g'] * SLACK


def logp_bound(B, mag, log_norm, N):
    """The log-prob bound from the per-datum bounds (summed over the last axis)."""
    s = np.sum(mag + B, axis=-1)
    return (np.sum(B, axis=-1) + (gamma(N + 1) + U) * s + U * abs(log_norm)) * SLACK


def pointwise_bound(B, mag, lconst, umag=None):
    """One datum of the record: its term's bound and the rounding of ``+ lconst_n``.  ``umag``:
    ``u mag`` itself, for a magnitude that is no double once SLACK is on it (the last double
    below exp's overflow); ``mag`` is then not read."""
    lc = 0.0 if lconst is None else np.abs(lconst)
    um = U * mag if umag is None else umag
    return (B + um + U * (B + lc)) * SLACK


def rowsum_bound(Bp, mag, lconst, N):
    """The as-written log-prob: the record's terms summed in numpy's pairwise order."""
    lc = 0.0 if lconst is None else np.abs(lconst)
    return (np.sum(Bp, axis=-1) + gamma(N) * np.sum(mag + lc + Bp, axis=-1)) * SLACK


def force_bound(A, rho, gabs):
    """``[.. x K]`` from ``rho``, ``gabs`` ``[.. x N]``."""
    absA = np.abs(A)
    N = A.shape[1]
    return (rho.dot(absA.T) + gamma(N) * (gabs + rho).dot(absA.T)) * SLACK


def lgamma_bound(x):
    """How far CPython's ``math.lgamma(x)`` may lie from the truth for an integer ``x >= 1``:
    exactly 0 for x <= 2 (returned as such); beyond, Lanczos' form ``log(sum) - g + (x - 0.5)
    (log(x + g - 0.5) - 1)`` -- 8u of the magnitude of each of the parts it adds."""
    if x <= 2:
        return 0.0
    a = x + LANCZOS_G - 0.5
    return 8 * U * (abs(math.log(a)) * (x - 0.5) + (x - 0.5) + LANCZOS_G + abs(math.log(x)) + 1.0)


# ---------------------------------------------------------------------------
# exact values
# ---------------------------------------------------------------------------
class ExactGLM(object):
    """Exact log-probs and forces of chains against one data set."""

    def __init__(self, family, A, ys, trials=None, offset=None, roundings=None):
        """``roundings``: the m of the mock datum's ``gamma_m S_n`` (None: K, the linear forward
        kernels' dot product; a forward model of another evaluation order states its own)."""
        self.family = family
        self.A = np.asarray(A, dtype=np.float64)
        self.K, self.N = self.A.shape
        self.roundings = self.K if roundings is None else int(roundings)
        self.ys = np.asarray(ys, dtype=np.float64)
        self.m = np.ones(self.N) if trials is None else np.asarray(trials, dtype=np.float64)
        self.off = np.zeros(self.N) if offset is None else np.asarray(offset, dtype=np.float64)
        self.ex = LB.Exact(self.A, np.zeros(self.N))

    def eta(self, theta):
        """``(eta as mpf list, eta rounded to doubles, delta)`` of one chain."""
        M = R.mp()
        theta = np.asarray(theta, dtype=np.float64)
        ints, s = self.ex.mock(theta)
        scale = M.mpf(2) ** s
        mock = [M.mpf(int(v)) / scale for v in ints]
        eta = [mk + M.mpf(float(o)) for mk, o in zip(mock, self.off)]
        S = np.abs(theta).dot(self.ex.absA) * SLACK
        mock_abs = np.array([float(abs(v)) for v in mock])
        delta = eta_delta(S, mock_abs, np.abs(self.off), self.roundings)
        return eta, np.array([float(v) for v in eta]), delta

    def chain(self, theta, log_norm=0.0, want_force=True):
        """dict(eta, delta, ll=[mpf], g=[mpf], lp=mpf (log_norm included), lp_bound,
        force=[mpf], force_bound=[K], B, rho, mag, gabs)."""
        M = R.mp()
        eta, etaf, delta = self.eta(theta)
        ll = [R.exact_ll(self.family, e, y, m) for e, y, m in zip(eta, self.ys, self.m)]
        B, rho, mag, gabs = term_bounds(self.family, etaf, delta, self.ys, self.m)
        out = dict(eta=etaf, delta=delta, ll=ll, B=B, rho=rho, mag=mag, gabs=gabs,
                   lp=M.fsum(ll) + M.mpf(float(log_norm)),
                   lp_bound=float(logp_bound(B, mag, log_norm, self.N)))
        if want_force:
            g = [R.exact_g(self.family, e, y, m) for e, y, m in zip(eta, self.ys, self.m)]
            # the force in integers: g_n to 240 bits, A exactly
            gi = np.array([int(M.floor(v * M.mpf(2) ** 240 + M.mpf(0.5))) for v in g], dtype=object)
            Gi = np.asarray(np.dot(self.ex.mA, gi), dtype=object).reshape(self.K)
            out['g'] = g
            out['force'] = [M.mpf(int(v)) / M.mpf(2) ** (240 + self.ex.sA) for v in Gi]
            out['force_bound'] = force_bound(self.A, rho, gabs)
        return out


def err(got, exact):
    """``|got - exact|`` as a float, ``exact`` an mpf."""
    M = R.mp()
    return float(abs(M.mpf(float(got)) - exact))


def float_case(family, theta, A, ys, trials=None, offset=None, log_norm=0.0):
    """numpy's values and the float form of the bounds for every chain of ``theta`` [C x K]:
    dict(eta, ll, g, lp, lp_bound, force, force_bound, B, mag)."""
    theta = np.atleast_2d(theta)
    K, N = A.shape
    mock = theta.dot(A)
    off = 0.0 if offset is None else offset
    eta = mock + off
    S = np.abs(theta).dot(np.abs(A)) * SLACK
    delta = 2.0 * eta_delta(S, np.abs(mock) + gamma(K) * S, np.abs(off), K)
    ll, g = R.term(family, eta, ys, trials)
    B, rho, mag, gabs = term_bounds(family, eta, delta, ys, trials)
    return dict(eta=eta, delta=delta, ll=ll, g=g, B=B, mag=mag,
                lp=R.sum_in_kernel_order(ll, log_norm), lp_bound=logp_bound(B, mag, log_norm, N),
                force=g.dot(A.T), force_bound=force_bound(A, rho, gabs))


# ---------------------------------------------------------------------------
# the inputs of the GPU tests
# ---------------------------------------------------------------------------
def case(family, K, N, C, seed, trials=True, offset=True):
    """``(A, ys, trials, offset, theta)``: a design of mixed signs with row magnitudes
    2**-20 .. 2**10, coefficients that put eta across +-40 (standard deviation 20; beyond 40
    for one datum in twenty), counts with a few zeros, trials 1 .. 20, offsets of size 1."""
    rs = np.random.RandomState(seed)
    e = rs.randint(-20, 11, size=(K, 1))
    A = rs.standard_normal((K, N)) * 2.0 ** e
    theta = rs.standard_normal((C, K)) * (20.0 / math.sqrt(K)) / 2.0 ** e[:, 0]
    if family == R.BINOMIAL_LOGIT:
        m = rs.randint(1, 21, size=N).astype(np.float64) if trials else None
        top = np.ones(N) if m is None else m
        ys = np.floor(rs.uniform(size=N) * (top + 1.0)).clip(0.0, top)
    else:
        m = None
        ys = rs.poisson(3.0, size=N).astype(np.float64)
    off = rs.standard_normal(N) if offset else None
    return A, ys, m, off, theta


# ---------------------------------------------------------------------------
# every instantiation: the dispatch tables of csrc/glm.hip restated, and the cases that reach them
# ---------------------------------------------------------------------------
ROW_KS = (4, 8, 16, 17, 18, 32, 33, 34, 36, 48, 49, 50, 64)      # one K per table row


def table_row(K):
    """``(KS, KV)`` of glm_logp_dispatch and glm_grad_dispatch_k (the gradient's RT is
    ceil(KS / 4)): KS MFMA k-steps of four coefficients, KV trailing coefficients on the VALU."""
    for top, row in ((4, (1, 0)), (8, (2, 0)), (16, (4, 0)), (17, (4, 1)), (18, (4, 2)), (32, (8, 0)),
                     (33, (8, 1)), (34, (8, 2)), (36, (9, 0)), (48, (12, 0)), (49, (12, 1)), (50, (12, 2)),
                     (64, (16, 0))):
        if K <= top:
            return row
    raise ValueError(K)


def chain_tiles(C):
    """CT of glm_ct: 16-chain tiles per wave."""
    return 2 if C >= 4096 else 1


TABLE_ROWS = tuple(table_row(K) for K in ROW_KS)


def force_cases():
    """``(K, N, C)``: every K of ``grad_bounds.K_LIST`` with a ragged and a whole-tile N at a small
    ragged C (CT = 1), and one K per table row at C = 4100 (CT = 2).  Which case reaches which row
    is :func:`table_row` of its K; the GPU test asserts that the rows reached are all of them."""
    cases = []
    for K in GB.K_LIST:
        cases += [(K, 35, 19), (K, 48, 19)]
    cases += [(K, 17, 4100) for K in ROW_KS]
    return cases


def case_seed(K, N, C, extras):
    return 1000 * K + N + C + int(bool(extras))


def exact_chains(C, N):
    """The chains a bound test compares with exact arithmetic: both sides of the 16-chain tile,
    of the workgroup and of the two-tiles-per-wave edge, the last one; at most six (three where
    a chain costs thousands of 50-digit terms)."""
    want = 3 if N > 1000 else 6
    pick = sorted(set(c for c in (0, 15, 16, 63, 64, 4095, 4096, C - 1) if 0 <= c < C))
    return pick if len(pick) <= want else pick[:1] + pick[-(want - 1):]


def dropped_coefficients(K):
    """The coefficients whose loss a wrong table row would cause: the last one, and every one the
    row of K leaves to the VALU (KB .. KB + KV - 1)."""
    KS, KV = table_row(K)
    return sorted(set([K - 1] + [4 * KS + v for v in range(KV) if 4 * KS + v < K]))


def dropped_visibility(family, K, N, C, extras, log_norm=0.0):
    """For each coefficient of :func:`dropped_coefficients`: numpy's float64 log-prob and force of
    the generated case with that coefficient set to zero, as the largest multiple of the exact
    bound over the chains of :func:`exact_chains`: ``{k: (logp, force)}``.  Both above 1 is what
    makes a wrong row of a dispatch table visible to the GPU test."""
    A, ys, m, off, theta = case(family, K, N, C, case_seed(K, N, C, extras), trials=extras, offset=extras)
    ex = ExactGLM(family, A, ys, m, off)
    chains = exact_chains(C, N)
    exact = [ex.chain(theta[c], log_norm) for c in chains]
    out = {}
    for k in dropped_coefficients(K):
        th = theta[chains].copy()
        th[:, k] = 0.0
        ll, g = R.term(family, R.eta_of(th.dot(A), off), ys, m)
        lp = R.sum_in_kernel_order(ll, log_norm)
        force = g.dot(A.T)
        a = max(err(lp[i], e['lp']) / e['lp_bound'] for i, e in enumerate(exact))
        b = max(err(x, w) / bd for i, e in enumerate(exact)
                for x, w, bd in zip(force[i], e['force'], e['force_bound']))
        out[k] = (a, b)
    return out


# ---------------------------------------------------------------------------
# the edge ladder: each eta at which the term changes behaviour, put exactly into the kernels
# ---------------------------------------------------------------------------
def _either_side(x):
    """The two doubles around the real ``x`` (an mpf that is no double)."""
    M = R.mp()
    f = float(x)
    lo = f if M.mpf(f) < x else float(np.nextafter(f, -np.inf))
    return [lo, float(np.nextafter(lo, np.inf))]


def exp_max():
    """The last double whose ``exp`` is a double (just below 1024 log 2 = 709.78...)."""
    M = R.mp()
    return _either_side(1024 * M.log(2))[0]


def edge_ladder():
    """+-0.0, the smallest subnormal and normal, u; the doubles either side of 52 log 2 and
    53 log 2 (1 + exp(-x) rounds to 1 from the first in directed, from the second in nearest
    rounding), of 1022 log 2 (exp(-x) goes subnormal), of 1024 log 2 (exp(x) overflows) and of
    1075 log 2 (exp(-x) rounds to 0); 1e3 and 1e300.  Each with both signs."""
    M = R.mp()
    ln2 = M.log(2)
    mags = [0.0, 2.0 ** -1074, 2.0 ** -1022, 2.0 ** -53]
    for k in (52, 53, 1022, 1024, 1075):
        mags += _either_side(k * ln2)
    mags += [1e3, 1e300]
    return [s * v for v in mags for s in (1.0, -1.0)]


EDGE_N = 17
EDGE_SCALES = (1.0, 2.0, 4.0, 8.0, 1.0)          # A[0, n], period 5: powers of two >= 1
EDGE_BIG_TRIALS = 2.0 ** 20
EDGE_FULL_BELOW = 700.0                           # Poisson: beyond, logp_bound's sum of e+ overflows


def edge_case(family, variant=1):
    """``(A, ys, trials, offset, theta)`` with chain c at ``edge_ladder()[c]``.

    variant 1: K = 1, ``A[0, n]`` of EDGE_SCALES (1.0 among them; never below 1, so that a
    subnormal edge is scaled exactly), no offset: ``mock = theta * A`` is exact, and it is what the
    pointwise kernel is handed as its mock tensor.  N = 17: one full tile, one with 15 padding
    columns.
    variant 2: K = 2 and an offset: ``A[1, n] = -offset_n``, ``theta[c, 1] = 1``, so the same eta
    arises as ``(edge * A[0, n] - offset_n) + offset_n`` with both parts nonzero (exactly where
    ``edge * A[0, n] - offset_n`` is a double: every edge from 2**-53 up; the smaller ones meet
    eta = +0.0).  The offsets are positive: the second design row has one sign, and the force
    of an overflowed Poisson chain is an infinity of that sign, not inf - inf.
    variant 3: variant 1 with every ``A[0, n] = 1``: the fused kernels meet the Poisson edges
    between 700 and exp's overflow as they are (scaled by 8 they have all overflowed).

    The sign of zero: ``edge_eta`` of variants 1 and 3 carries -0.0 into the element-wise kernel.
    The fused kernels cannot receive it -- their eta is ``fma(A, theta, +0.0)`` from the
    zero-initialised accumulator, +0.0 for either sign of theta -- so they meet +0.0 twice.

    y cycles through 0, 1, m with m through 1, 2, 20, 2**20 (binomial); through 0, 1, 3, 1e6
    (Poisson).  The large m is 2**20 and not larger because m |eta| must itself be a double at
    |eta| = 8e300 for the term to be finite (glm_term.hpp: "while y * eta itself is a double")."""
    ladder = np.array(edge_ladder())
    n = np.arange(EDGE_N)
    A = np.ones((1, EDGE_N)) if variant == 3 else np.array(EDGE_SCALES)[n % 5][None, :]
    theta = ladder[:, None].copy()
    if family == R.BINOMIAL_LOGIT:
        m = np.array([1.0, 2.0, 20.0, EDGE_BIG_TRIALS])[n % 4]
        ys = np.where(n % 3 == 0, 0.0, np.where(n % 3 == 1, 1.0, m))
    else:
        m = None
        ys = np.array([0.0, 1.0, 3.0, 1e6])[n % 4]
    off = None
    if variant == 2:
        off = np.array([0.25, 0.5, 1.0, 2.0])[n % 4]
        A = np.vstack([A, -off[None, :]])
        theta = np.hstack([theta, np.ones_like(theta)])
    return A, ys, m, off, theta


def edge_eta(data):
    """numpy's eta ``[C x N]`` of an edge case.  K = 1 without an offset: the element-wise
    product, exact and with the sign of a zero edge kept (a matrix product starts from +0.0 and
    loses it)."""
    A, _, _, off, theta = data
    with np.errstate(over='ignore', under='ignore'):
        if A.shape[0] == 1 and off is None:
            return theta[:, :1] * A[0][None, :]
        return R.eta_of(theta.dot(A), off)


def edge_overflow_chains(family, data):
    """The chains with a datum whose ``exp(eta)`` overflows (Poisson only)."""
    if family != R.POISSON_LOG:
        return []
    return [int(c) for c in np.nonzero(np.any(edge_eta(data) > exp_max(), axis=1))[0]]


def edge_moderate_chains(data):
    """The chains whose every |eta| is at most 700: the leapfrog's ladder."""
    return [int(c) for c in np.nonzero(np.all(np.abs(edge_eta(data)) <= EDGE_FULL_BELOW, axis=1))[0]]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def edge_pointwise_check(family, data, mock, ll, g):
    """``binf_glm_pointwise_f64``'s ll and g ``[C x N]`` of ``mock``, the tensor the kernel was
    handed (no offset, no constants): it must be ``edge_eta(edge_case(family, 1))`` bit for bit,
    the sign of every entry that of its edge, -0.0 included.  Every datum of every edge is held
    to the exact term within ``pointwise_bound`` / ``rho`` at delta = 0 -- a Poisson datum with
    700 < eta <= 709.78 too: its per-datum bound is finite there -- except a Poisson datum whose
    exp overflows, which is ll = -inf, g = +inf exactly.  At eta = +-0.0: g = m / 2 - y exactly and
    ll = -(m fl(log 2)) where y = 0 (binomial); exp(+-0) = 1 gives ll = -1, g = 1 - y where y = 0
    (Poisson).  An edge is counted once a datum of an unscaled column (A = 1) that carries the
    ladder's value, sign bit included, has been asserted.  Returns dict(edges=<edges counted>,
    overflowed=<data>, ll=, g=<largest fractions>)."""
    A, ys, m, off, theta = data
    assert off is None and A.shape[0] == 1
    ladder = np.array(edge_ladder())
    eta = edge_eta(data)
    assert _same_bits(mock, eta), 'the kernel was not handed the edges'
    assert np.array_equal(np.signbit(eta), np.repeat(np.signbit(ladder)[:, None], eta.shape[1], axis=1))
    C, N = eta.shape
    mm = np.ones(N) if m is None else m
    ll, g = np.asarray(ll), np.asarray(g)
    assert ll.shape == (C, N) and g.shape == (C, N)
    assert not np.isnan(ll).any() and not np.isnan(g).any()
    over = (eta > exp_max()) if family == R.POISSON_LOG else np.zeros_like(eta, dtype=bool)
    with np.errstate(invalid='ignore', over='ignore'):
        B, rho, _, _ = term_bounds(family, eta, 0.0, ys[None, :], mm[None, :])
        B, rho = np.broadcast_to(B, eta.shape), np.broadcast_to(rho, eta.shape)
        # at the last double below exp's overflow mag * SLACK is no double, u mag is
        mag = _mags(family, eta, 0.0, ys[None, :], mm[None, :])['mag']
        Bp = pointwise_bound(B, None, None, umag=(U * mag) * SLACK)
    out = dict(edges=0, overflowed=int(over.sum()), ll=0.0, g=0.0)
    for c in range(C):
        seen = False              # a datum at the edge itself, as the ladder has it, asserted
        for n in range(N):
            here = A[0, n] == 1.0 and _same_bits(eta[c, n], ladder[c])
            at = (c, n, float(eta[c, n]), float(ys[n]), float(mm[n]))
            if over[c, n]:
                assert ll[c, n] == -np.inf and g[c, n] == np.inf, at
                seen = seen or here
                continue
            assert np.isfinite(ll[c, n]) and np.isfinite(g[c, n]), at
            assert np.isfinite(Bp[c, n]) and np.isfinite(rho[c, n]), at
            a = err(ll[c, n], R.exact_ll(family, float(eta[c, n]), ys[n], mm[n])) / Bp[c, n]
            b = err(g[c, n], R.exact_g(family, float(eta[c, n]), ys[n], mm[n])) / rho[c, n]
            assert a <= 1.0 and b <= 1.0, at + (a, b)
            out['ll'], out['g'] = max(out['ll'], a), max(out['g'], b)
            if eta[c, n] == 0.0:
                if family == R.BINOMIAL_LOGIT:
                    assert g[c, n] == mm[n] / 2.0 - ys[n], at
                    assert ys[n] != 0.0 or ll[c, n] == -(mm[n] * math.log(2.0)), at
                else:
                    assert g[c, n] == 1.0 - ys[n], at
                    assert ys[n] != 0.0 or ll[c, n] == -1.0, at
            seen = seen or here
        out['edges'] += int(seen)
    return out


def edge_chain_check(family, data, log_norm, lp, grad, clean=None):
    """The fused log-prob ``[C]`` and gradient ``[C x K]`` of an edge case (any variant; the
    zero edges reach these kernels as +0.0 for either sign, see :func:`edge_case`).
    Binomial, every edge, and Poisson with every eta <= 700: finite and within the exact bound
    of ``ExactGLM.chain``.  A Poisson chain with an overflowed datum: lp = -inf, every gradient
    entry +inf times the sign of its design row.  A Poisson chain with 700 < max eta <= 709.78
    and no overflow (variant 3 has three) is held to the bound by the pointwise check alone --
    above 700 ``logp_bound``'s sum of e+ overflows, and so may the kernel's own sum of 17 terms
    of e**700 and more -- and here only to what follows without a bound: every term is below
    zero and every g above it (e > y), so lp < 0 and the gradient has the sign of its design
    row, infinities allowed.  No NaN anywhere.  ``clean``: ``(lp, grad)`` of the same launch
    with the overflowed chains' coefficients zeroed -- every other chain must carry the same
    bits.  Returns dict(edges=<chains held to a bound or to the overflow rule>, full,
    overflowed, pointwise_only, logp, grad)."""
    A, ys, m, off, theta = data
    lp, grad = np.asarray(lp), np.asarray(grad)
    C, K = theta.shape
    assert lp.shape == (C,) and grad.shape == (C, K)
    assert not np.isnan(lp).any() and not np.isnan(grad).any()
    eta = edge_eta(data)
    over = set(edge_overflow_chains(family, data))
    sign = np.sign(A[:, 0])
    assert np.all(sign != 0.0) and np.all(np.sign(A) == sign[:, None])
    ex = ExactGLM(family, A, ys, m, off)
    out = dict(edges=0, full=0, overflowed=0, pointwise_only=0, logp=0.0, grad=0.0)
    for c in range(C):
        if c in over:
            assert lp[c] == -np.inf and np.array_equal(grad[c], np.inf * sign), (c, lp[c], grad[c])
            out['overflowed'] += 1
            out['edges'] += 1
        elif family == R.POISSON_LOG and np.max(eta[c]) > EDGE_FULL_BELOW:
            assert lp[c] < 0.0 and np.all(grad[c] * sign > 0.0), (c, lp[c], grad[c])
            out['pointwise_only'] += 1
        else:
            assert np.isfinite(lp[c]) and np.all(np.isfinite(grad[c])), (c, lp[c], grad[c])
            e = ex.chain(theta[c], log_norm)
            assert np.isfinite(e['lp_bound']) and np.all(np.isfinite(e['force_bound'])), c
            a = err(lp[c], e['lp']) / e['lp_bound']
            b = max(err(x, w) / bd for x, w, bd in zip(grad[c], e['force'], e['force_bound']))
            assert a <= 1.0 and b <= 1.0, (c, float(theta[c, 0]), a, b)
            out['logp'], out['grad'] = max(out['logp'], a), max(out['grad'], b)
            out['full'] += 1
            out['edges'] += 1
    if clean is not None:
        keep = [c for c in range(C) if c not in over]
        assert np.array_equal(lp[keep].view(np.int64), np.asarray(clean[0])[keep].view(np.int64))
        assert np.array_equal(grad[keep].view(np.int64), np.asarray(clean[1])[keep].view(np.int64))
    return out


def edge_counts(family, data):
    """What :func:`edge_chain_check` must report for ``data``, from the ladder alone:
    ``(edges, full, overflowed, pointwise_only)``; edges + pointwise_only is the ladder's length."""
    ladder = edge_ladder()
    if family == R.BINOMIAL_LOGIT:
        return len(ladder), len(ladder), 0, 0
    top = float(np.max(data[0][0]))
    over = sum(1 for e in ladder if e * top > exp_max())
    mid = sum(1 for e in ladder if EDGE_FULL_BELOW < e * top <= exp_max())
    return len(ladder) - mid, len(ladder) - over - mid, over, mid


def self_test(seed=0):
    """numpy's own float64 results lie inside the bounds; the same with ONE mock datum moved by
    1e-9 of its S_n, with a dropped ``m``, and with the gradient's sign flipped lie outside."""
    out = []
    for family in R.FAMILIES:
        for K, N in ((5, 17), (33, 100)):
            A, ys, m, off, theta = case(family, K, N, 1, seed + K)
            ex = ExactGLM(family, A, ys, m, off)
            c = ex.chain(theta[0], 1.25)
            mock = theta[0].dot(A)
            ll, g = R.term(family, R.eta_of(mock, off), ys, m)
            lp = float(R.sum_in_kernel_order(ll, 1.25)[0])
            assert err(lp, c['lp']) <= c['lp_bound'], (family, K, N)
            f = g.dot(A.T)
            fe = np.array([err(a, b) for a, b in zip(f, c['force'])])
            assert np.all(fe <= c['force_bound']), (family, K, N)
            S = np.abs(theta[0]).dot(np.abs(A))
            n = int(np.argmax(c['B']))
            bad = mock.copy()
            bad[n] += 1e-9 * S[n]
            lb, gb = R.term(family, R.eta_of(bad, off), ys, m)
            moved = err(float(R.sum_in_kernel_order(lb, 1.25)[0]), c['lp']) / c['lp_bound']
            flipped = np.array([err(-a, b) for a, b in zip(f, c['force'])]) / c['force_bound']
            assert np.max(flipped) > 1.0, 'the force bound does not see a flipped sign'
            fig = dict(family=family, K=K, N=N, lp=err(lp, c['lp']) / c['lp_bound'],
                       force=float(np.max(fe / c['force_bound'])), moved=moved,
                       flipped=float(np.max(flipped)))
            if family == R.BINOMIAL_LOGIT:
                l1, _ = R.term(family, R.eta_of(mock, off), ys, None)
                fig['dropped_m'] = err(float(R.sum_in_kernel_order(l1, 1.25)[0]), c['lp']) / c['lp_bound']
                assert fig['dropped_m'] > 1.0, 'the log-prob bound does not see a dropped m'
            out.append(fig)
    return out
