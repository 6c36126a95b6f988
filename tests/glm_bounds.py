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
                ``B_n = max(y, m - y) delta + 2 u y H + m (8u t + 8u L + 3 u sp+) + 4 TINY``
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
                ``rho_n = m delta / 4 + 20 u m s+ + u y + 3 TINY``,  s+ <= 1
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
"""
import math

import numpy as np

import glm_ref as R
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
            m * (8 * U * q['t'] + 8 * U * q['L'] + 3 * U * q['sp']) + 4 * TINY
        rho = m * delta / 4 + 20 * U * m + U * y + 3 * TINY
    else:
        with np.errstate(invalid='ignore'):         # an overflowed e with delta = 0: no bound
            B = (y + q['e']) * delta + 2 * U * y * q['H'] + 10 * U * q['e'] + 3 * TINY
            rho = q['e'] * delta + 8 * U * q['e'] + U * (q['e'] + y) + 2 * TINY
    return B * SLACK, rho * SLACK, q['mag'] * SLACK, q['g'] * SLACK


def logp_bound(B, mag, log_norm, N):
    """The log-prob bound from the per-datum bounds (summed over the last axis)."""
    s = np.sum(mag + B, axis=-1)
    return (np.sum(B, axis=-1) + (gamma(N + 1) + U) * s + U * abs(log_norm)) * SLACK


def pointwise_bound(B, mag, lconst):
    """One datum of the record: its term's bound and the rounding of ``+ lconst_n``."""
    lc = 0.0 if lconst is None else np.abs(lconst)
    return (B + U * (mag + B + lc)) * SLACK


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

    def __init__(self, family, A, ys, trials=None, offset=None):
        self.family = family
        self.A = np.asarray(A, dtype=np.float64)
        self.K, self.N = self.A.shape
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
        delta = eta_delta(S, mock_abs, np.abs(self.off), self.K)
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
