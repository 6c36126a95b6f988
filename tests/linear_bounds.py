"""Derived error bounds for the linear forward model + Gaussian error model
(``binf_linear_forward_f64`` / ``binf_linear_gauss_logp_f64``), and the exact values
they are measured from.  Nothing here is a measured tolerance.

With ``u = 2**-53``, ``gamma_m = m u / (1 - m u)`` and ``S_n = sum_k |theta_k| |A_kn|``:

mock     ``|mock_n - exact| <= delta_n = gamma_K S_n`` -- K products and K - 1 additions,
         each rounded at most once, in ANY order, fused or not (Higham, Accuracy and
         Stability of Numerical Algorithms, 2nd ed., (3.5)).
chi^2    ``|chi2 - exact| <= sum_n (2 |r_n| rho_n + rho_n**2) + gamma_{N+1} chi2_exact``
         with ``r_n`` the exact residual and ``rho_n = delta_n + u (|r_n| + delta_n)`` the
         error of the computed residual (the mock datum's error plus one rounding of the
         subtraction); squaring and summing N terms in any order adds ``gamma_{N+1}``.
log-prob ``0.5 tau`` times the chi^2 bound plus ``8 u`` of the magnitude of each of the
         two terms ``0.5 tau chi2`` and ``0.5 N log tau`` (one ulp of the device's log and
         the roundings of the epilogue).

The exact values are computed in integer arithmetic: every double is an integer times a
power of two, so products and sums of doubles are exact integers over a common power of
two (the same numbers ``fractions.Fraction`` gives, much faster).  ``log tau`` is taken
from mpmath at 60 digits.

The bounds themselves are evaluated in double precision; ``SLACK = 1 + 2**-30`` covers
the roundings of that evaluation (a few thousand operations of relative error u each).

For the chains that are NOT compared with exact arithmetic the bound is evaluated on
numpy's float64 residuals ``r~``: since numpy's own result obeys the model above,
``|r_n| <= |r~_n| + rho_n`` and ``chi2_exact <= (chi2~ + first) / (1 - gamma_{N+1})``,
which is what :func:`chi2_bound_float` uses.
"""
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
SLACK = 1.0 + 2.0 ** -30


def gamma(m):
    return m * U / (1.0 - m * U)


# ---------------------------------------------------------------------------
# exact arithmetic on doubles
# ---------------------------------------------------------------------------
def to_ints(x):
    """``(m, s)`` with ``x == m / 2**s`` exactly: ``m`` an object array of Python ints."""
    x = np.asarray(x, dtype=np.float64)
    if not np.all(np.isfinite(x)):
        raise ValueError('exact arithmetic needs finite values')
    ratios = [float(v).as_integer_ratio() for v in x.ravel()]
    shifts = [d.bit_length() - 1 for _, d in ratios]
    s = max(shifts) if shifts else 0
    m = np.empty(len(ratios), dtype=object)
    for i, ((n, _), si) in enumerate(zip(ratios, shifts)):
        m[i] = n << (s - si)
    return m.reshape(x.shape), s


def abs_floats(ints, shift):
    """``|ints[j]| / 2**shift`` as doubles, each correctly rounded."""
    return np.array([float(Fraction(abs(int(v)), 1 << shift)) for v in ints], dtype=np.float64)


class Exact(object):
    """Exact mock data, residuals and chi^2 of chains against one data set."""

    def __init__(self, A, ys):
        self.A = np.asarray(A, dtype=np.float64)
        self.y = np.asarray(ys, dtype=np.float64)
        self.K, self.N = self.A.shape
        self.mA, self.sA = to_ints(self.A)
        self.mY, self.sY = to_ints(self.y)
        self.absA = np.abs(self.A)

    def mock(self, theta):
        """``(M, s)``: exact mock data ``M[n] / 2**s`` of one chain."""
        mT, sT = to_ints(theta)
        M = np.dot(mT, self.mA) if self.N else np.empty(0, dtype=object)
        return np.asarray(M, dtype=object).reshape(self.N), sT + self.sA

    def residual(self, theta):
        """``(M, s, R, sr)``: the exact mock data and the exact residuals ``R[n] / 2**sr``
        (mock minus data) of one chain."""
        M, s = self.mock(theta)
        return M, s, M * (1 << self.sY) - self.mY * (1 << s), s + self.sY

    def chain(self, theta):
        """dict(mock=(M, s), S=S_n, delta=delta_n, r=|r_n| as floats, chi2=Fraction,
        chi2_bound=float) for one chain."""
        theta = np.asarray(theta, dtype=np.float64)
        M, s, R, sr = self.residual(theta)
        chi2 = Fraction(int(np.sum(R * R)) if self.N else 0, 1 << (2 * sr))
        S = np.abs(theta).dot(self.absA) * SLACK
        delta = gamma(self.K) * S * SLACK
        rabs = abs_floats(R, sr) * SLACK
        rho = (delta + U * (rabs + delta)) * SLACK
        bound = (float(np.sum(2.0 * rabs * rho + rho * rho)) +
                 gamma(self.N + 1) * float(chi2)) * SLACK
        return dict(mock=(M, s), S=S, delta=delta, r=rabs, chi2=chi2, chi2_bound=bound)

    def mock_error(self, theta, got):
        """``|got_n - exact mock_n|`` as floats (rounded up by SLACK)."""
        M, s = self.mock(theta)
        G, sg = to_ints(got)
        sh = max(s, sg)
        D = G * (1 << (sh - sg)) - M * (1 << (sh - s))
        return abs_floats(D, sh)


def logp_exact_and_bound(chi2, chi2_bound, tau, N):
    """``(exact log-prob as mpmath.mpf, bound)`` from an exact chi^2 and its bound."""
    import mpmath
    mpmath.mp.dps = 60
    t = mpmath.mpf(float(tau))
    c = mpmath.mpf(chi2.numerator) / mpmath.mpf(chi2.denominator)
    a = c * t / 2
    b = mpmath.mpf(N) * mpmath.log(t) / 2
    bound = (0.5 * float(tau) * chi2_bound + 8 * U * (float(abs(a)) + float(abs(b)))) * SLACK
    return b - a, bound


def logp_error(got, exact):
    import mpmath
    mpmath.mp.dps = 60
    return float(abs(mpmath.mpf(float(got)) - exact))


# ---------------------------------------------------------------------------
# the same bounds on numpy's float64 values, for every chain of a batch
# ---------------------------------------------------------------------------
def mock_bound_float(theta, A):
    """delta [C x N]"""
    K = A.shape[0]
    return gamma(K) * np.abs(theta).dot(np.abs(A)) * SLACK * SLACK


def chi2_bound_float(theta, A, ys):
    """``(numpy mock [C x N], numpy chi2 [C], bound [C])`` -- see the module docstring."""
    N = A.shape[1]
    delta = mock_bound_float(theta, A)
    mock = theta.dot(A)
    r = np.abs(mock - ys)
    rho = (delta + U * (r + 2.0 * delta)) * SLACK
    first = np.sum(2.0 * (r + rho) * rho + rho * rho, axis=1)
    chi2 = np.sum((mock - ys) ** 2, axis=1)
    g = gamma(N + 1)
    return mock, chi2, (first + g / (1.0 - g) * (chi2 + first)) * SLACK


def logp_float(theta, A, ys, tau):
    """``(numpy log-prob [C], bound [C])`` with ``tau`` a scalar or ``[C]``."""
    N = A.shape[1]
    _, chi2, cb = chi2_bound_float(theta, A, ys)
    tau = np.broadcast_to(np.asarray(tau, dtype=np.float64), chi2.shape)
    a = 0.5 * chi2 * tau
    b = N * 0.5 * np.log(tau)
    return -0.5 * chi2 * tau + b, (0.5 * tau * cb + 8 * U * (np.abs(a) + 0.5 * tau * cb + np.abs(b))) * SLACK


# ---------------------------------------------------------------------------
# self-test: a bound that cannot fail shows nothing
# ---------------------------------------------------------------------------
def self_test(seed=0):
    """numpy's own float64 results lie inside the bounds; the same results with ONE mock
    datum moved by 1e-9 of its S_n lie outside them.  Returns the figures."""
    rs = np.random.RandomState(seed)
    out = []
    for K, N in ((4, 20), (7, 37), (33, 1000)):
        A = rs.standard_normal((K, N))
        theta = rs.standard_normal(K)
        ys = theta.dot(A) + 0.05 * rs.standard_normal(N)
        tau = 3.7
        ex = Exact(A, ys)
        c = ex.chain(theta)
        mock = theta.dot(A)
        err = ex.mock_error(theta, mock)
        assert np.all(err <= c['delta']), (K, N, float(np.max(err / c['delta'])))
        chi2 = float(np.sum((mock - ys) ** 2))
        chi2_err = float(abs(Fraction(chi2) - c['chi2']))
        assert chi2_err <= c['chi2_bound'], (K, N, chi2_err, c['chi2_bound'])
        lp_exact, lp_bound = logp_exact_and_bound(c['chi2'], c['chi2_bound'], tau, N)
        lp = -0.5 * chi2 * tau + N * 0.5 * np.log(tau)
        assert logp_error(lp, lp_exact) <= lp_bound
        # the float-evaluated bound contains the exact one's verdict
        lpf, bf = logp_float(theta[None, :], A, ys, tau)
        assert logp_error(lpf[0], lp_exact) <= bf[0] and bf[0] >= lp_bound * (1 - 1e-6)
        # injected error: one datum off by 1e-9 of S_n
        n = int(np.argmax(c['r']))
        bad = mock.copy()
        bad[n] += 1e-9 * c['S'][n]
        err_bad = ex.mock_error(theta, bad)
        assert err_bad[n] > c['delta'][n], 'the mock bound does not see 1e-9 S_n'
        chi2_bad = float(np.sum((bad - ys) ** 2))
        chi2_bad_err = float(abs(Fraction(chi2_bad) - c['chi2']))
        assert chi2_bad_err > c['chi2_bound'], 'the chi^2 bound does not see 1e-9 S_n'
        lp_bad = -0.5 * chi2_bad * tau + N * 0.5 * np.log(tau)
        assert logp_error(lp_bad, lp_exact) > lp_bound, 'the log-prob bound does not see 1e-9 S_n'
        out.append(dict(K=K, N=N, mock=float(np.max(err / c['delta'])),
                        chi2=chi2_err / c['chi2_bound'],
                        chi2_injected=chi2_bad_err / c['chi2_bound']))
    return out
