"""Host restatement of the generalised-linear error terms (``binf_amd/csrc/glm_term.hpp``) and
of the orders in which ``binf_amd/csrc/glm.hip`` sums them, in numpy float64; and the same
terms in mpmath at 50 digits, the truth both are measured from.  Host only.

The restatement follows the header line for line, every operation rounded on its own:

    eta = mock + offset                         (offset 0.0 when absent)
    binomial-logit:  t = exp(-|eta|)   sp = max(eta, 0) + log1p(t)   ll = y eta - m sp
                     s = eta >= 0 ? 1 / (1 + t) : t / (1 + t)        g = m s - y
    Poisson-log:     e = exp(eta)      ll = y eta - e                g = e - y

numpy's exp and log1p are the host library's, the device's are its own: the two agree to
rounding, not bit for bit (the bound of ``glm_bounds`` allows each its error)."""
import numpy as np

BINOMIAL_LOGIT, POISSON_LOG = 0, 1
FAMILIES = (BINOMIAL_LOGIT, POISSON_LOG)
PIECE = 1024                     # data points per piece (GLM_PIECE_TILES * 16)
DPS = 50


def eta_of(mock, offset=None):
    return np.asarray(mock, dtype=np.float64) + (0.0 if offset is None else offset)


def term(family, eta, y, m=None):
    """``(ll, g)`` of glm_term.hpp, elementwise; ``m`` None: 1.0."""
    eta = np.asarray(eta, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    m = 1.0 if m is None else np.asarray(m, dtype=np.float64)
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        if family == BINOMIAL_LOGIT:
            t = np.exp(-np.abs(eta))
            sp = np.maximum(eta, 0.0) + np.log1p(t)
            ll = y * eta - m * sp
            d = 1.0 + t
            s = np.where(eta >= 0.0, 1.0 / d, t / d)
            g = m * s - y
        elif family == POISSON_LOG:
            e = np.exp(eta)
            ll = y * eta - e
            g = e - y
        else:
            raise ValueError(family)
    return ll, g


def pointwise(family, mock, ys, trials=None, offset=None, lconst=None):
    """``(out_ll, out_grad)`` of ``binf_glm_pointwise_f64`` for ``mock`` [S x N]."""
    ll, g = term(family, eta_of(mock, offset), ys, trials)
    return (ll if lconst is None else ll + lconst), g


def sum_in_kernel_order(ll, log_norm=0.0):
    """``binf_linear_glm_logp_f64``'s sum of the terms ``ll`` [C x N] of each chain: pieces of
    1024 points; inside a piece lane lk sums n = lk, lk + 4, ... ascending from 0.0; the four
    as (0 + 1) + (2 + 3); pieces in piece order; ``log_norm`` last."""
    ll = np.atleast_2d(np.asarray(ll, dtype=np.float64))
    C, N = ll.shape
    total = None
    for p0 in range(0, max(N, 1), PIECE):
        piece = ll[:, p0:p0 + PIECE]
        lanes = []
        for lk in range(4):
            acc = np.zeros(C)
            # tile by tile: n = 16 t + lk + 4 r, r = 0 .. 3 -- ascending n of this residue class
            idx = [n for n in range(piece.shape[1]) if n % 4 == lk]
            for n in idx:
                acc = acc + piece[:, n]
            lanes.append(acc)
        s = (lanes[0] + lanes[1]) + (lanes[2] + lanes[3])
        total = s if total is None else total + s
    return total + log_norm


def logp(family, theta, A, ys, trials=None, offset=None, log_norm=0.0):
    """The fused log-prob with numpy's own matrix product for the mock data."""
    ll, _ = term(family, eta_of(np.atleast_2d(theta).dot(A), offset), ys, trials)
    return sum_in_kernel_order(ll, log_norm)


def grad(family, theta, A, ys, trials=None, offset=None):
    """The fused gradient ``[C x K]`` with numpy's products (its own summation order)."""
    _, g = term(family, eta_of(np.atleast_2d(theta).dot(A), offset), ys, trials)
    return g.dot(A.T)


# ---------------------------------------------------------------------------
# the truth: the same terms at 50 digits
# ---------------------------------------------------------------------------
def mp():
    import mpmath
    mpmath.mp.dps = DPS
    return mpmath


def exact_ll(family, eta, y, m=1):
    """``ll`` of one datum as an mpmath.mpf, ``eta`` an mpf (or an exact double)."""
    M = mp()
    eta, y, m = M.mpf(eta), M.mpf(y), M.mpf(m)
    if family == BINOMIAL_LOGIT:
        sp = (eta if eta > 0 else M.mpf(0)) + M.log1p(M.exp(-abs(eta)))
        return y * eta - m * sp
    return y * eta - M.exp(eta)


def exact_g(family, eta, y, m=1):
    """``g = -d ll / d eta`` in closed form, as an mpf."""
    M = mp()
    eta, y, m = M.mpf(eta), M.mpf(y), M.mpf(m)
    if family == BINOMIAL_LOGIT:
        t = M.exp(-abs(eta))
        s = 1 / (1 + t) if eta >= 0 else t / (1 + t)
        return m * s - y
    return M.exp(eta) - y


def exact_g_by_differences(family, eta, y, m=1):
    """``-d ll / d eta`` by a central difference of :func:`exact_ll` at 50 digits with
    h = 10**-15 max(1, |eta|) -- its truncation error h**2 |ll'''| / 6 <= 1e-30 m max(1, e**eta)
    scale is far below any double's rounding."""
    M = mp()
    eta = M.mpf(eta)
    h = M.mpf(10) ** -15 * max(1, abs(eta))
    return -(exact_ll(family, eta + h, y, m) - exact_ll(family, eta - h, y, m)) / (2 * h)


def exact_log_norm_terms(family, ys, trials=None):
    """The per-observation constants at 50 digits (mpf list)."""
    M = mp()
    out = []
    for i, y in enumerate(ys):
        y = int(y)
        if family == BINOMIAL_LOGIT:
            m = 1 if trials is None else int(trials[i])
            out.append(M.log(M.binomial(m, y)))
        else:
            out.append(-M.loggamma(y + 1))
    return out
