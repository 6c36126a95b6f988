"""Host restatement of the negative-binomial error term (``binf_amd/csrc/glm_term.hpp``), of
the count term's two orders (``binf_amd/csrc/negbin.hip``) and of the orders in which
``binf_amd/csrc/glm.hip`` sums the terms, in numpy float64; and the same at 50 digits in mpmath,
the truth both are measured from.  Host only.  Line for line:

    lam~ = clamp(lam, -708, 709)      phi = exp(lam~)          (one exp per chain)
    z = eta - lam~                    m = y + phi
    then glm_ref.term(BINOMIAL_LOGIT, z, y, m):  ll = y z - m sp(z)   g = m s(z) - y
    log_norm_chain[c] = tree(fl(T_j fl(log(fl(phi + j))))) + log_norm
    prefix[s][k]      = running sum over j = 0, 1, ... of fl(log(fl(phi + j))), read at j = v_k
    record[s][n]      = (ll + prefix[s][index[n]]) + lconst[n]
    log-prob[c]       = glm_ref.sum_in_kernel_order(ll)[c] + log_norm_chain[c]
    a chain with lam outside [-708, 709] (NaN included): log_norm_chain, record and log-prob -inf

numpy's exp and log are the host library's: they agree with the device's to rounding, not bit
for bit (``negbin_bounds`` allows each its error)."""
import numpy as np

import glm_ref as R

NEGBIN_LOG = 2
LAM_MIN, LAM_MAX = -708.0, 709.0
MAX_COUNT = 1 << 20
DPS = R.DPS
mp = R.mp


def regular(lam):
    lam = np.asarray(lam, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        return (lam >= LAM_MIN) & (lam <= LAM_MAX)


def clamp(lam):
    """negbin_lam: the nearer end of the range, LAM_MIN for a NaN."""
    lam = np.asarray(lam, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        return np.where(lam >= LAM_MIN, np.where(lam <= LAM_MAX, lam, LAM_MAX), LAM_MIN)


def phi_of(lam):
    return np.exp(clamp(lam))


def term(eta, y, lam):
    """``(ll, g)`` of ``eta`` [C x N] (or [N]) under ``lam`` [C] (or a scalar)."""
    eta = np.asarray(eta, dtype=np.float64)
    lc = clamp(lam)
    phi = np.exp(lc)
    if eta.ndim == 2 and np.ndim(lc) == 1:
        lc, phi = lc[:, None], phi[:, None]
    z = eta - lc
    m = np.asarray(y, dtype=np.float64) + phi
    return R.term(R.BINOMIAL_LOGIT, z, y, m)


def tail_counts(ys):
    """``T_j = #{n: y_n > j}``, j = 0 .. max(ys) - 1, as int64."""
    yi = np.asarray(ys).astype(np.int64)
    ymax = int(yi.max()) if yi.size else 0
    return np.array([int(np.sum(yi > j)) for j in range(ymax)], dtype=np.int64)


def count_term(lam, tail, log_norm):
    """``out_chain`` of binf_negbin_count_term_f64 for ``lam`` [C]: thread t of 256 sums
    j = t, t + 256, ... ascending from 0.0; a wave's 64 by the butterfly x += x[lane ^ o],
    o = 1 .. 32; the four waves as (0 + 1) + (2 + 3); ``log_norm`` last; -inf outside the range."""
    lam = np.atleast_1d(np.asarray(lam, dtype=np.float64))
    phi = phi_of(lam)
    T = np.asarray(tail, dtype=np.float64)
    ymax = T.shape[0]
    acc = np.zeros((lam.shape[0], 256))
    with np.errstate(divide='ignore'):
        for j in range(ymax):
            x = phi + float(j)
            acc[:, j % 256] = acc[:, j % 256] + T[j] * np.log(x)
    a = acc.reshape(-1, 4, 64)
    lanes = np.arange(64)
    for o in (1, 2, 4, 8, 16, 32):
        a = a + a[:, :, lanes ^ o]
    w = a[:, :, 0]
    s = ((w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])) + log_norm
    return np.where(regular(lam), s, -np.inf)


def prefix(lam, values):
    """``out_prefix`` [S x J]: one running sum over j = 0, 1, ... from 0.0, read at values[k]."""
    lam = np.atleast_1d(np.asarray(lam, dtype=np.float64))
    phi = phi_of(lam)
    out = np.zeros((lam.shape[0], len(values)))
    acc = np.zeros(lam.shape[0])
    j = 0
    for k, v in enumerate(values):
        while j < v:
            acc = acc + np.log(phi + float(j))
            j += 1
        out[:, k] = acc
    return out


def pointwise(mock, ys, offset, lam, pre=None, index=None, lconst=None):
    """``(out_ll, out_grad)`` of binf_negbin_pointwise_f64 for ``mock`` [S x N]."""
    ll, g = term(R.eta_of(mock, offset), ys, lam)
    if pre is not None:
        ll = ll + pre[:, index]
    if lconst is not None:
        ll = ll + lconst
    return np.where(regular(lam)[:, None], ll, -np.inf), g


def logp(theta, A, ys, offset, lam, lnc):
    """The fused log-prob with numpy's own matrix product for the mock data."""
    ll, _ = term(R.eta_of(np.atleast_2d(theta).dot(A), offset), ys, lam)
    s = R.sum_in_kernel_order(ll, 0.0) + lnc
    return np.where(regular(lam), s, -np.inf)


def grad(theta, A, ys, offset, lam):
    _, g = term(R.eta_of(np.atleast_2d(theta).dot(A), offset), ys, lam)
    return g.dot(A.T)


# ---------------------------------------------------------------------------
# the truth at 50 digits: lam is the given input, phi = exp(lam) exactly
# ---------------------------------------------------------------------------
def exact_ll(eta, y, lam):
    M = mp()
    lam = M.mpf(float(lam))
    return R.exact_ll(R.BINOMIAL_LOGIT, M.mpf(eta) - lam, y, M.mpf(y) + M.exp(lam))


def exact_g(eta, y, lam):
    M = mp()
    lam = M.mpf(float(lam))
    return R.exact_g(R.BINOMIAL_LOGIT, M.mpf(eta) - lam, y, M.mpf(y) + M.exp(lam))


def exact_prefix(lam, v):
    """``sum_{j<v} log(phi + j)`` as an mpf."""
    M = mp()
    phi = M.exp(M.mpf(float(lam)))
    return M.fsum(M.log(phi + j) for j in range(int(v)))


def exact_count(lam, tail):
    """``sum_j T_j log(phi + j)`` as an mpf."""
    M = mp()
    phi = M.exp(M.mpf(float(lam)))
    return M.fsum(int(t) * M.log(phi + j) for j, t in enumerate(tail))


def textbook_log_density(eta, y, lam, dps=150):
    """``lgamma(y + phi) - lgamma(phi) - lgamma(y + 1) + phi log phi + y eta - (y + phi)
    log(phi + mu)``, mu = exp(eta): the NB2 log density as the textbooks write it (mpf).  Its
    parts cancel -- at phi = e**30 they are 1e15 against a result that may be 1e-18 -- so it is
    evaluated at ``dps`` digits, the precision the kernels' form does not need."""
    M = mp()
    with M.workdps(dps):
        eta, lam = M.mpf(eta), M.mpf(float(lam))
        phi, mu = M.exp(lam), M.exp(eta)
        return +(M.loggamma(y + phi) - M.loggamma(phi) - M.loggamma(M.mpf(y) + 1) + phi * lam + y * eta -
                 (y + phi) * M.log(phi + mu))


def exact_log_density(eta, y, lam):
    """The form the kernels split: term + prefix - lgamma(y + 1) (mpf)."""
    M = mp()
    return exact_ll(eta, y, lam) + exact_prefix(lam, y) - M.loggamma(M.mpf(y) + 1)
