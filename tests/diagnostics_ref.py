"""Host restatement (numpy) of the convergence diagnostics of ``csrc/diagnostics.hip`` /
``binf_amd/diagnostics.py``, written from the contract in ``include/binf_hip.h``: per-chain
moments, lagged autocovariances, split-R^ and Geyer's effective sample size.  Nothing here
calls into the library.

Draws ``x[t, c, i]``, ``split`` in {1, 2}, ``n = T // split``; segment 0 is draws ``[0, n)``,
segment 1 is ``[T - n, T)``; split chain ``m = s * C + c``, ``M = split * C``.  Every multiply
and add is one numpy operation on float64, so each is rounded separately.  Sums over draws
are sequential from 0.0 (:func:`seq_sum`); sums over split chains are sequential from 0.0
inside blocks of 64 consecutive ``m`` and then sequential from 0.0 over the block sums
(:func:`blocked_sum`).

    K0 = x[first draw],  d_t = x_t - K0,  s1 = sum d_t,  s2 = sum d_t * d_t
    mean = K0 + s1 / n,  m2 = s2 - (s1 * s1) / n
    c_i = x_i - mean,    a_m(k) = (sum_{i < n - k} c_i * c_{i+k}) / n
    W = blocked(m2 / (n - 1)) / M,  g = blocked(mean) / M,  Bn = blocked((mean - g)^2) / (M - 1)
    varplus = ((n - 1) / n) * W + Bn,  rhat = sqrt(varplus / W)
    A(k) = (sum_b partial[b, k]) / M,  rho(k) = 1 - (W - (A(k) * n) / (n - 1)) / varplus
    P_j = rho(2j) + rho(2j + 1) while 2j + 1 <= K; stop at the first P_j < 0; P_j = P_{j-1}
    if P_{j-1} < P_j;  tau = -1 + 2 sum P_j;  ess = (M * n) / tau;  mcse = sqrt(varplus / ess)

Error bounds (the standard model fl(a op b) = (a op b)(1 + delta), |delta| <= u = 2^-53, no
underflow; gamma_k = k u / (1 - k u)), all against exact arithmetic ON THE RESTATEMENT'S OWN
ROUNDED d_t (resp. c_i), which is what ``tests/test_diagnostics.py`` evaluates with
``fractions.Fraction``.  Write S1 = sum d_t, S2 = sum d_t^2, Sa = sum |d_t| exactly.

* s1: n adds, the first onto 0.0 exact:          |s1 - S1| <= gamma_n Sa.
* s2: one rounding per product, n adds:          |s2 - S2| <= gamma_{n+1} S2.
* mean: q = fl(s1 / n) has |q - S1/n| <= (gamma_n + u (1 + gamma_n)) Sa / n <= gamma_{n+1} Sa / n,
  and mean = (K0 + q)(1 + delta), so
      |mean - (K0 + S1/n)| <= gamma_{n+1} Sa / n + u |mean| / (1 - u).
* m2: |s1^2 - S1^2| = |s1 - S1| |s1 + S1| <= gamma_n (2 + gamma_n) Sa^2, and Sa^2 <= n S2
  (Cauchy-Schwarz), so r = fl(fl(s1 s1) / n) has
      |r - S1^2/n| <= [gamma_n (2 + gamma_n) + gamma_2 (1 + gamma_n)^2] S2,
  and with the last subtraction's rounding on |s2| + |r|
      |m2 - (S2 - S1^2/n)| <= [gamma_{n+1} + gamma_n (2 + gamma_n) + gamma_2 (1 + gamma_n)^2
                               + u ((1 + gamma_{n+1}) + (1 + gamma_2)(1 + gamma_n)^2)] S2
  (:func:`m2_bound_factor`; about (3n + 5) u).  The bound is relative to S2 = sum (x_t - K0)^2,
  NOT to m2: S2 = m2 + n (K0 - mean)^2, so a first draw that lies z standard deviations from
  the chain's mean loses a factor of about 1 + z^2 against a centred two-pass variance.  The
  shift removes the offset of the whole chain (a chain at 1e9 +- 1 is as good as one at 0 +- 1);
  it is only as good as the first draw is typical.
* a_m(k): n - k products, n - k adds, one division: at most n + 2 roundings on every term,
      |a_m(k) - (sum c_i c_{i+k}) / n| <= gamma_{n+2} (sum |c_i c_{i+k}|) / n.
"""
import numpy as np

BLOCK = 64
U = 2.0 ** -53


def gamma(k):
    return k * U / (1.0 - k * U)


def m2_bound_factor(n):
    """The bracket of the m2 bound above, as a float (n in the thousands: well below 1)."""
    gn, gn1, g2 = gamma(n), gamma(n + 1), gamma(2)
    return gn1 + gn * (2 + gn) + g2 * (1 + gn) ** 2 + U * ((1 + gn1) + (1 + g2) * (1 + gn) ** 2)


def seq_sum(a):
    """Sum over axis 0, sequential from 0.0 (np.add.accumulate adds one element at a time)."""
    a = np.asarray(a, dtype=np.float64)
    with np.errstate(all='ignore'):
        return np.add.accumulate(np.concatenate([np.zeros((1,) + a.shape[1:]), a], axis=0), axis=0)[-1]


def block_sums(v):
    """[ceil(M / 64), ...]: the sum of every block of 64 consecutive entries of axis 0."""
    M = v.shape[0]
    return np.stack([seq_sum(v[b:b + BLOCK]) for b in range(0, M, BLOCK)], axis=0)


def blocked_sum(v):
    return seq_sum(block_sums(v))


def segments(x, split):
    """[n, M, D]: the split chains side by side, m = s * C + c."""
    x = np.asarray(x, dtype=np.float64)
    T = x.shape[0]
    assert split in (1, 2) and T // split >= 2
    n = T // split
    return x[:n] if split == 1 else np.concatenate([x[:n], x[T - n:]], axis=1)


def moments(x, split=1):
    """dict(n, M, K0, d, s1, s2, mean, m2), the last six [M x D] (d: [n x M x D])."""
    xs = segments(x, split)
    n = xs.shape[0]
    fn = np.float64(n)
    with np.errstate(all='ignore'):
        K0 = xs[0]
        d = xs - K0
        s1 = seq_sum(d)
        s2 = seq_sum(d * d)
        mean = K0 + s1 / fn
        m2 = s2 - (s1 * s1) / fn
    return dict(n=n, M=xs.shape[1], K0=K0, d=d, s1=s1, s2=s2, mean=mean, m2=m2)


def centred(x, split, mean):
    with np.errstate(all='ignore'):
        return segments(x, split) - mean


def autocov_chains(x, split, mean, max_lag):
    """a_m(k): [K + 1, M, D]."""
    c = centred(x, split, mean)
    n = c.shape[0]
    assert 0 <= max_lag <= n - 1
    with np.errstate(all='ignore'):
        return np.stack([seq_sum(c[:n - k] * c[k:]) / np.float64(n) for k in range(max_lag + 1)], axis=0)


def autocov_partials(a):
    """[ceil(M / 64), K + 1, D]: what the device leaves in its workspace."""
    return np.stack([block_sums(a[k]) for k in range(a.shape[0])], axis=1)


def default_max_lag(n):
    return min(n - 1, 64)


def tail(W, varplus, A, n, M):
    """Geyer's initial monotone sequence for ONE dimension: (ess, mcse, truncated) from the
    scalars W, varplus and A[0 .. K]."""
    f = np.float64
    fn, fn1, fM = f(n), f(n - 1), f(M)
    K = len(A) - 1
    total, prev, negative = f(0.0), f(0.0), False
    with np.errstate(all='ignore'):
        rho = lambda k: f(1.0) - (W - (A[k] * fn) / fn1) / varplus
        j = 0
        while 2 * j + 1 <= K:
            P = rho(2 * j) + rho(2 * j + 1)
            if P < 0.0:
                negative = True
                break
            if j > 0 and prev < P:
                P = prev
            total = total + P
            prev = P
            j += 1
        tau = f(-1.0) + f(2.0) * total
        ess = (fM * fn) / tau
        mcse = np.sqrt(varplus / ess)
    return ess, mcse, 0 if negative else 1


def summary(mean, m2, partials, n):
    """The across-chain step: dict(post_mean, W, Bn, varplus, sd, rhat[, ess, mcse, truncated]),
    each [D].  ``partials`` None: R^ only."""
    M, D = mean.shape
    assert M >= 2 and n >= 2
    f = np.float64
    with np.errstate(all='ignore'):
        W = blocked_sum(m2 / f(n - 1)) / f(M)
        g = blocked_sum(mean) / f(M)
        e = mean - g
        Bn = blocked_sum(e * e) / f(M - 1)
        varplus = (f(n - 1) / f(n)) * W + Bn
        out = dict(post_mean=g, W=W, Bn=Bn, varplus=varplus, sd=np.sqrt(varplus), rhat=np.sqrt(varplus / W))
        if partials is not None:
            A = seq_sum(partials) / f(M)                      # [K + 1, D]
            ess, mcse, trunc = np.empty(D), np.empty(D), np.empty(D, dtype=np.uint8)
            for i in range(D):
                ess[i], mcse[i], trunc[i] = tail(W[i], varplus[i], A[:, i], n, M)
            out.update(A=A, ess=ess, mcse=mcse, truncated=trunc)
    return out


def diagnose(x, split=2, max_lag=None):
    """Everything at once, as ``binf_amd.diagnostics.summary`` computes it."""
    mo = moments(x, split)
    K = default_max_lag(mo['n']) if max_lag is None else max_lag
    a = autocov_chains(x, split, mo['mean'], K)
    out = summary(mo['mean'], mo['m2'], autocov_partials(a), mo['n'])
    out.update(n=mo['n'], M=mo['M'], K=K, chain_mean=mo['mean'], chain_m2=mo['m2'], a=a)
    return out


# ---------------------------------------------------------------------------
# Inputs of the known-answer tests: AR(1) chains x_t = phi x_{t-1} + sqrt(1 - phi^2) e_t
# (unit stationary variance), 200 warm-up draws discarded.
# ---------------------------------------------------------------------------
AR_SEED = 5
AR_WARMUP = 200


def ar1(phi, T, C, D, seed=AR_SEED, shift=None):
    rs = np.random.RandomState(seed)
    e = rs.standard_normal((T + AR_WARMUP, C, D))
    x = np.empty_like(e)
    x[0] = e[0]
    s = np.sqrt(1.0 - phi * phi)
    for t in range(1, T + AR_WARMUP):
        x[t] = phi * x[t - 1] + s * e[t]
    x = x[AR_WARMUP:]
    if shift is not None:
        x = x + shift
    return np.ascontiguousarray(x)
