"""Derived error bounds for the negative-binomial kernels (``binf_negbin_count_term_f64``,
``binf_negbin_pointwise_f64``, ``binf_linear_negbin_logp_f64`` / ``_grad_f64``; csrc/glm_term.hpp,
csrc/glm.hip, csrc/negbin.hip) and the exact values they are measured from.  Nothing here is a
measured tolerance.  Host only.  Notation and machinery are those of ``glm_bounds`` (imported).

inputs
    ``lam`` (a double) is GIVEN: the exact value is that of ``phi = exp(lam)`` at 50 digits.  The
    kernels' own ``phi^ = exp(lam)`` is a transcendental like the others: ``|phi^ - phi| <= 8u phi``
    (no TINY: inside the regular range phi is a normal double).  It is held on its own for the
    host library in the CPU tests, and enters every bound below through ``dphi = 8u phi``.

term (``z = eta - lam``, ``m = y + phi``, then the binomial lines)
    ``z^ = fl(eta^ - lam)``: ``|z^ - z| <= dz = delta + u (|eta| + delta + |lam|)``.
    ``m^ = fl(y + phi^)``:   ``|m^ - m| <= dm = dphi + u (y + phi + dphi)``.
    The exact term is Lipschitz in z with ``max(y, m - y) = max(y, phi)`` -- the binomial bound of
    ``glm_bounds.term_bounds`` at ``(z, dz, y, m)`` -- and in m with ``sp(z)`` (``s(z) <= 1`` for g):
        ``B_n = B_binomial(z, dz, y, m) + dm sp+``,   ``rho_n = rho_binomial(z, dz, y, m) + dm``.
    The binomial formulas are evaluated at the exact m where the kernel has m^: a relative
    ``dm / m <= 10u`` on terms that are themselves O(u); one more SLACK covers it.

count term
    ``x^ = fl(phi^ + j)``: relative ``(dphi + u (phi + j)) / (phi + j) <= 9u`` (+ second order),
    so ``|log x^ - log x| <= 9.01u``; the device's log: ``8u |L| + TINY``; the product by the exact
    integer T_j: ``u T_j |L|``:   ``b_j = T_j (9.01u + 9u |L_j| + TINY)``,  L_j = log(phi + j).
    ymax computed terms in ANY order and ``+ log_norm``: ``glm_bounds.logp_bound(b, T |L|,
    log_norm, ymax)``.  The prefix at v: the same with T = 1, v terms and no constant.

record   ``(ll^ + P^) + lconst``: ``B_n + bP + u (mag + |P| + B_n + bP) (2 + u) + u |lconst|``.
log-prob ``glm_bounds.logp_bound(B, mag, lnc, N)`` for the N terms and the rounding of ``+ lnc``,
    plus the count term's own bound (lnc is the device's, computed from the same lam).
force    ``glm_bounds.force_bound(A, rho, gabs)``, ``gabs = max(m, y) = y + phi``.

Chains that are not compared with exact arithmetic are held to numpy's restatement within twice
the float form (delta doubled), as in ``glm_bounds.float_case``.
"""
import numpy as np

import glm_bounds as GBm
import glm_ref as R
import negbin_ref as NR

U = GBm.U
SLACK = GBm.SLACK
TINY = GBm.TINY
gamma = GBm.gamma
err = GBm.err


def phi_bound(phi):
    """``dphi``: what the kernel's exp(lam) may be off by."""
    return 8 * U * np.asarray(phi, dtype=np.float64) * SLACK


def term_bounds(eta, delta, y, lam):
    """``(B, rho, mag, gabs)`` elementwise; ``eta`` [.. x N] with ``lam`` broadcastable."""
    eta = np.asarray(eta, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    lam = NR.clamp(lam)
    phi = np.exp(lam)
    z = eta - lam
    dz = (delta + U * (np.abs(eta) + delta + np.abs(lam))) * SLACK
    dphi = phi_bound(phi)
    dm = (dphi + U * (y + phi + dphi)) * SLACK
    m = y + phi
    B, rho, mag, gabs = GBm.term_bounds(R.BINOMIAL_LOGIT, z, dz, y, m * np.ones_like(z))
    sp = GBm._mags(R.BINOMIAL_LOGIT, z, dz, y, m)['sp']
    return (B + dm * sp) * SLACK, (rho + dm) * SLACK, mag * SLACK, gabs * SLACK


def count_bounds(lam, tail):
    """``(b_j, mag_j)`` [ymax] of one chain's count term."""
    phi = float(NR.phi_of(lam))
    T = np.asarray(tail, dtype=np.float64)
    j = np.arange(T.shape[0], dtype=np.float64)
    L = np.abs(np.log(phi + j)) if T.shape[0] else np.zeros(0)
    return T * (9.01 * U + 9 * U * L + TINY) * SLACK, T * L * SLACK


def count_bound(lam, tail, log_norm):
    b, mag = count_bounds(lam, tail)
    return float(GBm.logp_bound(b, mag, log_norm, len(tail)))


def prefix_bound(lam, v):
    """``(bound, |P| upper limit)`` of the prefix at the value ``v``."""
    b, mag = count_bounds(lam, np.ones(int(v)))
    return float(GBm.logp_bound(b, mag, 0.0, int(v))), float(np.sum(mag + b))


def prefix_bounds(lam, values):
    """:func:`prefix_bound` for every chain of ``lam`` [C] and every value: ``(bound, |P| limit)``,
    both [C x J], by cumulative sums of the per-term allowances."""
    lam = np.atleast_1d(np.asarray(lam, dtype=np.float64))
    v = np.asarray(values).astype(np.int64)
    vmax = int(v.max()) if v.size else 0
    phi = NR.phi_of(lam)[:, None]
    L = np.abs(np.log(phi + np.arange(vmax, dtype=np.float64)[None, :]))
    b = (9.01 * U + 9 * U * L + TINY) * SLACK
    zero = np.zeros((lam.shape[0], 1))
    cb = np.concatenate([zero, np.cumsum(b, axis=1)], axis=1)[:, v]
    cm = np.concatenate([zero, np.cumsum(L * SLACK + b, axis=1)], axis=1)[:, v]
    g = np.array([gamma(int(x) + 1) + U for x in v])[None, :]
    return (cb + g * cm) * SLACK * SLACK, cm * SLACK


def record_bound(B, mag, bP, absP, lconst):
    lc = 0.0 if lconst is None else np.abs(lconst)
    return (B + bP + 2.5 * U * (mag + absP + B + bP) + U * lc) * SLACK


class ExactNB(object):
    """Exact log-probs and forces of chains against one data set."""

    def __init__(self, A, ys, offset=None):
        self.glm = GBm.ExactGLM(R.BINOMIAL_LOGIT, A, ys, None, offset)
        self.A = self.glm.A
        self.K, self.N = self.A.shape
        self.ys = self.glm.ys
        self.tail = NR.tail_counts(self.ys)

    def chain(self, theta, lam, log_norm=0.0, want_force=True):
        """dict(eta, delta, ll=[mpf], lp=mpf (count term and log_norm included), lp_bound,
        count=mpf, count_bound, force=[mpf], force_bound, B, rho, mag)."""
        M = R.mp()
        lam = float(lam)
        eta, etaf, delta = self.glm.eta(theta)
        ll = [NR.exact_ll(e, y, lam) for e, y in zip(eta, self.ys)]
        B, rho, mag, gabs = term_bounds(etaf, delta, self.ys, lam)
        count = NR.exact_count(lam, self.tail)
        cb = count_bound(lam, self.tail, log_norm)
        lnc = float(abs(count)) + abs(log_norm) + cb
        out = dict(eta=etaf, delta=delta, ll=ll, B=B, rho=rho, mag=mag, count=count, count_bound=cb,
                   lp=M.fsum(ll) + count + M.mpf(float(log_norm)),
                   lp_bound=float(GBm.logp_bound(B, mag, lnc, self.N)) + cb)
        if want_force:
            g = [NR.exact_g(e, y, lam) for e, y in zip(eta, self.ys)]
            gi = np.array([int(M.floor(v * M.mpf(2) ** 240 + M.mpf(0.5))) for v in g], dtype=object)
            Gi = np.asarray(np.dot(self.glm.ex.mA, gi), dtype=object).reshape(self.K)
            out['g'] = g
            out['force'] = [M.mpf(int(v)) / M.mpf(2) ** (240 + self.glm.ex.sA) for v in Gi]
            out['force_bound'] = GBm.force_bound(self.A, rho, gabs)
        return out


def float_case(theta, A, ys, offset, lam, log_norm=0.0):
    """numpy's values and the float form of the bounds for every chain of ``theta`` [C x K]
    under ``lam`` [C]: dict(eta, ll, g, lp, lp_bound, lnc, force, force_bound, B, rho, mag)."""
    theta = np.atleast_2d(theta)
    lam = np.asarray(lam, dtype=np.float64)
    K, N = A.shape
    mock = theta.dot(A)
    off = 0.0 if offset is None else offset
    eta = mock + off
    S = np.abs(theta).dot(np.abs(A)) * SLACK
    delta = 2.0 * GBm.eta_delta(S, np.abs(mock) + gamma(K) * S, np.abs(off), K)
    ll, g = NR.term(eta, ys, lam)
    B, rho, mag, gabs = term_bounds(eta, delta, ys, lam[:, None])
    tail = NR.tail_counts(ys)
    lnc = NR.count_term(lam, tail, log_norm)
    cb = np.array([count_bound(l, tail, log_norm) for l in lam])
    lp = R.sum_in_kernel_order(ll, 0.0) + lnc
    return dict(eta=eta, delta=delta, ll=ll, g=g, B=B, rho=rho, mag=mag, lnc=lnc, lp=lp,
                lp_bound=GBm.logp_bound(B, mag, 0.0, N) + U * np.abs(lnc) * SLACK + 2 * cb,
                force=g.dot(A.T), force_bound=GBm.force_bound(A, rho, gabs))


def case(K, N, C, seed, offset=True, ymax=300):
    """``(A, ys, offset, theta, lam)``: ``glm_bounds.case``'s design and coefficients (eta across
    +-40), counts that include 0 and a maximum of ``ymax``, lam spread over [-20, 20] across the
    chains (both ends included where C > 1)."""
    A, ys, _, off, theta = GBm.case(R.POISSON_LOG, K, N, C, seed, trials=False, offset=offset)
    rs = np.random.RandomState(seed + 7)
    ys = np.floor(rs.gamma(0.7, 12.0, size=N)).clip(0.0, float(ymax))
    ys[rs.randint(N)] = 0.0
    if N > 1:
        ys[(int(np.argmin(ys)) + 1) % N] = float(ymax)
    lam = np.linspace(-20.0, 20.0, C) if C > 1 else np.array([0.75])
    lam = lam[rs.permutation(C)]
    return A, ys, off, theta, lam


def self_test(seed=0):
    """numpy's own float64 results lie inside the exact bounds; with the count term dropped, with
    phi dropped from m, and with the gradient's sign flipped they lie outside."""
    out = []
    for K, N in ((5, 17), (33, 100)):
        A, ys, off, theta, lam = case(K, N, 3, seed + K)
        ex = ExactNB(A, ys, off)
        tail = NR.tail_counts(ys)
        for c in range(3):
            e = ex.chain(theta[c], lam[c], -3.5)
            ll, g = NR.term(R.eta_of(theta[c].dot(A), off), ys, lam[c])
            lnc = float(NR.count_term(lam[c], tail, -3.5)[0])
            lp = float(R.sum_in_kernel_order(ll, 0.0)[0]) + lnc
            a = err(lp, e['lp']) / e['lp_bound']
            f = g.dot(A.T)
            b = max(err(x, w) / bd for x, w, bd in zip(f, e['force'], e['force_bound']))
            assert a <= 1.0 and b <= 1.0, (K, N, c, a, b)
            dropped = err(float(R.sum_in_kernel_order(ll, 0.0)[0]) - 3.5, e['lp']) / e['lp_bound']
            l0, _ = R.term(R.BINOMIAL_LOGIT, R.eta_of(theta[c].dot(A), off) - lam[c], ys, ys)
            no_phi = err(float(R.sum_in_kernel_order(l0, 0.0)[0]) + lnc, e['lp']) / e['lp_bound']
            flipped = max(err(-x, w) / bd for x, w, bd in zip(f, e['force'], e['force_bound']))
            assert dropped > 1.0 and no_phi > 1.0 and flipped > 1.0, (K, N, c, dropped, no_phi, flipped)
            out.append(dict(K=K, N=N, lam=float(lam[c]), lp=a, force=b, dropped=dropped, no_phi=no_phi,
                            flipped=flipped))
    return out
