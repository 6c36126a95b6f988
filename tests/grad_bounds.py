"""Derived error bounds for the likelihood force of the polynomial and linear kinds
(``binf_poly_gauss_grad_f64``: ``G = A . ((theta . A - y) tau)``, csrc/poly.hip) and for
the chain-rule contraction (``binf_jacobian_contract_f64``, csrc/jacobian.hip), the exact
values they are measured from, and the integer data on which the kernels must return
exact bits.  Nothing here is a measured tolerance.  Host only.

The operation, for one chain with coefficients ``theta`` [K], design matrix ``A`` [K x N],
data ``y`` [N] and precision ``tau``:

    m_n = sum_k theta_k A_kn      d_n = m_n - y_n      r_n = d_n tau      G_i = sum_n A_in r_n

With ``u = 2**-53``, ``gamma_m = m u / (1 - m u)`` (linear_bounds.gamma) and
``S_n = sum_k |theta_k| |A_kn|``:

mock      ``|m^_n - m_n| <= delta_n = gamma_K S_n``: K products and K - 1 additions, each
          rounded at most once, in ANY order, fused or not (Higham, Accuracy and Stability
          of Numerical Algorithms, 2nd ed., (3.5)).  The MFMA k-steps and the FMAs of the
          VALU tail are such products and additions; the zero the accumulator starts from
          adds exactly.
residual  ``d^_n = (m^_n - y_n)(1 + e1)`` and ``r^_n = d^_n tau (1 + e2)`` with
          ``|e1|, |e2| <= u``: one rounding of the subtraction, one of the product by tau.
          So ``|d^_n - d_n| <= delta_n + u (|d_n| + delta_n) =: a_n``,
          ``|d^_n| <= (|d_n| + delta_n)(1 + u)`` and
          ``|r^_n - r_n| <= |tau| a_n + u |tau| |d^_n|
                         <= |tau| a_n (1 + u) + u |tau| (|d_n| + delta_n)(1 + u) =: rho_n``
          (the factor ``1 + u`` on the first term is not needed; it only rounds up).
force     the computed force is an N-term dot product of the computed residuals in SOME
          tree: ``G^_i = sum_n A_in r^_n (1 + t_n)`` with ``|t_n| <= gamma_N`` (N products,
          N - 1 additions).  The tiles of a split, the joins of the splits
          (split_reduce_kernel) and the xor-16 / xor-32 lane joins of the VALU rows are
          additions of that tree; zero-initialised accumulators, the zero residuals of
          data points beyond N and the zeros of empty splits add exactly.  Hence

              |G^_i - G_i| <= sum_n |A_in| rho_n + gamma_N sum_n |A_in| (|r_n| + rho_n).

No term of this is scaled or fitted.  It assumes that nothing overflows or underflows
(the generators below stay far from both).

contraction  ``out_k = sum_n J_kn r_n`` is an N-term dot product of the given doubles:
          ``|out^_k - out_k| <= gamma_N sum_n |J_kn| |r_n|`` (:func:`contract_bound`), for the
          MFMA form and for the per-chain FMA form alike.

The exact values come from integer arithmetic on the doubles (linear_bounds.to_ints,
object-array dot products): every double is an integer over a power of two, so ``m``,
``d``, ``r`` and ``G`` are exact integers over a common power of two.  The bounds are
evaluated in double precision; linear_bounds.SLACK covers the roundings of that.

For the chains that are not compared with exact arithmetic the bound is evaluated on
numpy's float64 residual (:func:`force_float`): numpy's own mock data and residual obey the
model above, so ``|d_n| (1 - u) <= |d~_n| + delta_n (1 + u)``; ``rho_n`` grows with ``|d_n|``,
so the bound evaluated at that upper limit of ``|d_n|`` is not below the exact one.  numpy's
force lies inside it as the device's does: the assertion on a device value is
``|got - numpy| <= 2 bound``.

Integer data (:func:`integer_case`, :func:`leapfrog_case`): when ``sum |terms|`` of every
sum, counted in units of the finest granularity ``2**-g`` of its terms, stays below
``2**53``, every product and every partial sum in any order is a double, nothing is
rounded, and a kernel returns the exact value bit for bit.  :func:`integer_case_width` and
the width returned by :func:`leapfrog_ints` are those counts' bit lengths."""
from fractions import Fraction

import numpy as np

import linear_bounds as LB

U = LB.U
SLACK = LB.SLACK
gamma = LB.gamma
OLD_BAR = 1e-10              # the allowance of test_mfma_gradient_matches_numpy_chain_rule


def _rho(abs_tau, abs_d, delta):
    """rho_n of the module docstring."""
    a = delta + U * (abs_d + delta)
    return abs_tau * a * (1.0 + U) + U * abs_tau * (abs_d + delta) * (1.0 + U)


# ---------------------------------------------------------------------------
# exact arithmetic on doubles
# ---------------------------------------------------------------------------
class ExactForce(object):
    """Exact forces of chains against one data set, and their bounds."""

    def __init__(self, A, ys):
        self.ex = LB.Exact(A, ys)
        self.K, self.N = self.ex.K, self.ex.N

    def parts(self, theta, tau):
        """``(D, sd, G, sg)``: residuals before the precision ``D[n] / 2**sd`` and the force
        ``G[i] / 2**sg`` of one chain, as Python ints."""
        ex = self.ex
        _, _, D, sd = ex.residual(theta)
        mt, st = LB.to_ints(tau)
        R = D * int(mt)
        G = np.asarray(np.dot(ex.mA, R), dtype=object).reshape(self.K)
        return D, sd, G, sd + st + ex.sA

    def force(self, theta, tau):
        """``(G, s)`` with ``G_i = G[i] / 2**s`` exactly."""
        _, _, G, sg = self.parts(theta, tau)
        return G, sg

    def chain(self, theta, tau):
        """dict(G=(ints, shift), bound=[K], S, delta, d=|d_n|, rho, scale=sum|A||r|) of one chain."""
        ex = self.ex
        theta = np.asarray(theta, dtype=np.float64)
        t = abs(float(tau))
        D, sd, G, sg = self.parts(theta, tau)
        S = np.abs(theta).dot(ex.absA) * SLACK
        delta = gamma(self.K) * S * SLACK
        d = LB.abs_floats(D, sd)
        rho = _rho(t, d, delta)
        scale = ex.absA.dot(d * t)
        bound = (ex.absA.dot(rho) + gamma(self.N) * ex.absA.dot(d * t + rho)) * SLACK
        return dict(G=(G, sg), bound=bound, S=S, delta=delta, d=d, rho=rho, scale=scale)

    def error(self, exact, got):
        """``|got_i - G_i|`` as floats, ``exact`` being ``(G, s)``."""
        G, s = exact
        H, sh = LB.to_ints(got)
        top = max(s, sh)
        diff = H * (1 << (top - sh)) - G * (1 << (top - s))
        return LB.abs_floats(diff, top)


def exact_to_float(exact):
    """The exact force rounded to doubles (for printing and for injected errors)."""
    G, s = exact
    return np.array([float(Fraction(int(v), 1 << s)) for v in G], dtype=np.float64)


# ---------------------------------------------------------------------------
# the same bound on numpy's float64 values, for every chain of a batch
# ---------------------------------------------------------------------------
def force_float(theta, A, ys, tau):
    """``(numpy force [C x K], bound [C x K])`` with ``tau`` a scalar or ``[C]``."""
    theta = np.asarray(theta, dtype=np.float64)
    C = theta.shape[0]
    N = A.shape[1]
    absA = np.abs(A)
    t = np.broadcast_to(np.asarray(tau, dtype=np.float64), (C,))[:, None]
    d = theta.dot(A) - ys
    force = (d * t).dot(A.T)
    delta = LB.mock_bound_float(theta, A)
    dup = (np.abs(d) + delta * (1.0 + U)) / (1.0 - U)
    rho = _rho(np.abs(t), dup, delta)
    bound = (rho.dot(absA.T) + gamma(N) * (np.abs(t) * dup + rho).dot(absA.T)) * SLACK * SLACK
    return force, bound


def old_bar(theta, A, ys, tau):
    """``1e-10 sum_n |A_in| |r_n|`` [C x K], as the parent's test evaluates it."""
    theta = np.asarray(theta, dtype=np.float64)
    t = np.broadcast_to(np.asarray(tau, dtype=np.float64), (theta.shape[0],))[:, None]
    return OLD_BAR * np.abs((theta.dot(A) - ys) * t).dot(np.abs(A).T)


# ---------------------------------------------------------------------------
# the chain-rule contraction
# ---------------------------------------------------------------------------
def contract_bound(J, r):
    """``gamma_N sum_n |J_kn| |r_n|``: ``J`` [K x N] or [C x K x N], ``r`` [N] or [C x N]."""
    J, r = np.abs(np.asarray(J, dtype=np.float64)), np.abs(np.asarray(r, dtype=np.float64))
    N = J.shape[-1]
    if J.ndim == 3:
        s = np.einsum('ckn,cn->ck', J, r.reshape(J.shape[0], N))
    else:
        s = r.dot(J.T)
    return gamma(N) * s * SLACK


def contract_error(J, r, got):
    """``|got_k - sum_n J_kn r_n|`` of one chain (``J`` [K x N], ``r`` [N]) as floats."""
    mJ, sJ = LB.to_ints(J)
    mr, sr = LB.to_ints(r)
    want = np.asarray(np.dot(mJ, mr), dtype=object).reshape(J.shape[0])
    H, sh = LB.to_ints(got)
    top = max(sJ + sr, sh)
    return LB.abs_floats(H * (1 << (top - sh)) - want * (1 << (top - sJ - sr)), top)


# ---------------------------------------------------------------------------
# designs
# ---------------------------------------------------------------------------
DESIGNS = ('normal', 'scaled', 'poly', 'zeros')


def design(kind, K, N, rs):
    """The four design matrices of the GPU tests: dense standard normal; the same with rows
    scaled by 2**randint(-30, 31); the polynomial on [-1, 1]; one with exact zeros (a third
    of the entries, one whole row, one whole column).  A fifth, 'positive' (|standard normal|,
    no zero), is for the non-finite test alone: one infinite coefficient then makes EVERY
    component of its chain's force infinite, of one sign."""
    if kind == 'normal':
        return rs.standard_normal((K, N))
    if kind == 'scaled':
        return rs.standard_normal((K, N)) * 2.0 ** rs.randint(-30, 31, size=(K, 1))
    if kind == 'poly':
        xs = np.linspace(-1.0, 1.0, N) if N > 1 else np.array([0.75])
        return np.vstack([xs ** i for i in range(K)])
    if kind == 'positive':
        return np.abs(rs.standard_normal((K, N))) + 2.0 ** -10
    if kind == 'zeros':
        A = rs.standard_normal((K, N))
        A[rs.uniform(size=(K, N)) < 1.0 / 3.0] = 0.0
        A[K // 2, :] = 0.0
        A[:, N // 3] = 0.0
        return A
    raise ValueError(kind)


def float_case(kind, K, N, C, seed):
    """``(A, ys, theta, tau [C])``: data near a truth, chains around it."""
    rs = np.random.RandomState(seed)
    A = design(kind, K, N, rs)
    scale = 1.0 / np.maximum(np.max(np.abs(A), axis=1), 2.0 ** -40)    # coefficients of size 1 / row
    truth = rs.standard_normal(K) * scale
    mock = truth.dot(A)
    ys = mock + 0.1 * (np.std(mock) + 1.0) * rs.standard_normal(N)
    theta = truth + 0.2 * rs.standard_normal((C, K)) * scale
    tau = rs.uniform(0.5, 4.0, size=C)
    return A, ys, theta, tau


# ---------------------------------------------------------------------------
# integer data: exact in every order
# ---------------------------------------------------------------------------
INT_A, INT_A_OFF, INT_THETA, INT_THETA_OFF, INT_Y = 4, 2, 3, 6, 9
INT_TAUS = (0.25, 0.5, 1.0, 2.0, 4.0)


def integer_case(K, N, C, seed):
    """``(A, ys, theta, tau [C])`` of small integers and power-of-two precisions.  The offsets
    make the operands asymmetric: they vary along k AND n (3 k + 7 n) and per chain, so a
    transposed or shifted operand map cannot cancel."""
    rs = np.random.RandomState(seed)
    k, n = np.arange(K)[:, None], np.arange(N)[None, :]
    A = rs.randint(-INT_A, INT_A + 1, size=(K, N)) + (3 * k + 7 * n) % (2 * INT_A_OFF + 1) - INT_A_OFF
    theta = rs.randint(-INT_THETA, INT_THETA + 1, size=(C, K)) + (np.arange(C) % (INT_THETA_OFF + 1))[:, None]
    ys = rs.randint(-INT_Y, INT_Y + 1, size=N)
    tau = np.array(INT_TAUS)[rs.randint(0, len(INT_TAUS), size=C)]
    return A.astype(np.float64), ys.astype(np.float64), theta.astype(np.float64), tau


def integer_force(A, ys, theta, tau):
    """The force of integer data in int64 arithmetic (precisions in quarters), as doubles."""
    Ai, yi, ti = A.astype(np.int64), ys.astype(np.int64), theta.astype(np.int64)
    t4 = np.broadcast_to(np.asarray(tau, dtype=np.float64) * 4.0, (theta.shape[0],))
    assert np.array_equal(Ai, A) and np.array_equal(yi, ys) and np.array_equal(ti, theta)
    assert np.array_equal(t4, np.round(t4))
    g4 = ((ti.dot(Ai) - yi) * t4.astype(np.int64)[:, None]).dot(Ai.T)
    return g4.astype(np.float64) / 4.0


def integer_case_width(K, N):
    """Bit length of the largest ``sum |terms|`` an :func:`integer_case` of this shape can
    reach, in units of its granularity (2**-2: the precisions), from Python ints."""
    a, th = INT_A + INT_A_OFF, INT_THETA + INT_THETA_OFF
    mock = K * a * th
    resid4 = (mock + INT_Y) * int(max(INT_TAUS) * 4)       # |d| max tau, in quarters
    return (N * a * resid4).bit_length()


# ---------------------------------------------------------------------------
# the fused leapfrog on integer data
# ---------------------------------------------------------------------------
LEAPFROG_CASES = [(5, 48, 2, 4), (33, 64, 2, 6), (17, 35, 3, 5)]      # K, N, L, dt = 2**-k


def leapfrog_case(K, N, C, seed):
    """``(A, ys, q, p, tau_exp [C])`` integers; the precision of chain c is 2**tau_exp[c]."""
    rs = np.random.RandomState(seed)
    k, n = np.arange(K)[:, None], np.arange(N)[None, :]
    A = rs.randint(-1, 2, size=(K, N)) + (3 * k + 7 * n) % 2
    q = rs.randint(-2, 3, size=(C, K)) + (np.arange(C) % 3)[:, None]
    p = rs.randint(-3, 4, size=(C, K)) - (np.arange(C) % 2)[:, None]
    ys = rs.randint(-9, 10, size=N)
    tau_exp = rs.randint(-1, 1, size=C)
    return A.astype(np.int64), ys.astype(np.int64), q.astype(np.int64), p.astype(np.int64), tau_exp


def _shift(x, e):
    """``x * 2**e`` on int64 rows (``e`` [C], either sign); a negative shift must be exact."""
    e = np.asarray(e, dtype=np.int64).reshape((-1,) + (1,) * (x.ndim - 1))
    up, down = np.maximum(e, 0), np.maximum(-e, 0)
    assert not np.any(x & ((np.int64(1) << down) - 1)), 'granularity finer than the common scale'
    return (x >> down) << up


def leapfrog_ints(A, ys, q, p, tau_exp, dt_exp, L):
    """hmc.py's leapfrog (half kick, L - 1 x [drift, kick], drift, half kick) under the force
    above in int64 arithmetic on a common scale 2**-g: ``(q, p, width)`` with q and p as
    doubles and ``width`` the bit length of the largest ``sum |terms|`` of any sum, in units
    of 2**-g (not finer than any term).  ``tau_exp`` and ``dt_exp`` are [C]: precision
    2**tau_exp, step 2**-dt_exp."""
    C = q.shape[0]
    tau_exp = np.broadcast_to(np.asarray(tau_exp, dtype=np.int64), (C,))
    dt_exp = np.broadcast_to(np.asarray(dt_exp, dtype=np.int64), (C,))
    # granularity after every stage, per chain: the precision costs -tau_exp bits (if negative),
    # a half kick dt_exp + 1, a kick dt_exp, a drift dt_exp
    g = int(np.max(np.maximum(-tau_exp, 0) * (L + 1) + dt_exp * (2 * L + 1) + 2))
    assert g < 62
    absA = np.abs(A)
    Q, P, Y = q << g, p << g, ys << g
    worst = 0

    def force(Q):
        nonlocal worst
        D = Q.dot(A) - Y
        R = _shift(D, tau_exp)
        worst = max(worst, int(np.max(np.abs(Q).dot(absA) + np.abs(Y))),
                    int(np.max(np.abs(R).dot(absA.T))))
        return R.dot(A.T)

    for l in range(L + 1):
        step = dt_exp + 1 if l in (0, L) else dt_exp
        kick = _shift(force(Q), -step)
        worst = max(worst, int(np.max(np.abs(P) + np.abs(kick))))
        P = P - kick
        if l < L:
            drift = _shift(P, -dt_exp)
            worst = max(worst, int(np.max(np.abs(Q) + np.abs(drift))))
            Q = Q + drift
    width = worst.bit_length()
    assert width < 63
    return Q.astype(np.float64) / 2.0 ** g, P.astype(np.float64) / 2.0 ** g, width


def leapfrog_fraction(A, ys, q, p, tau, dt, L):
    """The same leapfrog of ONE chain in ``fractions.Fraction``: ``(q, p)`` lists."""
    K, N = A.shape
    A = [[Fraction(int(v)) for v in row] for row in A]
    q, p = [Fraction(int(v)) for v in q], [Fraction(int(v)) for v in p]
    tau, dt = Fraction(tau), Fraction(dt)
    for l in range(L + 1):
        r = [(sum(q[k] * A[k][n] for k in range(K)) - int(ys[n])) * tau for n in range(N)]
        step = dt / 2 if l in (0, L) else dt
        p = [p[i] - step * sum(A[i][n] * r[n] for n in range(N)) for i in range(K)]
        if l < L:
            q = [q[i] + p[i] * dt for i in range(K)]
    return q, p


# ---------------------------------------------------------------------------
# self-test: a bound that cannot fail shows nothing
# ---------------------------------------------------------------------------
def _pairwise(v):
    return v[0] if len(v) == 1 else _pairwise(v[:len(v) // 2]) + _pairwise(v[len(v) // 2:])


def _numpy_forces(A, r):
    """numpy's force from given residuals in three orders: BLAS, sequential, pairwise."""
    terms = A * r[None, :]
    return [A.dot(r), np.cumsum(terms, axis=1)[:, -1], np.array([_pairwise(row) for row in terms])]


def self_test(seed=0, shapes=((5, 48), (33, 1040), (33, 16384))):
    """numpy's force in three summation orders lies inside the bound; three injected errors
    that pass the old ``1e-10 sum|A||r|`` bar lie outside it; the old bar is at least 50 bounds
    wide.  Returns the figures, one dict per shape."""
    out = []
    for K, N in shapes:
        rs = np.random.RandomState(seed + K + N)
        xs = np.linspace(-1.0, 1.0, N)
        A = np.vstack([xs ** i for i in range(K)])
        truth = rs.standard_normal(K)
        tau = 2.5
        ys = truth.dot(A) + rs.standard_normal(N) / np.sqrt(tau)
        theta = truth + 0.3 * rs.standard_normal(K)
        ef = ExactForce(A, ys)
        c = ef.chain(theta, tau)
        bound, bar = c['bound'], OLD_BAR * c['scale']
        fig = dict(K=K, N=N, bar_over_bound=float(np.min(bar / bound)))
        assert N > 16384 or fig['bar_over_bound'] >= 50.0, fig

        # numpy in three orders, and the float-evaluated bound
        mock = theta.dot(A)
        r = (mock - ys) * tau
        worst = 0.0
        for g in _numpy_forces(A, r):
            err = ef.error(c['G'], g)
            assert np.all(err <= bound), (K, N, float(np.max(err / bound)))
            worst = max(worst, float(np.max(err / bound)))
        fig['numpy'] = worst
        gf, bf = force_float(theta[None, :], A, ys, tau)
        assert np.all(bf[0] >= bound) and np.all(bf[0] <= 1.01 * bound + 1e-300)
        assert np.all(ef.error(c['G'], gf[0]) <= bf[0])

        def verdict(bad, seen=True):
            """injected: inside the old bar against numpy, outside the new bound"""
            old = np.abs(bad - A.dot(r)) <= bar
            new = ef.error(c['G'], bad) / bound
            assert np.all(old), 'the injected error does not pass the old bar'
            assert np.max(new) > 1.0 or not seen, 'the bound does not see the injected error'
            return float(np.max(new))

        # 1. one mock datum moved by 1e-11 of its S_n (ONE datum among 16384 is below
        #    gamma_16384 of the whole sum: reported there, asserted up to 2048 points)
        n = int(np.argmax(c['S'] * np.max(np.abs(A) / bound[:, None], axis=0)))
        bad = mock.copy()
        bad[n] += 1e-11 * c['S'][n]
        fig['mock_moved'] = verdict(A.dot((bad - ys) * tau), seen=N <= 2048)

        # 2. one product A_in r_n dropped, its size between the bound and the old bar (the high
        #    rows of the polynomial design are ~ 0 almost everywhere: they supply such products)
        prod = np.abs(A * r[None, :])
        ok = (prod > 4.0 * bound[:, None]) & (prod < 0.25 * bar[:, None])
        #    -- from degree 32 on; the 48 points of a degree-4 row are all of comparable size
        assert ok.any() or K < 33, 'no product between the bound and the old bar'
        fig['product_dropped'] = fig['product_dropped_row'] = None
        if ok.any():
            i = int(np.max(np.nonzero(ok.any(axis=1))[0]))
            n = int(np.argmax(np.where(ok[i], prod[i], 0.0)))
            bad = A.dot(r)
            bad[i] -= A[i, n] * r[n]
            fig['product_dropped'] = verdict(bad)
            fig['product_dropped_row'] = i

        # 3. the precision rounded to float32, at a theta near the least-squares one, where
        #    |G| / sum|A||r| is small but above the bound
        tau3 = 3.7
        t32 = float(np.float32(tau3))
        # (the truncated fit: the full one of a degree-32 monomial basis has coefficients of
        # 1e6 and more, whose S_n -- and with it the bound -- is as large)
        best = np.linalg.lstsq(A.T, ys, rcond=1e-4)[0]
        seen = None
        for e in range(-1, -9, -1):
            th3 = best + 10.0 ** e * rs.standard_normal(K)
            c3 = ef.chain(th3, tau3)
            r3 = th3.dot(A) - ys
            good, bad = A.dot(r3 * tau3), A.dot(r3 * t32)
            err3 = ef.error(c3['G'], bad) / c3['bound']
            if np.all(np.abs(bad - good) <= OLD_BAR * c3['scale']) and np.max(err3) > 1.0:
                assert np.all(ef.error(c3['G'], good) <= c3['bound'])
                seen = float(np.max(err3))
                fig['tau_float32_at'] = float(np.max(np.abs(good) / c3['scale']))
                break
        assert seen is not None, 'no theta at which a float32 precision passes the old bar only'
        fig['tau_float32'] = seen
        out.append(fig)
    return out


# ---------------------------------------------------------------------------
# the shapes of the GPU tests (csrc/poly.hip: grad_dispatch, grad_ct, grad_splits,
# grad_whole_tiles), shared with the CPU test of the integer generators' widths
# ---------------------------------------------------------------------------
K_LIST = (1, 4, 5, 8, 9, 16, 17, 18, 19, 32, 33, 34, 35, 36, 37, 48, 49, 50, 51, 64)
N_GENERAL = (1, 15, 17, 31, 35, 1027)
N_TRIMMED = (16, 32, 48, 1024, 1040, 3072)
C_LIST = (1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4100, 4113)
K_CORE = (5, 33, 64)


def force_cases():
    """``(K, N, C)``: every K with one general and one trimmed N at a small ragged C; every N
    and every C with K in (5, 33, 64), each C under both kernels; N = 272 (17 tiles) at
    C >= 4096 (16 splits, two chain tiles per wave)."""
    cases = []
    for K in K_LIST:
        cases += [(K, 35, 19), (K, 48, 19)]
    for K in K_CORE:
        cases += [(K, N, 17) for N in N_GENERAL + N_TRIMMED]
        cases += [(K, 272, 4100)]
        for C in C_LIST:
            cases += [(K, 17, C), (K, 32, C)]
    seen, out = set(), []
    for c in cases:
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


def sample_chains(C, seed):
    """The chains compared with exact arithmetic: both sides of the 16-chain tile, the
    workgroup and the two-tiles-per-wave edges, the last chain, and four drawn at random."""
    chains = set(c for c in (0, 15, 16, 63, 64, 4095, 4096, C - 1) if 0 <= c < C)
    chains.update(int(c) for c in np.random.RandomState(seed).randint(0, C, size=4))
    c = 0
    while len(chains) < min(C, 4):
        chains.add(c)
        c += 1
    return sorted(chains)
