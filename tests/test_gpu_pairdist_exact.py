"""The pair-distance restraint kernels (BASELINE config C5) against exact arithmetic
(tests/pairdist_exact.py: integer sqrt, 50-digit decimal), at the inputs where a
kernel that is only nearly right goes wrong.  Every kernel family is reached
through the C ABI, choosing its form by bead and chain counts and by giving or
withholding the packed targets and the workspace.

1. Distances, chi^2, log-prob, the memo and the one-launch energy on squared
   distances within c 2^-55 ulps of a rounding midpoint, around sqrt_rn's 2^-767
   cut, subnormal, zero, near DBL_MAX and overflowing: distances bitwise the
   correctly rounded root, chi^2 / log-prob bitwise numpy's pairwise sum, the
   energy within a pairwise-sum bound of its 50-digit value.
2. The force of every family per component against the 50-digit force, on rows
   around the 64-bead blocks, the last bead and a bead at equilibrium, held to

       |F - F*| <= tau (EPS_W sum_j |y/d| |dx| + (n + 2) u sum_j |w| |dx|)

   EPS_W bounds the relative error of one pair's y r, r = 1/d from the hardware
   seed r0 = (1 + e0)/d and ONE Newton step r0 (1.5 - 0.5 s r0^2): in exact
   arithmetic r1 = (1 - 1.5 e0^2 - 0.5 e0^3)/d.  The accuracy e0 of v_rsq_f64 is
   not documented; MEASURED on MI355X through the one-sided force kernel (two
   beads at a distance a with 26 significant bits, y = 1.5 2^k, w a read back
   from the force; 102400 squared distances over 2^-600 .. 2^600): the relative
   error of r1 is at most 3.48e-15 = 2^-48.03 (mean -1.7e-16: the -1.5 e0^2 term
   dominates, e0 ~ 2^-24.3; re-measured and printed by
   test_pair_weight_reciprocal_within_the_measured_seed_bound).  With margin e0 <= 2^-24, 1.5 e0^2 <= 1.5 * 2^-48
   (5.3e-15, 1.5x the worst measured).  The roundings of a pair on top (x_i - x_j:
   u, s from three products and two sums: 3u, halved by the root; the three
   operations of the Newton step: 3u; y r in the FMA: u; the difference's
   rounding carried by y/d: u) add 10u: EPS_W = 1.5 * 2^-48 + 10u.  The second
   term is the summation of n - 1 products w dx (each one rounded) and the scaling
   by tau, in any order.
3. Coincident beads: d = 0 makes the model's force NaN for both beads and nothing
   else; every force family, fused leapfrog and the per-step tier give that pattern,
   distances and chi^2 stay finite and bitwise.
4. Fused leapfrogs and HMCSampler.sample() against a 50-digit integration of
   hmc.py:116-123, held to trajectory_bound: first-order error propagation of
   the force bound and the updates' roundings, with a factor 2 allowed for the
   remainder (a margin, not a derived term).
"""
import ctypes
import decimal
import math

import numpy as np
import pytest
import torch

import pairdist_exact as PE
from binf_amd import _native

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
EPS_W = 1.5 * 2.0 ** -48 + 10 * U


def dev_t(a, device, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)


def pp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def host_sq(x, I, J):
    """(a*a + b*b) + e*e per pair, numpy float64 (no FMA), x [n, 3]"""
    a = x[I, 0] - x[J, 0]
    b = x[I, 1] - x[J, 1]
    e = x[I, 2] - x[J, 2]
    return (a * a + b * b) + e * e


def sym_ymat(n, ys):
    I, J = np.triu_indices(n, 1)
    ym = np.zeros((n, n))
    ym[I, J] = ys
    ym[J, I] = ys
    return ym


# ---------------------------------------------------------------------------
# 1. distances, chi^2, log-prob, memo, energy on hard and edge squared distances
# ---------------------------------------------------------------------------
def planted(n, svals, seed):
    """a chain whose pairs (2k, 2k + 1) have the squared distances svals[k] exactly
    (bead 2k at (a, b, z_k), bead 2k + 1 at (0, 0, z_k)); the other beads random"""
    rs = np.random.RandomState(seed)
    x = rs.uniform(-3.0, 3.0, size=(n, 3))
    for k, s in enumerate(svals):
        a, b = PE.realise(s)
        z = 4.0 * k + 1.0
        x[2 * k] = (a, b, z)
        x[2 * k + 1] = (0.0, 0.0, z)
    return x


def energy_bound(d, r, p, E):
    """|E~ - E*| for E = 0.5 sum p^2 + 0.5 sum r^2 (tau = 1): d from an s of exact-input
    roundings (differences u each, three products, two sums: rel 5u; the root halves it
    and rounds: 3.5u, taken as 4u), r = d - y rounded (u |r|), r^2 rounded (u r^2);
    numpy's pairwise sums of P terms err by at most (P / 8192 + log2 P + 32) u times the
    sum of their magnitudes (8-way unrolled leaves of 16, a tree, 8192-element chunks
    added in turn); the halvings are exact and E = 0.5 K - lp rounds once."""
    P = len(d)
    e = 4 * U * d + U * np.abs(r)
    per = (2 * np.abs(r) + e) * e + U * r * r
    hP = P / 8192.0 + math.log2(max(P, 2)) + 32
    hK = len(p) / 8192.0 + math.log2(max(len(p), 2)) + 32
    return 0.5 * (per.sum() + hP * U * np.sum(r * r)) + 0.5 * (hK + 1) * U * np.sum(p * p) + U * abs(E)


class Abi(object):
    def __init__(self, device):
        self.L = _native.lib()
        self.st = _native.stream_handle(device)
        self.device = device

    def ws_chi2(self, C, n, P, give):
        need = self.L.binf_pairdist_chi2_workspace_bytes(C, n, P)
        if not give or need <= 0:
            return None, 0
        return torch.empty(need // 8, dtype=torch.float64, device=self.device), need

    def logp(self, x, I, J, ys, C, n, give):
        P = I.numel()
        out = torch.empty(C, dtype=torch.float64, device=self.device)
        ws, nb = self.ws_chi2(C, n, P, give)
        assert self.L.binf_pairdist_gauss_logp_f64(pp(x), pp(I), pp(J), pp(ys), 1.0, None, pp(out), C, n, P,
                                                   pp(ws), nb, self.st) == 0
        return out

    def logp_memo(self, x, I, J, ys, C, n, give, memo):
        P = I.numel()
        out = torch.empty(C, dtype=torch.float64, device=self.device)
        ws, nb = self.ws_chi2(C, n, P, give)
        mx, ms, sk = memo
        assert self.L.binf_pairdist_gauss_logp_memo_f64(pp(x), pp(I), pp(J), pp(ys), 1.0, None, pp(out), pp(mx),
                                                        pp(ms), pp(sk), C, n, P, pp(ws), nb, self.st) == 0
        return out, sk

    def energy(self, x, p, I, J, ys, C, n, give):
        P = I.numel()
        en = torch.empty(C, dtype=torch.float64, device=self.device)
        lp = torch.empty(C, dtype=torch.float64, device=self.device)
        ws, nb = self.ws_chi2(C, n, P, give)
        kinds = (ctypes.c_int32 * 4)(1, 1, 1, 1)
        assert self.L.binf_pairdist_hmc_energy_f64(pp(x), pp(p), pp(I), pp(J), pp(ys), 1.0, None, 0.0, 0.0, 1,
                                                   kinds, None, 0.0, None, 0.0, pp(en), pp(lp), None, None, None,
                                                   C, n, P, pp(ws), nb, self.st) == 0
        return en, lp


# (n, C, give workspace, what it reaches)
CHI2_PATHS = [(24, 40, True, 'rows kernel, one row per chain'),
              (96, 6, False, 'rows kernel, 16 waves per chain'),
              (65, 1024, False, 'two-row form (C >= 1024, >= 2048 pairs)'),
              (182, 3, True, 'chunks (>= 2 x 8192 pairs, few chains)'),
              (182, 3, False, 'rows kernel with the workspace withheld'),
              (2100, 1, True, 'chunks beyond 2048 beads'),
              (2100, 1, False, 'generic row reduction beyond 2048 beads')]


@pytest.mark.parametrize('n,C,give,what', CHI2_PATHS)
def test_distances_and_chi2_bitwise_on_hard_and_edge_squared_distances(device, n, C, give, what):
    abi = Abi(device)
    P = n * (n - 1) // 2
    if 'chunks' in what:
        assert abi.L.binf_pairdist_chi2_workspace_bytes(C, n, P) > 0, what
    hard = [h.s for h in PE.hard_cases()]
    edges = PE.edge_values()
    per = n // 2 - 1                                   # planted pairs per chain (one bead pair spare)
    rng = np.random.RandomState(n + C)
    # the last chains plant the edge values and an overflowing difference (their chi^2 may be
    # inf), the others the hard cases c, c + H, ...; one chain plants the edges and hard cases
    # (and no overflow: its chi^2 stays finite)
    n_edge = min(C - 1, -(-len(edges) // per)) if C > 1 else 0
    H = C - n_edge
    plant = [hard[c::H][:per] for c in range(H)] + [edges[k * per:(k + 1) * per] for k in range(n_edge)]
    if C == 1:
        plant = [(edges + hard)[:per]]
    xs = np.stack([planted(n, sv, 17 * c + n) for c, sv in enumerate(plant)])
    if n_edge:
        xs[C - 1][n - 1] = (1e200, 0.0, -1e200)        # squared differences overflow: s = inf
    I, J = np.triu_indices(n, 1)
    s = np.stack([host_sq(xs[c], I, J) for c in range(C)])
    d_host = np.sqrt(s)
    if n_edge:
        assert np.isinf(d_host[C - 1]).any()
    # planted pairs: the host's s is the chosen one, its root the correctly rounded one
    pidx = [int(np.flatnonzero((I == 2 * k) & (J == 2 * k + 1))[0]) for k in range(n // 2)]
    planted_s = set()
    for c, sv in enumerate(plant):
        for k, want_s in enumerate(sv):
            assert s[c, pidx[k]] == want_s
            assert PE.cr_sqrt(want_s) == d_host[c, pidx[k]]
            planted_s.add(want_s)
    assert set(edges) <= planted_s or C == 1
    ys_np = np.abs(d_host[0] * (1.0 + 0.01 * rng.standard_normal(P)))
    ys_np[~np.isfinite(ys_np)] = 1.0
    x = dev_t(xs.reshape(C, 3 * n), device)
    I_d, J_d = dev_t(I, device, torch.int32), dev_t(J, device, torch.int32)
    ys = dev_t(ys_np, device)
    # distances
    got = _native.pairdist_forward(x, I_d, J_d).cpu().numpy()
    assert np.array_equal(got, d_host), what
    # chi^2 through the log-prob (tau = 1: lp = -0.5 chi^2 exactly)
    want_lp = np.array([-0.5 * np.sum((d_host[c] - ys_np) ** 2) * 1.0 + P * 0.5 * np.log(1.0) for c in range(C)])
    assert np.array_equal(abi.logp(x, I_d, J_d, ys, C, n, give).cpu().numpy(), want_lp), what
    memo = _native.new_chi2_memo(C, 3 * n, device)
    for step in ('miss', 'hit'):
        lp, sk = abi.logp_memo(x, I_d, J_d, ys, C, n, give, memo)
        assert np.array_equal(lp.cpu().numpy(), want_lp), (what, step)
        assert bool((sk[:C] != 0).all()) == (step == 'hit'), (what, step)
    # the one-launch energy (up to 2048 beads)
    if n > 2048:
        return
    pm = np.random.RandomState(C).standard_normal((C, 3 * n))
    en, lp = abi.energy(x, dev_t(pm, device), I_d, J_d, ys, C, n, give)
    assert np.array_equal(lp.cpu().numpy(), want_lp), what
    en = en.cpu().numpy()
    worst = 0.0
    for c in sorted({0, H // 2, H - 1}):
        if not np.isfinite(want_lp[c]):
            continue
        xc = xs[c]
        P_exact = decimal.Decimal(0)
        for q in range(P):
            dv, dd = PE.exact_pair(xc[I[q]], xc[J[q]])
            rr = PE.CTX.subtract(dd, PE.dec(ys_np[q]))
            P_exact = PE.CTX.add(P_exact, PE.CTX.multiply(rr, rr))
        K_exact = decimal.Decimal(0)
        for v in pm[c]:
            K_exact = PE.CTX.add(K_exact, PE.CTX.multiply(PE.dec(v), PE.dec(v)))
        E_exact = PE.CTX.multiply(decimal.Decimal('0.5'), PE.CTX.add(K_exact, P_exact))
        r = d_host[c] - ys_np
        bound = energy_bound(d_host[c], r, pm[c], en[c])
        err = abs(float(PE.CTX.subtract(PE.dec(en[c]), E_exact)))
        assert err <= bound, (what, c, err, bound)
        worst = max(worst, err / bound)
    print('energy %s: worst error / bound %.3g' % (what, worst))


# ---------------------------------------------------------------------------
# 2. the force of every family against the 50-digit force
# ---------------------------------------------------------------------------
def force_case(n, seed, eq_bead=None):
    """coordinates [n, 3] and a symmetric target matrix; bead eq_bead at equilibrium
    (its targets its exact distances, rounded once)"""
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((n, 3)) * 2.0
    I, J = np.triu_indices(n, 1)
    d = np.sqrt(host_sq(x, I, J))
    ys = np.abs(d + 0.1 * rs.standard_normal(len(I)))
    ym = sym_ymat(n, ys)
    if eq_bead is not None:
        for j in range(n):
            if j != eq_bead:
                ym[eq_bead, j] = ym[j, eq_bead] = PE.exact_distance(x[eq_bead], x[j])
    return x, ym


def rows_to_check(n, eq_bead):
    rows = {0, 1, n - 1, n - 2, eq_bead}
    for b in range(64, n, 64):                         # both sides of every 64-bead block edge
        rows |= {b - 1, b}
    if n > 2048:                                       # the 50-digit rows cost n each
        return sorted({0, 64, n // 2, n - 65, n - 1, eq_bead})
    if len(rows) > 14:
        edges = sorted(r for r in rows if r not in (0, 1, n - 1, n - 2, eq_bead))
        keep = edges[:4] + edges[-4:] + edges[len(edges) // 2 - 1:len(edges) // 2 + 1]
        rows = {0, 1, n - 1, n - 2, eq_bead} | set(keep)
    return sorted(r for r in rows if 0 <= r < n)


def check_force(got, x, ym, tau, rows, ctx):
    n = x.shape[0]
    ex = PE.force_rows(x, ym, tau, rows)
    A, W = PE.force_scales(x, ym, rows)
    worst = 0.0
    for i in rows:
        for k in range(3):
            bound = tau * (EPS_W * A[i][k] + (n + 2) * U * W[i][k])
            err = abs(float(PE.CTX.subtract(PE.dec(got[i, k]), ex[i][k])))
            assert err <= bound, (ctx, i, k, err, bound, got[i, k], float(ex[i][k]))
            worst = max(worst, err / bound)
    return worst


def test_pair_weight_reciprocal_within_the_measured_seed_bound(device):
    """The measurement EPS_W rests on: 1/d after the v_rsq_f64 seed and one Newton step,
    read back through the one-sided force kernel.  Two beads, (0, 0, 0) and (a, 0, 0) with a
    of 26 significant bits (s = a*a exact), target y = 1.5 2^k for a in [2^k, 2^(k+1)), tau = 1:
    the force on bead 1 is fl(w a) with w = fl(1 - y r), so r = (1 - F/a)/y recovers r to
    within ~3u.  Over 2^-600 .. 2^600 the worst relative error of r must stay inside the
    1.5 2^-48 the bound assumes (plus 4u of read-back rounding); the figure is printed."""
    rs = np.random.RandomState(1)
    per = 1024
    m = rs.randint(1 << 25, 1 << 26, size=per).astype(np.float64)
    worst = 0.0
    from fractions import Fraction
    for k in range(-300, 301, 25):
        a = np.ldexp(m, k - 25)
        x = np.zeros((per, 6))
        x[:, 3] = a
        y = float(np.ldexp(1.5, k))
        ymat = dev_t(np.array([[0.0, y], [y, 0.0]]), device)
        F = _native.pairdist_gauss_grad(dev_t(x, device), ymat, 1.0).cpu().numpy()[:, 3]
        for Fi, ai in zip(F, a):
            r = (1 - Fraction(Fi) / Fraction(ai)) / Fraction(y)
            worst = max(worst, abs(float(r * Fraction(ai) - 1)))
    print('1/d after seed + Newton: worst relative error %.3e = 2^%.2f' % (worst, math.log2(worst)))
    assert worst <= 1.5 * 2.0 ** -48 + 4 * U


# (n, C, packed, tiles workspace, family)
FORCE_CASES = [(20, 3, False, False, 'one-sided, 4 lanes per bead'),
               (20, 1024, False, False, 'one-sided, 1 lane per bead'),
               (32, 2, True, False, 'sym nblk 1'),
               (64, 2, False, False, 'sym nblk 1 full, targets through LDS'),
               (100, 2, True, False, 'sym nblk 2 ragged'),
               (192, 2, True, False, 'sym nblk 3 full'),
               (250, 2, False, False, 'sym nblk 4 ragged, targets through LDS'),
               (256, 2, True, False, 'sym nblk 4 full'),
               (320, 2, True, False, 'ring full'),
               (700, 2, True, False, 'ring ragged, odd nblk'),
               (1024, 1, True, False, 'ring full, 16 blocks'),
               (300, 2, True, True, 'tiles ragged'),
               (1500, 1, True, True, 'tiles beyond 1024'),
               (8192, 1, True, True, 'tiles at 8192'),
               (300, 2, False, False, 'one-sided without packed targets'),
               (1100, 1, False, False, 'one-sided beyond 1024, without packed targets')]


def run_grad(abi, xx, ymat, packed, ws, C, n, tau):
    out = torch.empty_like(xx)
    nb = 0 if ws is None else ws.numel() * 8
    assert abi.L.binf_pairdist_gauss_grad_packed_f64(pp(xx), pp(ymat), pp(packed), float(tau), None, pp(out), C, n,
                                                     pp(ws), nb, abi.st) == 0
    return out


def tiles_ws(abi, C, n, give):
    need = abi.L.binf_pairdist_tiles_workspace_bytes(C, n)
    if not give:
        return None
    assert need > 0
    return torch.empty(need // 8, dtype=torch.float64, device=abi.device)


@pytest.mark.parametrize('n,C,use_packed,give_ws,family', FORCE_CASES)
def test_force_of_every_family_against_50_digit_arithmetic(device, n, C, use_packed, give_ws, family):
    abi = Abi(device)
    eq = min(65, n - 3)
    x0, ym = force_case(n, 3 * n + C, eq_bead=eq)
    rs = np.random.RandomState(n)
    xs = np.concatenate([x0[None], x0[None] + 0.3 * rs.standard_normal((C - 1, n, 3))]) if C > 1 else x0[None]
    xx = dev_t(xs.reshape(C, 3 * n), device)
    ymat = dev_t(ym, device)
    packed = _native.pairdist_pack_targets(ymat) if use_packed else None
    if use_packed:
        assert packed is not None, family
    ws = tiles_ws(abi, C, n, give_ws)
    tau = 1.75
    g = run_grad(abi, xx, ymat, packed, ws, C, n, tau).cpu().numpy().reshape(C, n, 3)
    rows = rows_to_check(n, eq)
    worst = check_force(g[0], x0, ym, tau, rows, family)
    if C > 1:                                          # the last chain as well (few rows)
        worst = max(worst, check_force(g[C - 1], xs[C - 1], ym, tau, [0, n - 1, eq], family))
    # the equilibrium bead: its exact force is ~0, its error inside the same bound
    assert np.abs(g[0, eq]).max() <= tau * EPS_W * 4 * np.abs(x0[eq][None] - x0).sum() + 1e-300
    print('force %s (n=%d): worst error / bound %.3g' % (family, n, worst))


# ---------------------------------------------------------------------------
# 3. coincident beads
# ---------------------------------------------------------------------------
COINCIDE_CASES = [(20, 3, False, False), (20, 1024, False, False), (100, 2, True, False), (128, 2, False, False),
                  (250, 2, True, False), (1024, 1, True, False),
                  (320, 2, True, False), (700, 2, True, False), (300, 2, True, True), (1500, 1, True, True),
                  (300, 2, False, False), (1100, 1, False, False)]


@pytest.mark.parametrize('n,C,use_packed,give_ws', COINCIDE_CASES)
def test_coincident_beads_give_the_definitions_nan_pattern(device, n, C, use_packed, give_ws):
    abi = Abi(device)
    x0, ym = force_case(n, 7 * n)
    # coincident pairs where each masked or unmasked select of the ring / tile / sym kernels
    # meets them: a diagonal tile (always masked: its last half step), a tile across a block
    # edge, the last block's diagonal tile and, for n > 64, a tile pairing block 0 with the last
    # block (masked when n is ragged)
    pairs = [(10, 12), (3, 70 if n > 70 else n - 1), (n - 5, n - 4)]
    if n > 64:
        pairs.append((20, n - 3))
    for a, b in pairs:
        x0[b] = x0[a]
    co = sorted({v for pr in pairs for v in pr})
    assert len(co) == 2 * len(pairs)
    o = n - 2                                          # a real bead at the origin: the ghosts of a ragged
    x0[o] = 0.0                                        # last block sit there too, and are masked
    assert o not in co
    xs = np.repeat(x0[None], C, axis=0)
    xx = dev_t(xs.reshape(C, 3 * n), device)
    ymat = dev_t(ym, device)
    packed = _native.pairdist_pack_targets(ymat) if use_packed else None
    ws = tiles_ws(abi, C, n, give_ws)
    want = np.zeros((n, 3), dtype=bool)
    want[co] = True
    ex = PE.force_rows(x0, ym, 1.0, co + [o, 0])
    assert all(v.is_nan() for b in co for v in ex[b]) and not any(v.is_nan() for v in ex[o] + ex[0])
    g = run_grad(abi, xx, ymat, packed, ws, C, n, 1.0).cpu().numpy().reshape(C, n, 3)
    for c in (0, C - 1):
        assert np.array_equal(np.isnan(g[c]), want), (n, c)
        assert np.isfinite(g[c][~want]).all()
    # distances and chi^2: finite and bitwise
    I, J = np.triu_indices(n, 1)
    d_host = np.sqrt(host_sq(x0, I, J))
    I_d, J_d = dev_t(I, device, torch.int32), dev_t(J, device, torch.int32)
    got = _native.pairdist_forward(xx[:1], I_d, J_d).cpu().numpy()[0]
    assert np.array_equal(got, d_host) and np.isfinite(got).all()
    assert all(got[(I == a) & (J == b)][0] == 0.0 for a, b in pairs)
    ys_np = ym[I, J]
    lp = abi.logp(xx[:1], I_d, J_d, dev_t(ys_np, device), 1, n, True).cpu().numpy()[0]
    assert lp == -0.5 * np.sum((d_host - ys_np) ** 2) * 1.0 + len(I) * 0.5 * np.log(1.0)
    if n > 1024 and ws is None:                        # no fused leapfrog here (the library refuses it)
        return
    # fused leapfrog and the per-step tier, both modes, one step: after the half kick p_i, p_j
    # are NaN, the drift carries that to q_i, q_j, and the second half kick to every p
    rs = np.random.RandomState(n)
    p0 = dev_t(rs.standard_normal((C, 3 * n)), device)
    prior = (0.05, 0.1)
    for mode in (_native.MODE_EXACT, _native.MODE_FMA):
        for L in (1, 2):
            qa, pa = xx.clone(), p0.clone()
            nb = 0 if ws is None else ws.numel() * 8
            assert abi.L.binf_pairdist_leapfrog_packed_f64(pp(qa), None, pp(pa), pp(ymat), pp(packed), 1.0, None, 1,
                                                           prior[0], prior[1], 1, 1e-3, None, L, C, n, mode,
                                                           pp(ws), nb, abi.st) == 0
            qb, pb = xx.clone(), p0.clone()

            def force(q):
                return _native.sum_terms([_native.gauss_grad(q, prior[0], prior[1]),
                                          run_grad(abi, q, ymat, packed, ws, C, n, 1.0)])
            _native.leapfrog_kick(pb, force(qb), 1e-3, None, half=True, mode=mode)
            _native.leapfrog_drift(qb, pb, 1e-3, None, mode=mode)
            for _ in range(L - 1):
                _native.leapfrog_kick_drift(qb, pb, force(qb), 1e-3, None, mode=mode)
            _native.leapfrog_kick(pb, force(qb), 1e-3, None, half=True, mode=mode)
            qa, pa, qb, pb = (t.cpu().numpy().reshape(C, n, 3) for t in (qa, pa, qb, pb))
            assert np.array_equal(qa, qb, equal_nan=True) and np.array_equal(pa, pb, equal_nan=True), (mode, L)
            if L == 1:
                assert np.array_equal(np.isnan(qa[0]), want) and np.isnan(pa[0]).all(), (mode, L)
            else:
                assert np.isnan(qa[0]).all() and np.isnan(pa[0]).all(), (mode, L)


# ---------------------------------------------------------------------------
# 4. trajectories against a 50-digit integration
# ---------------------------------------------------------------------------
def trajectory_bound(x0, p0, ym, tau, prior, dt, L, grads):
    """Componentwise bound on |z~ - z*| after L leapfrog steps (hmc.py:116-123).

    Let eq, ep bound the deviation of the kernel's q, p from the exact ones.  A kick
    p' = p - h g(q) with the kernel's force g~(q~) = g(q~) + e, |e| <= B (the force
    bound of test 2 plus the prior's k (q - x0) and the term sum: 3u |g|), rounds once
    or twice (exact mode: h g and the difference; FMA mode: once), so

        ep' <= ep + h (Hrow eq_max + B) + u (|p'| + |h g|)

    with Hrow_i = tau sum_j 2 (|w_ij| + |y_ij / d_ij|) + k a row-sum bound of the energy's
    Hessian (first order: g(q~) - g(q) = H dq).  A drift q' = q + dt p rounds likewise:

        eq' <= eq + dt ep + u (|q'| + |dt p|).

    h = dt / 2 is exact.  Everything is evaluated on the exact trajectory; the test
    allows twice the result (the first-order remainder and the difference between
    the exact and the kernel's trajectory where the magnitudes are taken)."""
    n = x0.shape[0]
    k = prior[0]
    eq, ep = np.zeros((n, 3)), np.zeros((n, 3))
    q, p = x0.copy(), p0.copy()
    rows = list(range(n))
    for e, g in enumerate(grads):                      # L + 1 kicks, a drift between two
        if e > 0:
            qn = q + dt * p
            eq = eq + dt * ep + U * (np.abs(qn) + np.abs(dt * p))
            q = qn
        step = 0.5 * dt if e in (0, L) else dt
        g = PE.to_f64(g)
        A, W = PE.force_scales(q, ym, rows)
        B = (tau * (EPS_W * np.array([A[i] for i in rows]) + (n + 2) * U * np.array([W[i] for i in rows]))
             + 3 * U * (np.abs(g) + k * np.abs(q - prior[1])))
        dv = q[:, None, :] - q[None, :, :]
        d = np.sqrt((dv * dv).sum(axis=2))
        np.fill_diagonal(d, 1.0)
        r = np.abs(ym / d)
        np.fill_diagonal(r, 0.0)
        Hrow = tau * 2.0 * (np.abs(1.0 - r) + r).sum(axis=1) + k
        p = p - step * g
        ep = ep + step * (Hrow[:, None] * eq.max() + B) + U * (np.abs(p) + np.abs(step * g))
    return 2.0 * eq, 2.0 * ep


# (n, C, packed, tiles workspace, family)
TRAJ_CASES = [(20, 1, False, False, 'one-sided'), (100, 1, True, False, 'sym'),
              (300, 1, True, False, 'ring'), (300, 1, True, True, 'tiles')]


@pytest.fixture(scope='module')
def exact_trajectories():
    return {}


def traj_inputs(n):
    x0, ym = force_case(n, 11 * n)
    rs = np.random.RandomState(5 * n)
    p0 = rs.standard_normal((n, 3))
    return x0, ym, p0


@pytest.mark.parametrize('n,C,use_packed,give_ws,family', TRAJ_CASES)
def test_fused_leapfrog_against_50_digit_trajectory(device, exact_trajectories, n, C, use_packed, give_ws,
                                                    family):
    abi = Abi(device)
    x0, ym, p0 = traj_inputs(n)
    tau, prior, dt, L = 1.5, (0.05, 0.1), 2e-3, 3
    if n not in exact_trajectories:
        q, p, grads = PE.exact_leapfrog(x0, p0, ym, tau, prior, dt, L)
        bq, bp = trajectory_bound(x0, p0, ym, tau, prior, dt, L, grads)
        exact_trajectories[n] = (q, p, bq, bp)
    qd, pd, bq, bp = exact_trajectories[n]
    ymat = dev_t(ym, device)
    packed = _native.pairdist_pack_targets(ymat) if use_packed else None
    ws = tiles_ws(abi, C, n, give_ws)
    worst = 0.0
    for mode in (_native.MODE_EXACT, _native.MODE_FMA):
        qa, pa = dev_t(x0.reshape(1, -1), device), dev_t(p0.reshape(1, -1), device)
        nb = 0 if ws is None else ws.numel() * 8
        assert abi.L.binf_pairdist_leapfrog_packed_f64(pp(qa), None, pp(pa), pp(ymat), pp(packed), tau, None, 1,
                                                       prior[0], prior[1], 1, dt, None, L, C, n, mode,
                                                       pp(ws), nb, abi.st) == 0
        qg, pg = qa.cpu().numpy().reshape(n, 3), pa.cpu().numpy().reshape(n, 3)
        for got, ex, b, what in ((qg, qd, bq, 'q'), (pg, pd, bp, 'p')):
            err = np.array([[abs(float(PE.CTX.subtract(PE.dec(got[i, a]), ex[i][a]))) for a in range(3)]
                            for i in range(n)])
            assert (err <= b).all(), (family, mode, what, float((err / b).max()))
            worst = max(worst, float((err / b).max()))
    print('trajectory %s: worst error / bound %.3g' % (family, worst))


@pytest.mark.parametrize('n', [20, 100, 300])
def test_hmc_sample_against_50_digit_trajectory(device, exact_trajectories, n):
    """HMCSampler.sample() with the fused leapfrog and the one-launch energy: the accepted
    state is the exact trajectory's end within trajectory_bound, the energy before the
    move the exact one within energy_bound plus the prior's sum."""
    from binf_amd.example.distance import make_distance_likelihood
    from binf_amd.pdf import IsotropicGaussian
    from binf_amd.pdf.posteriors import Posterior
    from binf_amd.samplers.hmc import HMCSampler
    x0, ym, p0 = traj_inputs(n)
    tau, prior, dt, L = 1.5, (0.05, 0.1), 2e-3, 3
    if n not in exact_trajectories:
        q, p, grads = PE.exact_leapfrog(x0, p0, ym, tau, prior, dt, L)
        bq, bp = trajectory_bound(x0, p0, ym, tau, prior, dt, L, grads)
        exact_trajectories[n] = (q, p, bq, bp)
    qd, pd, bq, bp = exact_trajectories[n]
    I, J = np.triu_indices(n, 1)
    lik = make_distance_likelihood(ym[I, J], n)
    pri = IsotropicGaussian(prior[0], prior[1], name='coordinates_prior', variable_name='coordinates')
    cond = Posterior({lik.name: lik}, {pri.name: pri}).conditional_factory(precision=tau)
    s = HMCSampler(cond, dev_t(x0.reshape(1, -1), device), dt, L, variable_name='coordinates',
                   record_energies=True)
    assert s.fused_leapfrog and s.fused_energy
    out = s.sample(p0=dev_t(p0.reshape(1, -1), device), u=dev_t(np.array([1e-300]), device))
    assert bool(s.last_move_accepted[0])
    got = out.cpu().numpy().reshape(n, 3)
    err = np.array([[abs(float(PE.CTX.subtract(PE.dec(got[i, a]), qd[i][a]))) for a in range(3)] for i in range(n)])
    assert (err <= bq).all(), float((err / bq).max())
    # E before = 0.5 p.p + 0.5 tau chi^2 - N/2 log tau + 0.5 k |x - x0|^2, exactly
    chi = decimal.Decimal(0)
    for a_, b_ in zip(I, J):
        rr = PE.CTX.subtract(PE.exact_pair(x0[a_], x0[b_])[1], PE.dec(ym[a_, b_]))
        chi = PE.CTX.add(chi, PE.CTX.multiply(rr, rr))
    kin = sum((PE.dec(v) * PE.dec(v) for v in p0.reshape(-1)), decimal.Decimal(0))
    pri_s = sum(((PE.dec(v) - PE.dec(prior[1])) ** 2 for v in x0.reshape(-1)), decimal.Decimal(0))
    half = decimal.Decimal('0.5')
    ln_tau = decimal.Decimal(tau).ln(PE.CTX)
    E = half * kin + half * PE.dec(tau) * chi - half * len(I) * ln_tau + half * PE.dec(prior[0]) * pri_s
    eb = float(s.last_e_before[0])
    # the distances' and residuals' roundings as in energy_bound, scaled by tau; every sum
    # (pairwise, <= 3n or N terms) and the handful of scalar operations joining the four
    # terms within (log2 N + 40) u of the sum of their magnitudes (log tau: 2u)
    d = np.sqrt(host_sq(x0, I, J))
    r = d - ym[I, J]
    e = 4 * U * d + U * np.abs(r)
    mags = (0.5 * float(kin) + 0.5 * tau * float(chi) + 0.5 * len(I) * abs(math.log(tau))
            + 0.5 * prior[0] * float(pri_s))
    bound = 0.5 * tau * float(((2 * np.abs(r) + e) * e).sum()) + (math.log2(len(I)) + 40) * U * mags
    assert abs(float(PE.CTX.subtract(PE.dec(eb), E))) <= bound, (float(E), eb, bound)
