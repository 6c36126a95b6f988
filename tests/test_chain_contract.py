"""The host restatement of the chain-resident kernels (tests/chain_contract.py) held to the
truth on its own, without a GPU: a restatement written by reading a kernel's contract can
share the kernel's mistakes.

    fma          oracle_fma_f64 against exact rational arithmetic, correctly rounded;
    tree         the derived leaves against np.sum (bits) and the library's exported geometry;
    integer      on integer data every order gives the same bits: the three layouts return the
                 exact force and the exact leapfrog trajectory, in both modes;
    bound        on the float designs of tests/grad_bounds.py each restated force lies inside
                 the DERIVED force bound against its exact value (the bound the MFMA kernels
                 meet), a 10-step trajectory inside that bound propagated through the leapfrog
                 map (poly_bounds.PolyBound.transition, parametrised by it);
    injections   five departures the old 1e-10 bar lets through, each of which changes bits;
    ties         no accept test of the GPU file's cases is within 8 ulp of a tie, under any of
                 the three candidates of log tau: the GPU test may assert every flag."""
from fractions import Fraction

import numpy as np
import pytest

import chain_contract as CC
import grad_bounds as GB
import linear_resident_ref as RR
import poly_bounds as PB
from binf_amd import _native
from oracle import c_oracle


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---------------------------------------------------------------------------
# fma
# ---------------------------------------------------------------------------
def fma_triples():
    rs = np.random.RandomState(53)
    n = 2000
    def mant(size):
        return rs.randint(2 ** 52, 2 ** 53, size=size).astype(np.float64) * rs.choice([-1.0, 1.0], size=size)
    out = []
    # random, exponents wide apart and close
    a, b = mant(n) * 2.0 ** rs.randint(-80, 80, size=n), mant(n) * 2.0 ** rs.randint(-80, 80, size=n)
    out.append((a, b, mant(n) * 2.0 ** rs.randint(-160, 160, size=n)))
    out.append((a, b, a * b * (1.0 + rs.randint(-4, 5, size=n) * 2.0 ** -50) * -1.0))
    # cancelling to a few bits: c = -(a b rounded), the result is the product's rounding error
    out.append((a, b, -(a * b)))
    out.append((a, b, -(a * b) * (1.0 + 2.0 ** -52)))
    # the product is a rounding midpoint: two odd 27-bit factors give an odd 54-bit integer
    f, g = (2 * rs.randint(2 ** 25 + 2 ** 24, 2 ** 26, size=n) + 1).astype(np.float64), \
        (2 * rs.randint(2 ** 25 + 2 ** 24, 2 ** 26, size=n) + 1).astype(np.float64)
    assert np.all(f * g >= 2.0 ** 53)
    tiny = rs.choice([0.0, 2.0 ** -300, -2.0 ** -300, 1.0, -1.0, 0.5, -0.5], size=n)
    out.append((f, g * rs.choice([-1.0, 1.0], size=n), tiny))
    # subnormal results, and the smallest normals
    e = rs.randint(-1080, -1015, size=n)
    out.append((mant(n) * 2.0 ** -52, mant(n) * 2.0 ** -52 * 2.0 ** e.astype(np.float64), mant(n) * 2.0 ** -1126 *
                rs.choice([0.0, 1.0], size=n)))
    return [np.concatenate([t[i] for t in out]) for i in range(3)]


def exact_fma(a, b, c):
    """fma of finite doubles from exact rational arithmetic; int / int division is correctly rounded."""
    r = Fraction(a) * Fraction(b) + Fraction(c)
    if r != 0:
        return float(r)
    if a * b == 0 and c == 0:                 # a sum of two zeros: -0 only if both are
        return -0.0 if (np.signbit(a) != np.signbit(b)) and np.signbit(c) else 0.0
    return 0.0                                # exact cancellation rounds to +0


def test_fma_is_the_correctly_rounded_fused_multiply_add():
    a, b, c = fma_triples()
    assert len(a) >= 10000
    got = c_oracle.fma(a, b, c)
    want = np.array([exact_fma(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)])
    assert same_bits(got, want), int(np.sum(bits(got) != bits(want)))
    assert np.sum(got != a * b + c) > 3000          # ... and is not the unfused expression
    assert np.sum((got != 0) & (np.abs(got) < 2.0 ** -1022)) > 500, 'no subnormal results'
    # signed zeros, infinities, NaN: the rules of IEEE 754
    z, i, q = 0.0, np.inf, np.nan
    special = [(z, 3.0, z, z), (-z, 3.0, z, z), (-z, 3.0, -z, -z), (z, -3.0, -z, -z), (z, z, -z, z), (2.0, 3.0, -6.0, z),
               (-2.0, 3.0, 6.0, z), (i, 2.0, 1.0, i), (-i, 2.0, 1.0, -i), (i, z, 1.0, q), (i, 1.0, -i, q), (i, 1.0, i, i),
               (2.0, 3.0, i, i), (2.0, 3.0, -i, -i), (q, 1.0, 1.0, q), (1.0, q, 1.0, q), (1.0, 1.0, q, q),
               (2.0 ** 1023, 2.0, -2.0 ** 1023, 2.0 ** 1023), (2.0 ** 1023, 2.0, z, i)]
    with np.errstate(all='ignore'):
        sa, sb, sc, sw = [np.array(v) for v in zip(*special)]
        got = c_oracle.fma(sa, sb, sc)
    for g, w, row in zip(got, sw, special):
        assert (np.isnan(g) and np.isnan(w)) or (g == w and np.signbit(g) == np.signbit(w)), row
    # broadcasting, as the restatement calls it
    assert c_oracle.fma(np.ones((3, 1)), np.arange(4.0), 1.0).shape == (3, 4)


# ---------------------------------------------------------------------------
# the tree
# ---------------------------------------------------------------------------
def test_derived_leaves_are_numpys_and_the_librarys_for_every_length_to_1024():
    rs = np.random.RandomState(8)
    raggeds = 0
    for N in range(1025):
        x = rs.standard_normal((3, N)) * 10.0 ** rs.uniform(-6, 6, size=(3, N))
        got = CC.np_sum(x)
        assert same_bits(got, [np.sum(row) for row in x]), N
        H, lv = CC.leaves(N)
        assert H == _native.pairwise_tree_height(N) == CC.tree_height(N), N
        assert [_native.pairwise_leaf(N, H, path) for path in range(1 << H)] == lv, N
        # the canonical leaves tile 0 .. N in order; the lane slots own every datum once
        canon = [l for l in lv if l[3]]
        assert [l[0] for l in canon] == list(np.cumsum([0] + [l[1] for l in canon])[:-1]), N
        assert sum(l[1] for l in canon) == N and all(l[1] <= 128 for l in lv)
        L = CC.Lanes(N)
        owned = np.sort(L.idx[:, L.canon][L.mask[:, L.canon]])
        assert np.array_equal(owned, np.arange(N)), N
        raggeds += CC.ragged(N)
    assert raggeds > 100 and CC.ragged(257) and CC.ragged(513) and not CC.ragged(1024)
    assert [l[2] for l in CC.leaves(257)[1] if l[3]] == [1, 2, 2]
    assert same_bits(CC.np_sum(np.zeros(0)), 0.0) and same_bits(CC.np_sum(np.array([-0.0])), 0.0)
    # the coefficient sums are the same rule: both branches (K < 8, K >= 8)
    for K in CC.K_LINEAR:
        x = rs.standard_normal((4, K))
        assert same_bits(CC.np_sum(x), [np.sum(row) for row in x]), K


# ---------------------------------------------------------------------------
# integer tier
# ---------------------------------------------------------------------------
def layouts_of(A_or_xs, ys, K, N, fused, poly, inject=None):
    """The restatements that cover a problem: the linear one on the design matrix, and for a
    polynomial design (given as abscissae) the two polynomial layouts as well."""
    if not poly:
        return [CC.Contract('linear', A_or_xs, ys, fused=fused, inject=inject)]
    A = np.vstack([np.asarray(A_or_xs, dtype=np.float64) ** k for k in range(K)])
    out = [CC.Contract('linear', A, ys, fused=fused, inject=inject),
           CC.Contract('poly', A_or_xs, ys, K=K, fused=fused, inject=inject)]
    if N <= 128:
        out.append(CC.Contract('lane', A_or_xs, ys, K=K, fused=fused, inject=inject))
    return out


INTEGER_FORCE_SHAPES = [(1, 1), (3, 7), (5, 48), (16, 129), (9, 257), (13, 513), (16, 1024)]


@pytest.mark.parametrize('K,N', INTEGER_FORCE_SHAPES)
def test_integer_force_is_exact_in_both_modes(K, N):
    assert GB.integer_case_width(K, N) <= 53
    A, ys, theta, tau = GB.integer_case(K, N, 7, seed=K + N)
    want = GB.integer_force(A, ys, theta, tau)
    for fused in (False, True):
        con = CC.Contract('linear', A, ys, fused=fused)
        assert same_bits(con.force(theta, tau), want)
        chi2 = ((theta.astype(np.int64).dot(A.astype(np.int64)) - ys.astype(np.int64)) ** 2).sum(axis=1)
        assert same_bits(con.chi2(theta), chi2.astype(np.float64))


def poly_integer_case(K, N, C, seed):
    """Small integer abscissae under the data of grad_bounds.leapfrog_case."""
    _, ys, q, p, tau_exp = GB.leapfrog_case(K, N, C, seed)
    xs = np.random.RandomState(seed + 1).randint(-2, 3, size=N)
    A = np.vstack([xs ** k for k in range(K)]).astype(np.int64)
    return xs, A, ys, q, p, tau_exp


@pytest.mark.parametrize('poly,K,N,L,dte', [(False, 5, 48, 2, 4), (False, 16, 129, 2, 5), (False, 3, 257, 3, 5),
                                            (False, 9, 513, 2, 6), (False, 13, 1024, 2, 6), (False, 1, 1, 3, 1),
                                            (True, 1, 7, 3, 2), (True, 3, 37, 2, 4), (True, 4, 128, 2, 6),
                                            (True, 4, 257, 2, 6), (True, 3, 513, 2, 7)])
def test_integer_leapfrog_is_exact_in_both_modes(poly, K, N, L, dte):
    C = 5
    if poly:
        xs, A, ys, q, p, tau_exp = poly_integer_case(K, N, C, seed=N)
    else:
        A, ys, q, p, tau_exp = GB.leapfrog_case(K, N, C, seed=N)
        xs = None
    qi, pi, width = GB.leapfrog_ints(A, ys, q, p, tau_exp, dte, L)
    assert width <= 53, width                     # every intermediate of every order is a double
    tau, dt = 2.0 ** tau_exp, 2.0 ** -dte
    Af, yf = A.astype(np.float64), ys.astype(np.float64)
    fq, fp = zip(*[GB.leapfrog_fraction(A, ys, q[c], p[c], tau[c], dt, L) for c in range(C)])
    want_q, want_p = np.array(fq, dtype=np.float64), np.array(fp, dtype=np.float64)
    assert same_bits(want_q, qi) and same_bits(want_p, pi)
    for fused in (False, True):
        for con in layouts_of(xs if poly else Af, yf, K, N, fused, poly):
            got_q, got_p = con.leapfrog(q.astype(np.float64), p.astype(np.float64), tau, dt, L)
            assert same_bits(got_q, want_q) and same_bits(got_p, want_p), (con.layout, fused)
            assert same_bits(con.force(q.astype(np.float64), tau),
                             GB.integer_force(Af, yf, q.astype(np.float64), tau))


# ---------------------------------------------------------------------------
# bound tier
# ---------------------------------------------------------------------------
BOUND_SHAPES = [(4, 20), (7, 37), (9, 200), (16, 129), (3, 513), (16, 1024)]
STEP_ROUNDINGS = 2.0           # each of two trajectories rounds every product and sum of a step once


def bound_case(kind, K, N, C, seed):
    A, ys, theta, tau = GB.float_case(kind, K, N, C, seed)
    xs = (np.linspace(-1.0, 1.0, N) if N > 1 else np.array([0.75])) if kind == 'poly' else None
    return A, xs, ys, theta, tau


def trajectory_bound(A, ys, theta, p0, tau, dt, L):
    """numpy's trajectory of one chain and the derived per-evaluation bound propagated through
    the leapfrog map: two evaluations that each lie inside the bound differ by at most two."""
    case = RR.Case(A, ys)
    fb = lambda q, t: 2.0 * GB.force_float(q[None, :], A, ys, t)[1][0]
    return case.pb.transition(theta, p0, tau, dt, L, force_bound=fb, step_roundings=STEP_ROUNDINGS)


@pytest.mark.parametrize('kind', GB.DESIGNS)
def test_restated_force_and_trajectory_lie_inside_the_derived_bound(kind):
    worst_f, worst_q, bar_ratio = 0.0, 0.0, np.inf
    for K, N in BOUND_SHAPES:
        C, L = 3, 10
        A, xs, ys, theta, tau = bound_case(kind, K, N, C, seed=K * N)
        ef = GB.ExactForce(A, ys)
        rs = np.random.RandomState(K + N)
        scale = 1.0 / np.maximum(np.max(np.abs(A), axis=1), 2.0 ** -40)
        dt = CC.stable_dt(A, tau.max(), safety=0.25)
        p0 = rs.standard_normal((C, K)) * scale * 0.1 / (L * dt)       # every coefficient moves by ~ a tenth of its size
        exact = [ef.chain(theta[c], tau[c]) for c in range(C)]
        for fused in (False, True):
            for con in layouts_of(xs if kind == 'poly' else A, ys, K, N, fused, kind == 'poly'):
                g = con.force(theta, tau)
                for c in range(C):
                    err, bound = ef.error(exact[c]['G'], g[c]), exact[c]['bound']
                    assert np.all(err <= bound), (con.layout, K, N, err, bound)
                    ratio = err[bound > 0] / bound[bound > 0]          # a row of zeros: force and bound are 0
                    worst_f = max(worst_f, float(ratio.max()))
                    bar_ratio = min(bar_ratio, float(np.min((GB.OLD_BAR * exact[c]['scale'])[bound > 0] / bound[bound > 0])))
                q, _ = con.leapfrog(theta, p0, tau, dt, L)
                for c in range(C):
                    t = trajectory_bound(A, ys, theta[c], p0[c], tau[c], dt, L)
                    err = np.abs(q[c] - t['q'])
                    assert np.all(err <= t['bq']), (con.layout, fused, K, N, err, t['bq'])
                    ratio = err[t['bq'] > 0] / t['bq'][t['bq'] > 0]
                    worst_q = max(worst_q, float(ratio.max()))
    print('%s: restated force error / derived bound %.3g, 10-step trajectory difference / propagated bound %.3g, '
          'old bar / derived bound >= %.3g' % (kind, worst_f, worst_q, bar_ratio))


# ---------------------------------------------------------------------------
# injected errors: each passes the old bar and changes bits
# ---------------------------------------------------------------------------
INJECTION_SHAPES = [(4, 20), (8, 128), (9, 200), (16, 129), (5, 257), (3, 513), (5, 920), (16, 1024)]


@pytest.mark.parametrize('inject', CC.INJECTIONS)
def test_an_injected_error_passes_the_old_bar_and_changes_bits(inject):
    changed = []
    for layout in ('linear', 'poly', 'lane'):
        for K, N in INJECTION_SHAPES:
            if layout == 'lane' and N > 128:
                continue
            C, L = 3, 10
            design, A, ys, theta, tau = CC.data(layout, K, N, C, seed=K + N)
            p0 = np.random.RandomState(N).standard_normal((C, K))
            dt = CC.stable_dt(A, 4.0)
            clean = CC.Contract(layout, design, ys, K=K)
            dirty = CC.Contract(layout, design, ys, K=K, inject=inject)
            qc, _ = clean.leapfrog(theta, p0, tau, dt, L)
            qd, _ = dirty.leapfrog(theta, p0, tau, dt, L)
            case = RR.Case(A, ys)
            for c in range(C):
                t = case.transition(theta[c], p0[c], tau[c], dt, L)
                for name, q in (('clean', qc), (inject, qd)):
                    err = np.abs(q[c] - t['q'])
                    assert np.all(err <= t['bq']), (name, layout, K, N, float(np.max(err / t['bq'])))
            if not same_bits(qc, qd):
                changed.append((layout, K, N))
    print('%s: inside the old bar everywhere; bits differ on %d shapes: %s' % (inject, len(changed), changed))
    for layout in ('linear', 'poly') + (() if inject in ('swap_levels', 'redundant_weight') else ('lane',)):
        # one lane per chain has no butterfly and no redundant path
        assert any(s[0] == layout for s in changed), (inject, layout)


# ---------------------------------------------------------------------------
# accept ties of the GPU file's cases
# ---------------------------------------------------------------------------
def test_no_accept_test_of_the_gpu_cases_is_near_a_tie():
    flags = []
    for layout, i in CC.hmc_case_ids():
        t = CC.hmc_expect(CC.hmc_case(layout, i))
        assert np.all(t['tie_free']) and np.all(t['acc'] == t['acc'][0]), (layout, i)
        flags.append(t['acc'][0])
    for c in CC.extra_hmc_cases():                    # the cross-checks and the non-finite test's clean chains
        t = CC.hmc_expect(c)
        assert c['C'] in CC.CHAINS and np.all(t['tie_free']) and np.all(t['acc'] == t['acc'][0]), (c['layout'], c['K'], c['N'])
        flags.append(t['acc'][0])
    for layout, move, i in CC.gibbs_case_ids():
        t = CC.gibbs_expect(CC.gibbs_case(layout, move, i))
        assert t['tie_free'] and t['flags_agree'], (layout, move, i)
        flags.append(t['acc'].reshape(-1))
    flags = np.concatenate(flags)
    print('%d accept tests, %d rejected' % (len(flags), int((~flags).sum())))
    assert (~flags).sum() >= 100 and flags.sum() >= 100


def test_the_shape_lists_cover_what_the_kernels_branch_on():
    for ks, sh in ((CC.K_LINEAR, CC.LINEAR_SHAPES), (CC.K_POLY, CC.POLY_SHAPES)):
        assert sorted(set(N for _, N in sh)) == list(CC.N_LIST)
        for K in ks:
            assert (K, 1024) in sh, K
            assert any(CC.ragged(N) and CC.tree_height(N) <= CC.MAX_HEIGHT for k, N in sh if k == K), K
    assert [N for N in CC.N_LIST if CC.tree_height(N) > CC.MAX_HEIGHT] == [1023]
    assert not _native.linear_resident_supported(5, 1023) and _native.linear_resident_supported(16, 1024)
    assert all(N <= 128 for _, N in CC.LANE_SHAPES) and set(K for K, _ in CC.LANE_SHAPES) == set(CC.K_POLY)
    assert set((K + 3) // 4 * 4 for K in CC.K_LINEAR) == {4, 8, 12, 16}
    assert CC.Lanes(17).TC == 3 and CC.Lanes(7).TC == 1 and CC.Lanes(37).TC == 5      # the three force variants
    cs = [CC.hmc_case('linear', i) for i in range(len(CC.LINEAR_SHAPES))]
    for key, vals in (('C', CC.CHAINS), ('L', (1, 2, 10)), ('fused', (False, True))):
        assert set(c[key] for c in cs) == set(vals), key
    assert any(np.isscalar(c['tau']) and c['tau'] == 1.0 for c in cs) and any(not np.isscalar(c['tau']) for c in cs)
    assert any(np.isscalar(c['dt']) for c in cs) and any(not np.isscalar(c['dt']) for c in cs)
    assert set((c['prior'] is None, bool(c['prior'] and c['prior'][2])) for c in cs) == {(True, False), (False, True),
                                                                                        (False, False)}
    assert set((c['pre'] is None, c['post'] is None) for c in cs) == {(a, b) for a in (True, False) for b in (True, False)}
    assert [c['C'] for c in cs if (c['K'], c['N']) == (16, 1024)] == [300]
