"""What tests/poly_range.py claims, shown on numpy and mpmath alone (no GPU): the input classes
meet their conditions, the bounds contain numpy's own values, the bounds are tighter than the
allowance they replace, and the assertion functions the device run uses reject kernels that are
subtly wrong.  Run with -s to see the tables."""
import numpy as np
import pytest

import poly_range as P

NP = P.NumpyRoutes()


# ---------------------------------------------------------------------------
# the input classes
# ---------------------------------------------------------------------------
def test_ladder_is_what_it_says():
    L = P.LADDER
    assert len(L) == 20 and len(set(L.view(np.int64).tolist())) == 20 and np.all(np.isfinite(L))
    with np.errstate(all='ignore'):
        sq = L * L
    assert np.all(sq[:6] == 0.0) and np.all(sq[16:] == P.INF) and np.all(np.isfinite(sq[:16]))
    assert sq[14] == 2.0 ** 1022 and sq[6] == sq[7] == P.TINY and (2.0 ** -536) ** 2 == 4 * P.TINY
    assert np.signbit(L[1]) and not np.signbit(L[0])
    assert sorted(set(P.kmax_of(K) for K in P.K_LIST)) == list(P.KMAXES)
    for m in P.KMAXES:                                   # exactly full, and the first padded K
        assert m in P.K_LIST and (m == 64 or m + 1 in P.K_LIST)
    assert P.STRIDE_SHAPE[1] > 256 * 256


@pytest.mark.parametrize('N', P.N_LIST)
def test_class_f_is_finite_and_class_o_is_not(N):
    for K in sorted(set(P.CHI_K + ((P.K_LIST) if N == 9 else ()))):
        for C in P.C_LIST:
            for small in (False, True):
                f = P.case('F', K, N, C, small_ys=small)
                assert np.all(np.isfinite(f['mock'])) and np.all(np.isfinite(P.ref_chi2(f['mock'], f['ys'])))
                if N >= 1 and C >= 9 and not small:
                    assert P.class_f_holds(f), (K, N, C)
                if small and N >= 1:                     # the tiny chains: whole quanta, odd ones among them
                    chi2 = P.ref_chi2(f['mock'], f['ys'])[::3] / P.TINY
                    assert np.all(chi2 == np.round(chi2)) and np.all(chi2 <= 9 * N)
                    assert C < 9 or np.any(chi2 % 2 == 1)
            o = P.case('O', K, N, C)
            if K >= 2 and N >= 7 and C >= 9:
                assert P.class_o_holds(o), (K, N, C)
                chi2 = P.ref_chi2(o['mock'], o['ys'])
                assert np.all(np.isfinite(o['mock'][2::3])) and np.all(chi2[2::3] == P.INF)
            assert np.all(np.isfinite(o['xs'])) and not np.any(np.isnan(o['ys']))
            if N >= 2:
                assert P.INF in o['ys'] and -P.INF in o['ys']


@pytest.mark.parametrize('K', P.K_LIST)
def test_forward_cases_meet_their_conditions(K):
    f, o = P.forward_case('F', K), P.forward_case('O', K)
    assert len(f['xs']) == P.FORWARD_N == 23 and f['theta'].shape == (9, K)
    assert P.class_f_holds(f)
    assert set(P.MODERATE.view(np.int64).tolist()) <= set(f['xs'].view(np.int64).tolist())
    assert set(P.LADDER.view(np.int64).tolist()) <= set(o['xs'].view(np.int64).tolist())
    if K >= 2:
        assert P.class_o_holds(o)
    zeros = np.concatenate([f['mock'][-2:].ravel(), o['mock'][-2:].ravel()])
    assert np.all(zeros == 0.0) and not np.all(np.signbit(zeros))
    if K % 2:                                            # a -0.0 result is in play
        assert np.any(np.signbit(zeros))


def test_stride_case_is_finite_and_large():
    s = P.stride_case()
    assert s['mock'].shape == (2, 65836) and np.all(np.isfinite(s['mock']))
    assert np.any(np.isnan(s['ys'])) and np.any(np.isinf(s['ys']))


# ---------------------------------------------------------------------------
# the zero-padded recurrence is polyval
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('K', P.K_LIST)
def test_padded_horner_restated_in_numpy_is_polyval(K):
    """Horner<KMAX> with zero padding, emulated: POLYVAL's bits on classes F, O and X, the sign of
    zero and the NaN pattern at x = +-inf included -- the device run is expected to pass."""
    be = P.KernelRestated()
    P.check_forward(be, P.forward_case('F', K), 'F K=%d' % K)
    P.check_forward(be, P.forward_case('O', K), 'O K=%d' % K)
    P.check_forward_spoiled(be, P.forward_case('F', K), 'K=%d' % K)


# ---------------------------------------------------------------------------
# the bounds contain numpy
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('N', P.N_LIST)
def test_logp_bound_contains_numpy(N):
    worst = {}
    for cls, small in (('F', False), ('F', True), ('O', False)):
        cs = P.case(cls, 5, N, 70, small_ys=small)
        w, held = P.check_epilogue(NP, cs, '%s N=%d' % (cls, N))
        worst[cls + ('s' if small else '')] = max(w.values())
        assert held > 0 or cls == 'O'
    print('N = %5d: numpy / logp_bound  F %.3f  F small ys %.3f  O %.3f' % (N, worst['F'], worst['Fs'], worst['O']))


def test_tau_scaled_underflow_allowance_is_needed_and_enough():
    """numpy on a chi^2 of 3 * 2^-1074 (halved: 1.5 quanta, rounds to 2) times tau = 1e300, against
    exact arithmetic ON THAT chi^2: 2.5e-24 off -- far outside a flat allowance of 2 quanta, inside
    TINY (tau / 2 + 1).  Against chi2_f = -2 lp(1) (what the device tests use) the halving is not
    seen at all: the value is within the rounding terms alone."""
    M = P.mp()
    for N in (0, 1, 9):
        for odd in (1.0, 3.0, 5.0, 7.0, 1001.0):
            chi2, tau = odd * P.TINY, 1e300
            got = float(P.ref_logp(np.array([chi2]), tau, N)[0])
            E, bound = P.exact_logp(chi2, tau, N)
            err = abs(M.mpf(got) - E)
            assert err <= bound, (N, odd)
            chi2_f = -2.0 * float(P.ref_logp(np.array([chi2]), 1.0, N)[0])
            assert chi2_f != chi2 and abs(chi2_f - chi2) == P.TINY
            E_f, bound_f = P.exact_logp(chi2_f, tau, N)
            rounding_only = bound_f - M.mpf(P.TINY) * (M.mpf(tau) / 2 + 1)
            assert abs(M.mpf(got) - E_f) <= rounding_only + M.mpf(P.TINY) / 2
            if N == 0:
                flat = bound - M.mpf(P.TINY) * (M.mpf(tau) / 2 + 1) + 2 * M.mpf(P.TINY)
                assert err > 1e10 * flat
                assert float(err / bound) > 0.99
                print('chi2 = %d quanta, tau = 1e300, N = 0: numpy is %s from exact, %.6f of logp_bound'
                      % (odd, M.nstr(err, 4), float(err / bound)))


def test_gamma_bound_contains_numpy():
    worst = 0.0
    for shape, rate in P.GAMMA_PARAMS:
        for C in (1, 257):
            for tau in P.gamma_taus(C):
                worst = max(worst, P.check_gamma_logp(NP, tau, shape, rate, 'C=%d' % C))
    print('numpy / gamma_bound: %.3f' % worst)
    # 0 * (-inf) at shape = 1 is numpy's NaN, and it is held as such
    assert np.isnan(P.ref_gamma_logp(np.array([0.0]), 1.0, 0.2)[0])


@pytest.mark.parametrize('N', [n for n in P.N_LIST if n >= 1])
def test_logp_bound_is_below_the_old_allowance(N):
    """The allowance it replaces: 1e-13 times the largest |lp| of the batch (rel_close).  Per
    launch of the epilogue grid on class F, the largest bound of a chain against that allowance."""
    cs = P.case('F', 5, N, 70)
    chi2 = P.ref_chi2(cs['mock'], cs['ys'])
    scalars, vectors = P.tau_sets(70)
    least = P.INF
    for tau in scalars + vectors:
        t = np.broadcast_to(np.asarray(tau, dtype=np.float64), chi2.shape)
        lp = P.ref_logp(chi2, t, N)
        ok = (t > 0) & np.isfinite(t) & np.isfinite(lp)
        if not ok.any():
            continue
        old = 1e-13 * max(np.abs(lp[ok]).max(), 1e-300)
        new = max(float(P.logp_bound(chi2[c], t[c], N)) for c in np.flatnonzero(ok))
        assert new <= old, (N, tau, new, old)
        least = min(least, old / new)
    print('N = %5d: old allowance / largest logp_bound of the launch >= %.0f' % (N, least))
    assert least >= 1.0


# ---------------------------------------------------------------------------
# mutations
# ---------------------------------------------------------------------------
def _fails(fn, *a, **k):
    try:
        fn(*a, **k)
    except AssertionError:
        return True
    return False


def test_folded_zero_product_is_caught():
    """Horner with x * 0.0 folded to 0, visible where an instantiation is exactly full (a padded
    one meets 0 * x in its padding steps anyway): class X catches it there (x = +-inf must give
    NaN in every chain), class O where a -0.0 leading coefficient meets a negative x."""
    table = []
    for K in P.K_LIST:
        be = P.FoldedHorner()
        x = _fails(P.check_forward_spoiled, be, P.forward_case('F', K))
        o = _fails(P.check_forward, be, P.forward_case('O', K))
        table.append((K, x, o))
        assert (x or o) == (K in P.KMAXES), (K, x, o)
    print('x * 0.0 folded: K -> caught on class X / class O: %s'
          % ', '.join('%d %s/%s' % (K, 'y' if x else 'n', 'y' if o else 'n') for K, x, o in table))
    assert any(o for _, _, o in table)


def test_padding_with_the_next_chain_is_caught():
    for K in P.K_LIST:
        be = P.PadsWithNextChain()
        caught = _fails(P.check_forward, be, P.forward_case('F', K))
        assert caught == (K not in P.KMAXES), K         # an instantiation exactly full has no padding
    print('padding from the next chain: caught at every K of %s'
          % (tuple(K for K in P.K_LIST if K not in P.KMAXES),))


def _old_rel_close(got, want, rtol=1e-13):
    scale = np.abs(want).max() if want.size else 1.0
    return np.abs(got - want).max() <= rtol * max(scale, 1e-300)


def test_sloppy_log_passes_the_old_check_and_leaves_the_bound():
    """A log with a relative error of 1e-13: inside rel_close(1e-13) on the old test's precisions
    (uniform in [0.5, 4] and 2.5), outside logp_bound -- by the printed factor."""
    be = P.SloppyLog()
    worst = 0.0
    for N in (9, 300, 8193):
        cs = P.case('F', 5, N, 70)
        chi2 = P.ref_chi2(cs['mock'], cs['ys'])
        taus = np.random.RandomState(1).uniform(0.5, 4.0, size=70)
        for tau in (2.5, taus):
            got, want = be.logp_routes(cs, tau)['poly_gauss_logp'], P.ref_logp(chi2, tau, N)
            assert _old_rel_close(got, want)
            t = np.broadcast_to(tau, chi2.shape)
            for c in range(70):
                E, bound = P.exact_logp(chi2[c], t[c], N)
                worst = max(worst, P.fraction(got[c], E, bound))
        assert _fails(P.check_epilogue, be, cs, scalars=[2.5], vectors=[taus])
        assert _fails(P.check_epilogue, be, cs)
    print('log off by 1e-13: passes rel_close(1e-13), reaches %.0f times logp_bound' % worst)
    assert worst > 50.0


@pytest.mark.parametrize('N', [n for n in P.N_LIST if n >= 1])
def test_one_datum_short_leaves_the_bound(N):
    assert _fails(P.check_epilogue, P.OneDatumShort(), P.case('F', 5, N, 9))
    assert not _fails(P.check_epilogue, NP, P.case('F', 5, N, 9))


@pytest.mark.parametrize('N', [n for n in P.N_LIST if n >= 1])
def test_a_wrong_weighted_reduction_is_caught(N):
    """The weighted route is compared on finite, distinct numbers (class F), so (c) rejects a
    reduction that forgets the leaf's tail (every N that has one), divides by the neighbour's
    weight (N >= 2) or adds the terms up in another order (once the pairwise tree has more than
    one leaf): at K = 1 and K = 5 with 9 and 70 chains in every case; at the larger K a few data
    with |x| > 1 dominate the sum and a small datum may leave no trace, so there the mutant may
    pass a case, and never fails where it does the right thing.  With one weight at an edge
    numpy still passes."""
    for K in P.CHI_K:
        for C in P.C_LIST:
            cs = P.case('F', K, N, C)
            wchi = P.ref_chi2(cs['mock'], cs['ys'], cs['weights'])
            assert np.all(np.isfinite(wchi)) and (C < 9 or P.class_f_holds(cs))
            # (mutant, where it differs from numpy at all, where it must be caught); from 8 data
            # on numpy adds eight interleaved partial sums, so a running sum is another order
            for mutant, wrong, must in ((P.WeightedTailDropped(), N % 8 != 0, N % 8 != 0),
                                        (P.WrongWeight(), N >= 2, N >= 2),
                                        (P.WeightedOtherOrder(), N >= 8, N >= 129)):
                caught = _fails(P.check_chi2_unit, mutant, cs)
                assert not caught or wrong, (type(mutant).__name__, K, N, C)
                if K <= 5 and C >= 9:
                    assert caught or not must, (type(mutant).__name__, K, N, C)
    cs = P.case('F', 5, N, 9)
    P.check_weight_edges(NP, cs)
    assert _fails(P.check_weight_edges, P.WrongWeight(), cs) == (N >= 2)
    kinds = set()
    for j, value in enumerate(P.WEIGHT_EDGES):              # the edges do leave the finite range
        x = P.spoil(cs, 'weights', (j * 5 + N // 2) % N, value)
        r = P.ref_chi2(x['mock'], x['ys'], x['weights'])
        kinds |= set('nan' if np.isnan(v) else '+inf' if v == P.INF else '-inf' if v == -P.INF else 'finite' for v in r)
    assert kinds == {'nan', '+inf', '-inf', 'finite'}


@pytest.mark.parametrize('N', P.SHARED_N)
def test_a_leaking_reduction_is_caught(N):
    cs = P.case('F', 5, N, 9)
    assert _fails(P.check_containment, P.LeakyReduction(), cs)
    P.check_containment(NP, cs)
    P.check_bad_datum(NP, cs)
    P.check_chi2_unit(NP, cs)
