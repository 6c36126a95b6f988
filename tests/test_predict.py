"""``tests/predict_ref.py`` held honest without a GPU: the numpy restatement of the predictive
density (``oracle/ref_example.py:predict``) stays inside ``density_bound`` of the exact value on
every input builder, three deliberately wrong restatements do not, the non-finite rules of
``exact_density`` are numpy's, and ``kernel_plan`` is the library's own cut of the samples
wherever the library answers without a device."""
import numpy as np
import pytest

import predict_ref as P
from binf_amd import _native
from oracle import ref_example as E

S_CPU = (1, 5, 17, 300, 2000)
NX, NY = 3, 5
POINTS = ((0, 0), (2, 4), (1, 2))


def numpy_density(col, y, tau):
    """oracle/ref_example.py:predict with the mock column handed in as one-coefficient samples."""
    with np.errstate(all='ignore'):
        return float(E.predict(0.0, y, np.asarray(col)[:, None], tau, polynomial=lambda x, c: c[0]))


def cases(name, sizes=S_CPU):
    """(label, mock column, y, precision, chunk) over the sizes and points of this module."""
    for S in sizes:
        variants = [dict(carrier=c) for c in P.one_dominant_carriers(S)] if name == 'one_dominant' else [dict()]
        for kw in variants:
            mock, tau, ys = P.BUILDERS[name](S, NX, NY, **kw)
            for i, j in POINTS:
                yield '%s S=%d %s (%d,%d)' % (name, S, kw, i, j), mock[:, i], ys[i, j], tau, max(1, (S + 3) // 4)


@pytest.mark.parametrize('name', sorted(P.BUILDERS))
def test_numpy_restatement_is_inside_the_bound(name):
    """|numpy - exact| <= density_bound(depth = S): the bound is not vacuous (it is a few ulps of
    the density, see the printed figures) and the reference alone stays inside it."""
    worst, kinds = 0.0, set()
    for label, col, y, tau, _ in cases(name):
        ex = P.exact_density(col, y, tau)
        got = numpy_density(col, y, tau)
        ratio = P.error_over_bound(got, ex, depth=len(tau))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (label, got, float(ex['density']), ratio)
        assert got >= 0.0
        if P.below_half_quantum(ex):
            assert got in (0.0, P.Q), (label, got)
        kinds.add('zero' if got == 0.0 else 'subnormal' if got < 2.0 ** -1022 else 'normal')
        # a bound worth the name: at its widest (the far tail at S = 2000) it is u (6 a + |lse| + S)
        # with a, |lse| ~ 750 -- 8e-13 of the density, under the flat 1e-12 it replaces
        if got >= 2.0 ** -1000:
            assert float(P.density_bound(ex, depth=len(tau)) / ex['density']) <= 1e-12, label
    print('%s: worst |numpy - exact| / bound = %.3f' % (name, worst))
    if name == 'far_tail':
        assert kinds == {'zero', 'subnormal', 'normal'}, kinds


def test_grid_bound_is_density_bound_for_a_whole_grid():
    """The vectorised bound the GPU tests lay over every point is the derived one (to 1e-9 of
    itself: it takes its weights from doubles), and the plain mean of the Gaussian densities is
    inside ITS bound of the exact value."""
    assert 0.5 * np.log(2.0 * np.pi) == P.HALF_LOG_2PI          # the restatement's constant
    import mpmath
    for name, kw in (('mild', {}), ('one_dominant', dict(carrier=16)), ('near_equal_chunk_maxima', {})):
        for S, depth, joined in ((1, 16, False), (17, 17, False), (300, 34, True)):
            mock, tau, ys = P.BUILDERS[name](S, NX, NY, **kw)
            p, bound, bound_mean = P.grid_bound(mock, tau, ys, depth, joined)
            mean = P.mean_of_densities(mock, tau, ys)
            for i, j in POINTS:
                ex = P.exact_density(mock[:, i], ys[i, j], tau)
                want = float(P.density_bound(ex, depth, joined))
                assert abs(bound[i, j] - want) <= 1e-9 * want, (name, S, i, j)
                assert abs(mpmath.mpf(float(mean[i, j])) - ex['density']) <= bound_mean[i, j], (name, S, i, j)


# ---------------------------------------------------------------------------
# controls: wrong restatements
# ---------------------------------------------------------------------------
def lse_density(f, S):
    with np.errstate(all='ignore'):
        M = f.max()
        return float(np.exp(np.log(np.exp(f - M).sum()) + M) / S)


def chunk_pairs(f, chunk):
    with np.errstate(all='ignore'):
        return [(f[lo:lo + chunk].max(), np.exp(f[lo:lo + chunk] - f[lo:lo + chunk].max()).sum())
                for lo in range(0, f.shape[0], chunk)]


def joined_density(f, chunk, S, back=None):
    """The chunked path as csrc/predict.hip joins it; ``back``: the maximum added back."""
    pairs = chunk_pairs(f, chunk)
    with np.errstate(all='ignore'):
        M = max(m for m, _ in pairs)
        t = sum(s * np.exp(m - M) for m, s in pairs)
        return float(np.exp(np.log(t) + (M if back is None else back(pairs))) / S)


def drops_the_tail(col, y, tau, chunk):
    """WRONG: the last S % 16 samples never reach the sum (a lane loop that stops at the last
    full round).  Caught by ``mild`` (S = 17, 300: 8e12 times the bound at worst) and, where
    the carrier is the last sample, by ``one_dominant`` (the density comes out 0: 3e14 times
    the bound); every other builder is above 1e9 times as well."""
    f = P.terms_f64(col, y, tau)
    n = f.shape[0] - f.shape[0] % 16
    return lse_density(f[:n], f.shape[0]) if n else float('nan')


def joins_with_the_first_maximum(col, y, tau, chunk):
    """WRONG: the chunk sums are scaled to the global maximum, but the FIRST chunk's maximum is
    added back.  Caught by ``mild`` (1e14 times the bound) and by ``one_dominant`` with the
    carrier outside the first chunk (the density comes out 0: 3e14 times); NOT by
    ``near_equal_chunk_maxima`` (0.04 of the bound), where the two maxima are an ulp apart and
    the slip is one rounding of the log-sum -- inside any honest bound.  That builder is there
    for the kernel's join, where close maxima make every chunk's scale factor matter."""
    return joined_density(P.terms_f64(col, y, tau), chunk, len(tau), back=lambda pairs: pairs[0][0])


def divides_by_the_chunk(col, y, tau, chunk):
    """WRONG: the mean is taken over the chunk length, not S.  Caught by every builder at every
    S > 1 (a factor ~4 on the density: 5e12 times the bound in the far tail, where the bound
    is widest, to 7e14 times on ``one_dominant``)."""
    return joined_density(P.terms_f64(col, y, tau), chunk, chunk)


def worst_by_builder(wrong, sizes):
    out = {}
    for name in sorted(P.BUILDERS):
        w = 0.0
        for label, col, y, tau, chunk in cases(name, sizes):
            ex = P.exact_density(col, y, tau)
            w = max(w, P.error_over_bound(wrong(col, y, tau, chunk), ex, depth=len(tau), joined=True))
        out[name] = w
    return out


def test_the_chunked_join_written_here_is_inside_the_bound():
    """The controls below differ from THIS in one slip each: it must be inside the bound itself."""
    w = worst_by_builder(lambda col, y, tau, chunk: joined_density(P.terms_f64(col, y, tau), chunk, len(tau)),
                         (5, 17, 300))
    print('right join, worst error / bound by builder:', {k: round(v, 3) for k, v in w.items()})
    assert max(w.values()) <= 1.0, w


@pytest.mark.parametrize('wrong,caught_by', [(drops_the_tail, ('mild', 'one_dominant')),
                                             (joins_with_the_first_maximum, ('mild', 'one_dominant')),
                                             (divides_by_the_chunk, tuple(sorted(P.BUILDERS)))],
                         ids=lambda v: getattr(v, '__name__', None))
def test_a_wrong_restatement_leaves_the_bound(wrong, caught_by):
    w = worst_by_builder(wrong, (17, 300))
    print('%s, worst error / bound by builder:' % wrong.__name__, {k: '%.3g' % v for k, v in w.items()})
    for name in caught_by:
        assert w[name] > 1.0, (name, w)


# ---------------------------------------------------------------------------
# non-finite inputs
# ---------------------------------------------------------------------------
def test_non_finite_rules_are_numpys():
    """NaN exactly where oracle/ref_example.py:predict is NaN, on every point of the poisoned
    grids the GPU tests use; where both are finite the restatement is inside the bound."""
    n = 0
    for label, mock, tau, ys in P.nonfinite_cases(17, 9, S=20):
        for i, j in P.sample_points(17, 9, 12) + P.poisoned_points(label, 17, 9):
            ex = P.exact_density(mock[:, i], ys[i, j], tau)
            got = numpy_density(mock[:, i], ys[i, j], tau)
            assert (got != got) == (ex['density'] != ex['density']), (label, i, j, got)
            assert (got != got) == bool(P.nonfinite_nan_mask(label, 17, 9)[i, j]), (label, i, j, got)
            if got == got:
                assert P.error_over_bound(got, ex, depth=20) <= 1.0, (label, i, j)
            n += got != got
    assert n > 0


# ---------------------------------------------------------------------------
# the cut of the samples
# ---------------------------------------------------------------------------
GRIDS = [(1, 1), (16, 8), (17, 8), (16, 9), (17, 9), (33, 17), (3, 5), (100, 150),
         (1, 8 * 1023), (1, 8 * 1023 + 1), (16 * 32, 8 * 32), (16 * 32, 8 * 31), (16 * 16, 8 * 4), (16 * 16 + 1, 8 * 4),
         (1, 524280), (524280, 1)]
SIZES = [1, 255, 256, 511, 512, 513, 767, 768, 1023, 1024, 4096, 16383, 16384, 16385, 16640, 51200]


def test_kernel_plan_is_the_librarys_cut():
    L = _native.lib()
    seen = set()
    for nx, ny in GRIDS:
        for S in SIZES:
            plan = P.kernel_plan(S, nx, ny)
            assert plan['need'] == (0 if plan['ns'] == 1 else plan['ns'] * nx * ny * 16)
            assert L.binf_predictive_density_workspace_bytes(S, nx, ny) == plan['need'], (S, nx, ny)
            assert 0 < plan['last'] <= plan['chunk'] and (plan['ns'] == 1 or plan['chunk'] >= 256)
            seen.add(plan['ns'])
    assert {1, 2, 3, 4, 64} <= seen
    table = {(511, 1, 1): (1, 511, 511), (512, 1, 1): (2, 256, 256), (513, 1, 1): (2, 257, 256),
             (1023, 17, 9): (3, 341, 341), (16384, 1, 1): (64, 256, 256), (16385, 1, 1): (64, 257, 194)}
    for (S, nx, ny), want in table.items():
        plan = P.kernel_plan(S, nx, ny)
        assert (plan['ns'], plan['chunk'], plan['last']) == want
    assert P.kernel_plan(511, 1, 1)['depth'] == 32 + 15 and P.kernel_plan(16385, 1, 1)['depth'] == 17 + 15 + 63
    assert L.binf_predictive_density_workspace_bytes(0, 1, 1) == 0
