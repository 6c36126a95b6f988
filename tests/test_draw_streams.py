"""The host restatement of the draw streams (tests/draw_streams.py) draws from the
right distributions -- so that "device == restatement" (tests/test_gpu_draw_streams.py)
means something.  No GPU, no library call.

Seeds and sizes are fixed, so every statistical condition below is deterministic; the
level is one for the whole file: p > 1e-3, |z| < 3.29 (the same two-sided level).  The
seeds were taken as written (the first tried), the achieved statistics are printed.
"""
import functools

import numpy as np
import pytest
from scipy import stats

import draw_streams as ds

P_MIN = 1e-3
Z_MAX = 3.29
N_ZIG = 1 << 24


def test_philox_restatements_meet_the_known_answers():
    """Random123's published vectors for philox4x32-10 (those of test_native_abi.py),
    scalar and vectorised."""
    kat = [([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
           ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
           ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
            [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]
    for ctr, key, want in kat:
        assert ds.philox4x32_10(ctr, key) == want
        got = ds.philox_v(*[np.array([c, c], dtype=np.uint64) for c in ctr], key[0], key[1])
        assert [int(g[1]) for g in got] == want


def test_xoshiro_scalar_and_vector_forms_agree():
    """... and meet xoshiro128++'s defining recurrence on a hand-checkable state."""
    g = ds.Xo128([1, 2, 3, 4])
    # rotl(1 + 4, 7) + 1 = 641; then s = [7, 0, 1026, 12288] (Blackman & Vigna's update)
    assert g.next() == 641 and g.s == [7, 0, 1026, 6 << 11]
    streams = np.array([0, 1, (1 << 40) + 5, ds.BIG_U_STREAM + 3], dtype=np.int64)
    v = ds.XoV(streams, ds.SEED, (1 << 63) + 9)
    s = [ds.Xo128.seeded(int(k), ds.SEED, (1 << 63) + 9) for k in streams]
    for _ in range(50):
        assert [int(x) for x in v.next()] == [g.next() for g in s]
    mask = np.array([True, False, True, False])
    before = [list(g.s) for g in s]
    out = v.next(mask)
    for k, g in enumerate(s):
        assert int(out[k]) == g.next()
        assert [int(a[k]) for a in v.s] == (g.s if mask[k] else before[k])


def test_ziggurat_tables_in_mpmath():
    """Equal layer areas, the base layer (strip + tail) of the same area, X[0] = V / f(R),
    monotone edges down to 0, ZIG_RATIO[i] == X[i+1] / X[i] exactly, ZIG_TAIL_R == X[1].
    The table holds doubles, so its areas agree only to the rounding of its entries: an
    edge near x = 1 moved by half an ulp changes a layer's area v = 4.9e-4 by
    x f(x) u / v = 1.4e-13 relative, and each edge comes from the one before it, so at
    worst the 1024 errors add up: 1.4e-10.  The bound is 2e-10 (a wrong digit in any entry
    is eight decades above it)."""
    t = ds.check_tables()
    print(t)
    assert t['area_spread'] < 2e-10 and t['base_vs_layers'] < 2e-10 and t['x0_vs_base'] < 2e-10
    assert t['monotone'] and t['ratio_exact'] and t['tail_r']


@functools.lru_cache(maxsize=None)
def philox_zig():
    return ds.zig_stream(ds.SEED + 100, ds.ZIG_OFF - 100, 0, N_ZIG, trace=True)


@functools.lru_cache(maxsize=None)
def xoshiro_zig():
    return ds.fused_streams(1, N_ZIG // 8, 8, ds.SEED + 101, 77, trace=True)[0]


def test_slow_path_census():
    """The census of the issue's prototype: 0.43 % of the candidates leave the fast path
    and about 5e-5 reach the tail -- binomial, at the file's level."""
    for name, d in (('philox', philox_zig()), ('xoshiro', xoshiro_zig())):
        c = d.counts()
        slow = N_ZIG - c['fast']
        print(name, c, 'marginal decisions', d.info['marginal_decisions'])
        # exact probabilities: a candidate is slow unless |u| < X[i+1] / X[i]; tail = base
        # layer beyond R, i.e. the mass of the density beyond R
        p_slow = float(np.mean(1.0 - ds.ZR))
        p_tail = 2 * stats.norm.sf(ds.TAIL_R)
        for got, p in ((slow, p_slow), (c['tail'], p_tail)):
            z = (got - N_ZIG * p) / np.sqrt(N_ZIG * p * (1 - p))
            print('  count %d expected %.1f z %.2f' % (got, N_ZIG * p, z))
            assert abs(z) < Z_MAX
        assert d.info['marginal_decisions'] == 0 and not d.marginal.any()


def _wedge_definition(trace):
    """accept iff y < f(x) with y uniform between f(X[i]) and f(X[i+1]): the wedge rule
    as Marsaglia & Tsang define it, in mpmath, NOT in the divided form the code uses."""
    import mpmath as mp
    mp.mp.dps = 50
    X = [mp.mpf(float(v)) for v in ds.ZX]
    F = [mp.exp(-x * x / 2) for x in X]
    out = []
    for x, layer, U, _ in trace:
        y = F[layer + 1] + mp.mpf(U) * (F[layer] - F[layer + 1])
        out.append(bool(y < mp.exp(-mp.mpf(x) ** 2 / 2)))
    return out


@pytest.mark.parametrize('stream', [philox_zig, xoshiro_zig])
def test_wedge_rule_against_its_definition(stream):
    trace = stream().info['wedge_trace']
    assert len(trace) > 60000
    want = _wedge_definition(trace)
    wrong = [k for k, (t, w) in enumerate(zip(trace, want)) if t[3] != w]
    assert not wrong, [trace[k] for k in wrong[:5]]
    # ... and the accepted count against the sum of the exact acceptance probabilities
    x, layer, _, acc = [np.array(c) for c in zip(*trace)]
    f = lambda v: np.exp(-0.5 * v * v)                                      # noqa: E731
    p = np.clip((f(x) - f(ds.ZX[layer])) / (f(ds.ZX[layer + 1]) - f(ds.ZX[layer])), 0.0, 1.0)
    z = (acc.sum() - p.sum()) / np.sqrt(np.sum(p * (1 - p)))
    print('wedge tests %d accepted %d expected %.1f z %.2f' % (len(trace), acc.sum(), p.sum(), z))
    assert abs(z) < Z_MAX


@pytest.mark.parametrize('stream', [philox_zig, xoshiro_zig])
def test_conditional_distributions_of_the_ziggurat(stream):
    d = stream()
    z = d.ref.ravel()
    path = d.path.ravel()
    tail = np.abs(z[path == ds.TAIL]) - ds.TAIL_R
    assert tail.size > 700 and (tail > 0).all()
    sfr = stats.norm.sf(ds.TAIL_R)
    ks = stats.kstest(tail, lambda t: 1.0 - stats.norm.sf(ds.TAIL_R + t) / sfr)
    print('tail draws %d KS p %.3f; negative %d' % (tail.size, ks.pvalue, np.sum(z[path == ds.TAIL] < 0)))
    assert ks.pvalue > P_MIN
    zs = (np.sum(z[path == ds.TAIL] < 0) - 0.5 * tail.size) / np.sqrt(0.25 * tail.size)
    assert abs(zs) < Z_MAX
    # the whole stream
    ks = stats.kstest(z, 'norm')
    print('whole stream KS D %.2e p %.3f' % (ks.statistic, ks.pvalue))
    assert ks.pvalue > P_MIN
    # the wedge-accepted and redrawn elements sit inside their layers
    assert np.abs(z[path != ds.TAIL]).max() < ds.TAIL_R


GAMMA_N = 200000


@pytest.mark.parametrize('shape', ds.GAMMA_SHAPES)
def test_gamma_stream_distribution(shape):
    d = ds.gamma_stream(shape, ds.SEED + 200, 1 << 40, 12345, GAMMA_N)
    ks = stats.kstest(d.ref, stats.gamma(shape).cdf)
    hist = np.bincount(d.info['attempts'])
    print('shape %g KS p %.3f attempts %s t<=0 %d' % (shape, ks.pvalue, hist[:6], d.info['t_retries']))
    assert ks.pvalue > P_MIN and (d.ref > 0).all() and d.info['exhausted'] == 0
    assert d.info['marginal_decisions'] == 0
    if shape == 1.0:
        assert hist[2:].sum() > 0 and d.info['t_retries'] > 0
    if shape >= 1.0:
        same = ds.gamma_stream(shape, ds.SEED + 200, 1 << 40, 12345, 4096, small=False)
        assert np.array_equal(same.ref, d.ref[:4096]) and np.array_equal(same.bound, d.bound[:4096])
    # a window of the stream is the stream
    w = ds.gamma_stream(shape, ds.SEED + 200, 1 << 40, 12345 + 777, 100)
    assert np.array_equal(w.ref, d.ref[777:877])


def test_tiny_shape_underflows_only_where_it_must():
    """shape = 0.001: U**1000 leaves the double range for about half the draws.  An exact
    0 may appear only where the mpmath value rounds to 0 (below half the smallest
    subnormal), and nowhere else."""
    import mpmath as mp
    mp.mp.dps = 50
    shape, n = 0.001, 4000
    d = ds.gamma_stream(shape, ds.SEED + 300, 5, 0, n)
    half = mp.mpf(2) ** -1075
    e = mp.mpf(1.0 / shape)
    zeros = 0
    for k in range(n):
        exact = mp.mpf(float(d.info['before_pow'][k])) * mp.mpf(float(d.info['pow_base'][k])) ** e
        assert (d.ref[k] == 0.0) == bool(exact <= half), (k, d.ref[k], exact)
        zeros += d.ref[k] == 0.0
    print('zeros %d of %d' % (zeros, n))
    assert 0.3 * n < zeros < 0.7 * n


def test_windows_are_slices_of_the_stream():
    seed, off = ds.SEED + 400, ds.ZIG_OFF - 400
    for f in (ds.uniform_stream, ds.box_muller_stream, ds.zig_stream):
        whole = f(seed, off, 0, 20001)
        for e0, n in ((1, 1), (12345, 1001), (7000, 2)):
            assert np.array_equal(f(seed, off, e0, n).ref, whole.ref[e0:e0 + n])
    u = ds.uniform_stream(seed, off, 0, 1000).ref
    assert 0.0 <= u.min() and u.max() < 1.0


def test_the_gpu_cases_meet_no_marginal_decision():
    """What tests/test_gpu_draw_streams.py compares has no marginal element at all, and
    the paths it asks for are there."""
    total = 0
    for seed, off, e0, n, _ in ds.ZIG_CASES:
        d = ds.zig_stream(seed, off, e0, n)
        total += d.info['marginal_decisions'] + int(d.marginal.sum())
    for case in ds.GAMMA_CASES:
        d = ds.gamma_stream(*case)
        total += d.info['marginal_decisions'] + int(d.marginal.sum())
    for case in ds.FUSED_CASES:
        d = ds.fused_streams(*case)[0]
        total += d.info['marginal_decisions'] + int(d.marginal.sum())
    for case in ds.BIG_CASES:
        d = ds.big_streams(*case)[0]
        total += d.info['marginal_decisions'] + int(d.marginal.sum())
    assert total == 0


def test_fused_layouts():
    """Slots per lane and group size of the persistent kernel's instantiations, and the
    leaves of ragged trees (numpy's pairwise summation splits at n/2 rounded down to 8)."""
    assert ds.fused_layout(8) == (0, 1, 1) and ds.fused_layout(64) == (0, 8, 8)
    assert ds.fused_layout(33) == (0, 8, 8) and ds.fused_layout(96) == (0, 12, 4)
    assert ds.fused_layout(1024) == (3, 16, 8) and ds.fused_layout(2048) == (4, 16, 8)
    assert ds.fused_layout(200) == (1, 16, 8)
    assert ds.leaves(200, 1) == [(0, 0, 96), (1, 96, 104)]
    assert ds.leaves(33, 0) == [(0, 0, 33)]
    lv = ds.leaves(777, ds.tree_height(777))
    assert sum(ln for _, _, ln in lv) == 777 and all(ln <= 128 for _, _, ln in lv)
    assert [o for _, o, _ in lv] == list(np.cumsum([0] + [ln for _, _, ln in lv[:-1]]))


def test_the_bounds_see_each_injected_defect():
    seen = ds.self_test()
    print(seen)
    for name in ('zig: fast value + 64 ulp', 'zig: tail value + 64 ulp', 'zig: wedge flipped',
                 'zig: tail sign flipped', 'box-muller: + 64 ulp', 'gamma 0.5: wrong offset',
                 'gamma 2.5: wrong offset', 'gamma 2.5: + 64 ulp', 'fused: wedge flipped',
                 'fused: tail sign flipped'):
        assert seen[name] > 0, name
    for name in ('zig: sound', 'box-muller: sound', 'gamma 0.5: sound', 'gamma 2.5: sound', 'fused: sound'):
        assert seen[name] == 0, name
