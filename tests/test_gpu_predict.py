"""``binf_predictive_density_f64`` and its host mirror (``binf_amd/example/misc.py``:
``predict`` / ``predict_grid`` / ``prediction_tube``) against the numpy restatement of
``binf/example/misc.py:3-16`` and ``plots.py:8-27`` (``oracle/ref_example.py``, whose integrand
and tube post-processing are pinned by reference output -- tests/test_ref_predict.py).

Floating-point bar: 1e-12 relative on every density (the kernel sums the samples lane-strided,
not in numpy's pairwise order, and uses the device library's log / exp; measured ~1e-15), the
Horner values underneath are bit-identical; the 5 % / 95 % limits are grid values and must be
EQUAL.

The second half of the module holds the kernel to EXACT arithmetic instead: every density it
samples lies within ``predict_ref.density_bound`` of the mpmath value of the expression, a bound
derived from the kernel's order of operations (its docstring; the one assumption is that the
device library's exp / log are within an ulp) and held honest on the CPU by
tests/test_predict.py.  The calls go through the C ABI with ``out`` and the workspace between
sentinels.  Worst |device - exact| / bound of the module on an MI355X: 0.463 (``far_tail``,
S = 17, the 1 x 1 grid); by builder far_tail 0.463, wide_precision 0.305, mild 0.209,
near_equal_chunk_maxima 0.147, one_dominant 0.076; the chunked boundaries 0.079 at most, the
largest grid 0.251.  Each test prints its own."""
import ctypes

import numpy as np
import pytest
import torch

import predict_ref as P
from binf_amd import _native
from binf_amd.example import misc
from binf_amd.example.likelihood import POLYVAL
from binf_amd.samplers import BinfState
from conftest import golden_files, load_golden
from oracle import ref_example as E

pytestmark = pytest.mark.gpu

RTOL = 1e-12


def dev_t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device)


def close(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return np.all(np.abs(got - want) <= RTOL * np.abs(want))


@pytest.mark.parametrize('path', golden_files('ref_predict_'), ids=lambda p: p.split('ref_predict_')[-1][:-4])
def test_tube_and_points_against_the_restatement(device, path):
    g = load_golden(path)
    samples = (dev_t(g['coefficients'], device), dev_t(g['precisions'], device))
    t = misc.prediction_tube(samples, POLYVAL, g['predict_space'], g['ys_from'], g['ys_to'], int(g['n_ys']))
    assert np.array_equal(t.predicted_ys, g['predicted_ys'])
    assert close(t.probs, g['probs_in']) and t.probs.min() >= 0.0
    assert np.array_equal(t.lower, g['lower']) and np.array_equal(t.upper, g['upper'])
    assert close(t.cdfs, g['cdfs']) and close(t.prediction, g['prediction'])
    for x, y in zip(g['pts_x'], g['pts_y']):
        want = E.predict(x, y, g['coefficients'], g['precisions'])
        got = misc.predict(x, y, samples, POLYVAL)
        assert isinstance(got, float) and abs(got - want) <= RTOL * want


@pytest.mark.parametrize('S,K,nx,ny', [(1, 1, 1, 1), (5, 3, 1, 7), (16, 4, 16, 8), (17, 4, 17, 9),
                                       (257, 33, 33, 150), (3000, 4, 100, 31),
                                       # few points, many samples: the samples are cut into chunks
                                       (5000, 4, 3, 7), (511, 4, 1, 1), (512, 4, 1, 1), (20000, 4, 33, 17)])
def test_grid_shapes_against_the_restatement(device, S, K, nx, ny):
    rs = np.random.RandomState(S + nx)
    c = rs.standard_normal((S, K)) * 0.3
    tau = rs.gamma(4.0, 0.5, size=S)
    xs = rs.uniform(-1, 1, size=nx)
    ys = rs.standard_normal((nx, ny)) * 2
    got = misc.predict_grid(xs, ys, (dev_t(c, device), dev_t(tau, device)), POLYVAL).cpu().numpy()
    stride = max(1, (nx * ny) // 40)                 # the restatement loops in Python: a sample of the grid
    for flat in range(0, nx * ny, stride):
        i, j = divmod(flat, ny)
        want = E.predict(xs[i], ys[i, j], c, tau)
        assert abs(got[i, j] - want) <= RTOL * want, (i, j)
    # every point: the mean of the Gaussian densities (vectorised numpy, no log_sum_exp)
    m = np.array([[E.R.polyval(x, ci) for x in xs] for ci in c])                       # [S, nx]
    dens = np.sqrt(tau / (2 * np.pi))[:, None, None] * np.exp(-0.5 * tau[:, None, None] *
                                                              (m[:, :, None] - ys[None]) ** 2)
    assert np.all(np.abs(got - dens.mean(0)) <= 1e-11 * dens.mean(0) + 1e-300)


def test_states_of_a_sampling_loop_and_chain_batched_states(device):
    """``samples`` as the reference's loop collects them (a list of BinfState), one chain or a
    batch of chains per state: every chain of every state is one sample."""
    rs = np.random.RandomState(9)
    c = rs.standard_normal((12, 4)) * 0.2
    tau = rs.gamma(4.0, 0.5, size=12)
    single = [BinfState(dict(coefficients=dev_t(c[i], device), precision=float(tau[i]))) for i in range(12)]
    batched = [BinfState(dict(coefficients=dev_t(c[i:i + 4], device), precision=dev_t(tau[i:i + 4], device)))
               for i in (0, 4, 8)]
    want = E.predict(0.3, -0.1, c, tau)
    a, b = misc.predict(0.3, -0.1, single, POLYVAL), misc.predict(0.3, -0.1, batched, POLYVAL)
    assert a == b and abs(a - want) <= RTOL * want
    with pytest.raises(ValueError):
        misc.predict(0.3, -0.1, [], POLYVAL)
    with pytest.raises(ValueError):
        misc.predict_grid([0.0, 1.0], [[0.0]], single, POLYVAL)


def test_a_users_polynomial_callable_is_applied_as_given(device):
    rs = np.random.RandomState(10)
    c, tau = rs.standard_normal((50, 3)) * 0.2, rs.gamma(4.0, 0.5, size=50)
    calls = []

    def cubic_free(xs, coefficients):                 # c0 + c1 x + c2 x^2 through the library's Horner
        calls.append(tuple(coefficients.shape))
        return _native.poly_forward(coefficients, xs)

    xs, ys = np.linspace(-1, 1, 5), rs.standard_normal((5, 6))
    samples = (dev_t(c, device), dev_t(tau, device))
    got = misc.predict_grid(xs, ys, samples, cubic_free)
    assert calls == [(50, 3)] and torch.equal(got, misc.predict_grid(xs, ys, samples, POLYVAL))


def test_nan_and_inf_follow_numpy(device):
    c = np.zeros((4, 2))
    xs, ys = np.array([0.0, 1.0]), np.array([[0.0, 0.5], [1.0, -1.0]])
    with np.errstate(all='ignore'):
        for tau in ([1.0, -1.0, 2.0, 1.0],            # log of a negative precision: NaN everywhere
                    [0.0, 0.0, 0.0, 0.0],              # every term -inf: inf - inf = NaN, as numpy has it
                    [0.0, 1.0, 0.0, 4.0]):             # -inf terms drop out of the sum
            tau = np.array(tau)
            got = misc.predict_grid(xs, ys, (dev_t(c, device), dev_t(tau, device)), POLYVAL).cpu().numpy()
            want = np.array([[E.predict(xs[i], ys[i, j], c, tau) for j in range(2)] for i in range(2)])
            assert np.array_equal(np.isnan(got), np.isnan(want))
            ok = ~np.isnan(want)
            assert np.all(np.abs(got[ok] - want[ok]) <= RTOL * np.abs(want[ok]))
    # many samples on a small grid (chunks of samples joined by a second launch): a chunk whose
    # terms are all -inf drops out, all chunks -inf give NaN, one NaN term poisons the point
    S = 4000
    assert _native.lib().binf_predictive_density_workspace_bytes(S, 2, 2) > 0
    cs = np.zeros((S, 2))
    with np.errstate(all='ignore'):
        for tau in (np.where(np.arange(S) < 1500, 0.0, 2.0), np.zeros(S),
                    np.where(np.arange(S) == 3999, -1.0, 1.0), np.where(np.arange(S) % 2 == 0, 0.0, 3.0)):
            got = misc.predict_grid(xs, ys, (dev_t(cs, device), dev_t(tau, device)), POLYVAL).cpu().numpy()
            want = np.array([[E.predict(xs[i], ys[i, j], cs, tau) for j in range(2)] for i in range(2)])
            assert np.array_equal(np.isnan(got), np.isnan(want))
            ok = ~np.isnan(want)
            assert np.all(np.abs(got[ok] - want[ok]) <= RTOL * np.abs(want[ok]))
    # far tails underflow to 0 without NaN
    got = misc.predict_grid([0.0], [[1e6]], (dev_t(c, device), dev_t(np.ones(4), device)), POLYVAL)
    assert float(got[0, 0]) == 0.0


def test_c_abi_refusals(device):
    lib = _native.lib()
    mock = dev_t(np.zeros((4, 3)), device)
    tau = dev_t(np.ones(4), device)
    ys = dev_t(np.zeros((3, 5)), device)
    out = torch.empty((3, 5), dtype=torch.float64, device=device)
    h = 0.5 * np.log(2 * np.pi)
    args = lambda m, t, y, o, S=4, nx=3, ny=5, ws=None, wb=0: (m, t, y, o, S, nx, ny, h, ws, wb, None)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.binf_predictive_density_f64(*args(p(mock), p(tau), p(ys), p(out), S=0)) == _native.E_ARG
    assert lib.binf_predictive_density_f64(*args(None, p(tau), p(ys), p(out))) == _native.E_ARG
    assert lib.binf_predictive_density_f64(*args(p(mock), p(tau), p(ys), p(ys))) == _native.E_ALIAS
    assert lib.binf_predictive_density_f64(*args(p(mock), p(tau), p(ys), p(out), nx=0)) == 0
    assert lib.binf_predictive_density_f64(*args(p(mock), p(tau), p(ys), p(out))) == 0
    torch.cuda.synchronize()
    assert torch.all(out > 0)
    # many samples on a small grid need the workspace the library asks for
    S = 4096
    big, taus = dev_t(np.zeros((S, 3)), device), dev_t(np.ones(S), device)
    need = lib.binf_predictive_density_workspace_bytes(S, 3, 5)
    assert need > 0 and lib.binf_predictive_density_workspace_bytes(4, 3, 5) == 0
    ws = torch.empty(need // 8, dtype=torch.float64, device=device)
    assert lib.binf_predictive_density_f64(*args(p(big), p(taus), p(ys), p(out), S=S)) == _native.E_ARG
    assert lib.binf_predictive_density_f64(*args(p(big), p(taus), p(ys), p(out), S=S, ws=p(ws), wb=need - 8)) == _native.E_ARG
    assert lib.binf_predictive_density_f64(*args(p(big), p(taus), p(ys), p(out), S=S, ws=p(out), wb=need)) == _native.E_ALIAS
    assert lib.binf_predictive_density_f64(*args(p(big), p(taus), p(ys), p(out), S=S, ws=p(ws), wb=need)) == 0
    torch.cuda.synchronize()
    assert torch.all(out > 0)


# ---------------------------------------------------------------------------
# The kernel against EXACT arithmetic inside the derived bound of tests/predict_ref.py, through
# the C ABI, with ``out`` and the workspace between sentinels.
# ---------------------------------------------------------------------------
SENT = -7.25
worst_ratio = [0.0, '']           # largest |device - exact| / bound seen by this module's tests


def carve(a, device, before=0, after=0):
    """``a`` on the device inside a larger sentinel-filled buffer: (view, whole buffer).
    ``before`` doubles in front shift the view off 16-byte alignment when odd."""
    flat = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    whole = torch.full((before + flat.size + after,), SENT, dtype=torch.float64, device=device)
    view = whole[before:before + flat.size]
    view.copy_(torch.from_numpy(flat))
    return view, whole


def guards_intact(whole, before, n):
    w = whole.cpu().numpy()
    return bool(np.all(w[:before] == SENT) and np.all(w[before + n:] == SENT))


def abi_density(device, mock, tau, ys, rc_want=0, sync=True):
    """One call of binf_predictive_density_f64 on carved buffers: the densities [nx x ny] (or the
    untouched ``out``), guards and inputs checked.  The workspace is exactly ``need`` bytes."""
    L = _native.lib()
    S, nx = mock.shape
    ny = ys.shape[1]
    md, mw = carve(mock, device, 1, 1)
    td, tw = carve(tau, device, 1, 1)
    yd, yw = carve(ys, device, 3, 1)
    od, ow = carve(np.full(nx * ny, SENT), device, 3, 5)
    need = L.binf_predictive_density_workspace_bytes(S, nx, ny)
    assert need == P.kernel_plan(S, nx, ny)['need']
    wd, ww = carve(np.full(need // 8, SENT), device, 1, 7) if need else (None, None)
    kept = [w.clone() for w in (mw, tw, yw)]
    rc = L.binf_predictive_density_f64(md.data_ptr(), td.data_ptr(), yd.data_ptr(), od.data_ptr(), S, nx, ny,
                                       P.HALF_LOG_2PI, wd.data_ptr() if need else None, need,
                                       _native.stream_handle(device))
    assert rc == rc_want, _native.last_error()
    if sync:
        torch.cuda.synchronize()
    assert guards_intact(ow, 3, nx * ny) and (not need or guards_intact(ww, 1, need // 8))
    for w, k in zip((mw, tw, yw), kept):                          # the inputs are never written
        assert torch.equal(w.view(torch.int64), k.view(torch.int64))
    return od.cpu().numpy().reshape(nx, ny)


def hold_to_the_bound(got, mock, tau, ys, points, label):
    """Every (i, j) of ``points`` against exact arithmetic inside density_bound at the kernel's
    own depth; the worst error / bound."""
    S, nx = mock.shape
    plan = P.kernel_plan(S, nx, ys.shape[1])
    worst = 0.0
    for i, j in points:
        ex = P.exact_density(mock[:, i], ys[i, j], tau)
        g = float(got[i, j])
        if ex['density'] != ex['density']:
            assert g != g, (label, i, j, g)
            continue
        assert g == g and g >= 0.0 and not np.signbit(g), (label, i, j, g)
        ratio = P.error_over_bound(g, ex, plan['depth'], plan['joined'])
        assert ratio <= 1.0, (label, i, j, g, float(ex['density']), ratio)
        if P.below_half_quantum(ex):
            assert g in (0.0, P.Q), (label, i, j, g)
        worst = max(worst, ratio)
    if worst > worst_ratio[0]:
        worst_ratio[:] = [worst, label]
    return worst


def hold_every_point(got, mock, tau, ys, label):
    """Every point against the plain mean of the Gaussian densities (vectorised numpy): the two
    may differ by the sum of their derived bounds (predict_ref.grid_bound)."""
    plan = P.kernel_plan(mock.shape[0], mock.shape[1], ys.shape[1])
    _, bound, bound_mean = P.grid_bound(mock, tau, ys, plan['depth'], plan['joined'])
    diff = np.abs(got - P.mean_of_densities(mock, tau, ys))
    assert np.all(diff <= bound + bound_mean), (label, np.argmax(diff - bound - bound_mean))


EVERY_POINT = ('mild', 'one_dominant', 'near_equal_chunk_maxima')      # finite, normal densities
S_UNCHUNKED = (1, 15, 16, 17, 255, 511)
SHAPES = ((1, 1), (15, 7), (16, 8), (17, 9), (33, 17))


@pytest.mark.parametrize('name', sorted(P.BUILDERS))
def test_every_builder_is_inside_the_bound_on_both_sides_of_every_tile(device, name):
    worst, kinds = 0.0, set()
    for S in S_UNCHUNKED:
        for nx, ny in SHAPES:
            assert P.kernel_plan(S, nx, ny)['ns'] == 1
            # one_dominant: every carrier (each sample lane, the first, the last sample) at
            # the grid with partial tiles in both directions, the last sample everywhere
            variants = [dict()] if name != 'one_dominant' else \
                [dict(carrier=c) for c in (P.one_dominant_carriers(S) if (nx, ny) == (17, 9) else [S - 1])]
            for kw in variants:
                mock, tau, ys = P.BUILDERS[name](S, nx, ny, **kw)
                got = abi_density(device, mock, tau, ys)
                label = '%s S=%d %dx%d %s' % (name, S, nx, ny, kw)
                pts = P.sample_points(nx, ny, 4 if kw else 8)
                if name in EVERY_POINT:
                    hold_every_point(got, mock, tau, ys, label)
                else:
                    assert not np.any(np.isnan(got)) and np.all(got >= 0.0), label
                    edges = P.edge_points(mock, tau, ys)           # an exact 0, a subnormal, where there is one
                    kinds |= set(edges)
                    pts = pts[:6] + [p for p in edges.values() if p not in pts[:6]]
                worst = max(worst, hold_to_the_bound(got, mock, tau, ys, pts, label))
    if name == 'far_tail':
        assert kinds == {'zero', 'subnormal', 'normal'}, kinds
    print('%s: worst |device - exact| / bound = %.3f (module so far %.3f, %s)' % ((name, worst) + tuple(worst_ratio)))


CHUNK_TABLE = {(511, 1, 1): (1, 511, 511), (512, 1, 1): (2, 256, 256), (513, 1, 1): (2, 257, 256),
               (1023, 17, 9): (3, 341, 341), (16384, 1, 1): (64, 256, 256), (16385, 1, 1): (64, 257, 194)}


@pytest.mark.parametrize('S,nx,ny', sorted(CHUNK_TABLE))
def test_the_chunked_path_on_its_boundaries(device, S, nx, ny):
    """(ns, chunk, samples of the last chunk) as the table says; the carrier of one_dominant in
    the first chunk, at the start of the last chunk and at the last sample; chunk maxima an ulp
    or two apart."""
    plan = P.kernel_plan(S, nx, ny)
    assert (plan['ns'], plan['chunk'], plan['last']) == CHUNK_TABLE[(S, nx, ny)]
    worst = 0.0
    pts = P.sample_points(nx, ny, 6)
    for name, kw in [('one_dominant', dict(carrier=5)), ('one_dominant', dict(carrier=(plan['ns'] - 1) * plan['chunk'])),
                     ('one_dominant', dict(carrier=S - 1)), ('near_equal_chunk_maxima', dict())]:
        mock, tau, ys = P.BUILDERS[name](S, nx, ny, **kw)
        got = abi_density(device, mock, tau, ys)
        label = '%s S=%d %dx%d %s' % (name, S, nx, ny, kw)
        worst = max(worst, hold_to_the_bound(got, mock, tau, ys, pts, label))
        hold_every_point(got, mock, tau, ys, label)
    print('S=%d %dx%d: worst |device - exact| / bound = %.3f (module so far %.3f, %s)' % ((S, nx, ny, worst) + tuple(worst_ratio)))


def test_one_point_alone_and_inside_a_grid_that_fills_the_chip(device):
    """The same point through the chunked path (a 1 x 1 grid, S = 512: two chunks) and the
    unchunked one (1 x 8192 points: 1024 workgroups): each inside its bound of the exact value,
    so at most the sum of the two bounds apart."""
    import mpmath
    S, ny, j = 512, 8192, 4097
    mock, tau, ys = P.mild(S, 1, ny)
    alone, grid = P.kernel_plan(S, 1, 1), P.kernel_plan(S, 1, ny)
    assert alone['ns'] == 2 and grid['ns'] == 1
    a = abi_density(device, mock, tau, ys[:, j:j + 1])
    b = abi_density(device, mock, tau, ys)
    ex = P.exact_density(mock[:, 0], ys[0, j], tau)
    wa = hold_to_the_bound(a, mock, tau, ys[:, j:j + 1], [(0, 0)], 'alone')
    wb = hold_to_the_bound(b, mock, tau, ys, [(0, j), (0, 0), (0, ny - 1)], 'in the grid')
    both = P.density_bound(ex, alone['depth'], True) + P.density_bound(ex, grid['depth'], False)
    assert abs(mpmath.mpf(float(a[0, 0])) - mpmath.mpf(float(b[0, j]))) <= both
    hold_every_point(b, mock, tau, ys, 'in the grid')
    print('alone %.3f, in the grid %.3f of the bound' % (wa, wb))


@pytest.mark.parametrize('S', [20, 600], ids=['unchunked', 'chunked'])
@pytest.mark.parametrize('nx,ny', [(17, 9), (33, 17)])
def test_a_poisoned_value_stays_where_it_is(device, nx, ny, S):
    """predict_ref.nonfinite_cases: a NaN in one mock[s, i] makes row i NaN and a NaN in one
    ys[i, j] that point, with i and j in the last partial tiles (where the clamped reads of dead
    threads land) -- every other point keeps the bits it has without the NaN.  +inf or negative
    precision: NaN everywhere; mock = +-inf under a positive precision and zero precisions: terms
    of -inf, dropped (exact arithmetic, the bound); all precisions zero: NaN."""
    assert P.kernel_plan(S, nx, ny)['joined'] == (S == 600)
    clean_in = P.mild(S, nx, ny)
    clean = abi_density(device, *clean_in)
    assert not np.any(np.isnan(clean))
    pts = P.sample_points(nx, ny, 4) + P.poisoned_points('', nx, ny)
    hold_to_the_bound(clean, *clean_in, pts[:4], 'clean %d' % S)
    for label, mock, tau, ys in P.nonfinite_cases(nx, ny, S):
        got = abi_density(device, mock, tau, ys)
        mask = P.nonfinite_nan_mask(label, nx, ny)
        assert np.array_equal(np.isnan(got), mask), label
        with np.errstate(all='ignore'):                 # the witness: the numpy restatement
            for i, j in pts:
                want = E.predict(0.0, ys[i, j], mock[:, i, None], tau, polynomial=lambda x, c: c[0])
                assert np.isnan(want) == mask[i, j], (label, i, j)
        if label in ('nan_mock', 'nan_y'):
            assert np.array_equal(got[~mask].view(np.int64), clean[~mask].view(np.int64)), label
        if label in ('pinf_mock', 'ninf_mock'):
            assert np.array_equal(got[:nx - 1].view(np.int64), clean[:nx - 1].view(np.int64)), label
        if not mask.all():
            hold_to_the_bound(got, mock, tau, ys, pts, '%s S=%d %dx%d' % (label, S, nx, ny))


def test_the_largest_grid_a_call_accepts_and_the_first_it_refuses(device):
    """ny = 65535 * 8 is the last grid of one x-point that fits blockIdx.y; one more is refused
    before anything is launched."""
    ny = 65535 * 8
    assert ny == 524280
    mock, tau = np.array([[0.3]]), np.array([1.7])
    ys = np.linspace(-3.0, 3.5, ny)[None, :]
    got = abi_density(device, mock, tau, ys)
    w = hold_to_the_bound(got, mock, tau, ys, [(0, 0), (0, ny - 1), (0, 7), (0, 8), (0, ny - 8), (0, ny - 9), (0, ny // 2)],
                          'largest grid')
    hold_every_point(got, mock, tau, ys, 'largest grid')
    print('largest grid: worst |device - exact| / bound = %.3f' % w)
    ys1 = np.linspace(-3.0, 3.5, ny + 1)[None, :]
    out = abi_density(device, mock, tau, ys1, rc_want=_native.E_UNSUPPORTED)
    assert np.all(out == SENT)


def test_refusals_touch_no_byte(device):
    """The workspace over each input, over ``out``, too small, missing, and not 8-byte aligned:
    each refused on the host, ``out`` and the workspace still at their sentinels."""
    L = _native.lib()
    S, nx, ny = 4096, 3, 5
    mock, tau, ys = P.mild(S, nx, ny)
    md, mw = carve(mock, device, 1, 1)
    td, tw = carve(tau, device, 1, 1)
    yd, yw = carve(ys, device, 1, 1)
    od, ow = carve(np.full(nx * ny, SENT), device, 1, 1)
    need = L.binf_predictive_density_workspace_bytes(S, nx, ny)
    assert need == 16 * nx * ny * 16
    wd, ww = carve(np.full(need // 8, SENT), device, 1, 2)
    kept = [w.clone() for w in (mw, tw, yw)]
    s = _native.stream_handle(device)

    def call(ws, wb, out=od):
        return L.binf_predictive_density_f64(md.data_ptr(), td.data_ptr(), yd.data_ptr(), out.data_ptr(), S, nx, ny,
                                             P.HALF_LOG_2PI, ws, wb, s)
    assert call(md.data_ptr(), need) == _native.E_ALIAS
    assert call(td.data_ptr(), need) == _native.E_ALIAS
    assert call(yd.data_ptr(), need) == _native.E_ALIAS
    assert call(od.data_ptr(), need) == _native.E_ALIAS
    assert call(wd.data_ptr(), need, out=wd[2:]) == _native.E_ALIAS
    assert call(None, need) == _native.E_ARG
    assert call(wd.data_ptr(), need - 8) == _native.E_ARG
    assert call(wd.data_ptr() + 4, need) == _native.E_ARG
    assert 'not 8-byte aligned' in _native.last_error()
    torch.cuda.synchronize()
    assert bool((ow == SENT).all()) and bool((ww == SENT).all())
    for w, k in zip((mw, tw, yw), kept):
        assert torch.equal(w.view(torch.int64), k.view(torch.int64))
    # a grid that needs no workspace refuses a misaligned one all the same, and takes none
    assert L.binf_predictive_density_workspace_bytes(4, nx, ny) == 0
    small = lambda ws: L.binf_predictive_density_f64(md.data_ptr(), td.data_ptr(), yd.data_ptr(), od.data_ptr(), 4, nx, ny,
                                                     P.HALF_LOG_2PI, ws, 0, s)
    assert small(wd.data_ptr() + 4) == _native.E_ARG
    torch.cuda.synchronize()
    assert bool((ow == SENT).all()) and bool((ww == SENT).all())
    assert small(None) == 0 and call(wd.data_ptr(), need) == 0
    torch.cuda.synchronize()
    assert guards_intact(ow, 1, nx * ny) and guards_intact(ww, 1, need // 8) and bool((od > 0).all())


def test_a_side_stream_gives_the_same_bits(device):
    """A chunked call (two launches and a workspace) on a side stream, its inputs produced on that
    stream with no synchronisation before the call, against the same call on the default
    stream."""
    S, nx, ny = 1023, 17, 9
    assert P.kernel_plan(S, nx, ny)['ns'] == 3
    mock, tau, ys = P.mild(S, nx, ny)
    want = abi_density(device, mock, tau, ys)
    host = [torch.from_numpy(np.ascontiguousarray(v)).pin_memory() for v in (mock * 0.5, tau * 0.5, ys * 0.5)]
    L = _native.lib()
    need = L.binf_predictive_density_workspace_bytes(S, nx, ny)
    side = torch.cuda.Stream(device=device)
    with torch.cuda.stream(side):
        md, td, yd = (h.to(device, non_blocking=True) * 2.0 for h in host)     # exact: halves doubled
        ow = torch.full((nx * ny + 8,), SENT, dtype=torch.float64, device=device)
        ww = torch.full((need // 8 + 8,), SENT, dtype=torch.float64, device=device)
        assert _native.stream_handle(device) == side.cuda_stream
        rc = L.binf_predictive_density_f64(md.data_ptr(), td.data_ptr(), yd.data_ptr(), ow[3:].data_ptr(), S, nx, ny,
                                           P.HALF_LOG_2PI, ww[1:].data_ptr(), need, _native.stream_handle(device))
        assert rc == 0, _native.last_error()
    side.synchronize()
    assert guards_intact(ow, 3, nx * ny) and guards_intact(ww, 1, need // 8)
    got = ow[3:3 + nx * ny].cpu().numpy().reshape(nx, ny)
    assert np.array_equal(got.view(np.int64), want.view(np.int64))
