"""The rank layer on the device (``csrc/ranks.hip``, ``binf_amd/diagnostics.py``) against the
host restatement ``tests/rank_diagnostics_ref.py``, bit for bit (NaN where the restatement has
NaN): the entry points through the C ABI with every output carved out of a sentinel buffer,
and ``rank_normalise`` / ``quantiles`` / ``rank_summary`` through Python.

The sort pads a dimension's S values to the power of two P >= S.  P <= 1024 and P <= 8192 are
sorted whole in one workgroup's LDS (two tile sizes); beyond that tiles of 8192 are sorted and
merged in LDS and the strides of 8192 and above are compare-exchange passes over the
workspace, up to three strides per pass while that many are left above the tile (P = 16384: one
pass of one stride; P = 262144: passes of one, two and three strides).  The load tiles 1, 2, 4 or 8 dimensions per workgroup.
The shapes below sit on either side of each of those edges."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import diagnostics_ref as DR
import rank_diagnostics_ref as RR
from binf_amd import _native, diagnostics
from binf_amd.dist import SampleStore
from binf_amd.pdf import IsotropicGaussian
from binf_amd.samplers.hmc import HMCSampler
from binf_amd.samplers.rng import DeviceRNG
from conftest import ROOT

pytestmark = pytest.mark.gpu

SENT = -7.25
GUARD = 66
PROBS = (0.0, 1.0, 1.0 / 3.0, 0.05, 0.5, 0.95, 0.25, 0.975, 0.1, 2.0 / 3.0)
GIB = float(1 << 30)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_ieee(a, b):
    """Bit for bit where the values are numbers (the sign of a zero included); NaN where the
    other is NaN (the sign and payload of a NaN are not part of the contract)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb)) and same_bits(np.where(na, 0.0, a), np.where(nb, 0.0, b))


class Guarded(object):
    """An output of ``shape`` inside a sentinel-filled buffer, off 16-byte alignment when
    ``odd``; ``take()`` checks both guard zones and returns the values."""

    def __init__(self, shape, device, dtype=torch.float64, odd=False):
        self.n = int(np.prod(shape))
        self.shape = shape
        self.before = GUARD + (1 if odd else 0)
        self.fill = SENT if dtype == torch.float64 else 0xA5
        self.whole = torch.full((self.before + self.n + GUARD,), self.fill, dtype=dtype, device=device)
        self.view = self.whole[self.before:self.before + self.n]

    def ptr(self):
        return self.view.data_ptr()

    def take(self, written=True):
        w = self.whole.cpu().numpy()
        assert np.all(w[:self.before] == self.fill) and np.all(w[self.before + self.n:] == self.fill), 'guard zone'
        body = w[self.before:self.before + self.n].reshape(self.shape)
        if not written:
            assert np.all(body == self.fill)
        return body


def carve(x, device, before=GUARD, st=None, sc=None):
    """numpy ``x [T x C x D]`` on the device as a view at element strides (st, sc, 1) of a
    sentinel-filled buffer that ends with the view's last element + GUARD."""
    T, C, D = x.shape
    sc = D if sc is None else sc
    st = C * sc if st is None else st
    span = (T - 1) * st + (C - 1) * sc + D
    whole = torch.full((before + span + GUARD,), SENT, dtype=torch.float64, device=device)
    view = whole[before:before + span].as_strided((T, C, D), (st, sc, 1))
    view.copy_(torch.from_numpy(x))
    return view, whole


def layout(view):
    T, C, D = view.shape
    st, sc, si = view.stride()
    return view.data_ptr(), st, sc, (1 if D == 1 else si), T, C, D


def host_table(S):
    return diagnostics.rank_z_table(S, 'cpu').numpy()


def abi_rank(device, view, split, odd=False, want_sorted=True, want_z=True):
    """binf_rank_normalise_f64 through the C ABI: (sorted [D x S], z [split * n x C x D])."""
    L, s = _native.lib(), _native.stream_handle(device)
    p, st, sc, si, T, C, D = layout(view)
    Tp = split * (T // split)
    S = Tp * C
    need = L.binf_rank_sort_workspace_bytes(S, D)
    P = 1 << max((S - 1).bit_length(), 1)
    assert need == 12 * D * P + 256
    ws = Guarded((need // 8,), device)
    srt = Guarded((D, S), device, odd=odd) if want_sorted else None
    z = Guarded((Tp, C, D), device, odd=not odd) if want_z else None
    ztab = diagnostics.rank_z_table(S, device) if want_z else None
    rc = L.binf_rank_normalise_f64(p, st, sc, si, T, C, D, split, None if ztab is None else ztab.data_ptr(),
                                   None if srt is None else srt.ptr(), None if z is None else z.ptr(),
                                   ws.ptr(), need, s)
    assert rc == 0, _native.last_error()
    ws.take()
    if ztab is not None:
        assert same_ieee(ztab.cpu().numpy(), host_table(S))                # the table is read only
    return (None if srt is None else srt.take()), (None if z is None else z.take())


def abi_quantiles(device, sorted_np, probs, odd=False):
    L, s = _native.lib(), _native.stream_handle(device)
    D, S = sorted_np.shape
    src = torch.from_numpy(np.ascontiguousarray(sorted_np)).to(device)
    out = Guarded((len(probs), D), device, odd=odd)
    rc = L.binf_sorted_quantiles_f64(src.data_ptr(), S, D, (_native.ctypes.c_double * len(probs))(*probs),
                                     len(probs), out.ptr(), s)
    assert rc == 0, _native.last_error()
    assert same_ieee(src.cpu().numpy(), sorted_np)
    return out.take()


def abi_map(device, view, split, op, param_np, odd=False):
    L, s = _native.lib(), _native.stream_handle(device)
    p, st, sc, si, T, C, D = layout(view)
    Tp = split * (T // split)
    param = torch.from_numpy(np.ascontiguousarray(param_np)).to(device)
    out = Guarded((Tp, C, D), device, odd=odd)
    rc = L.binf_draws_map_f64(p, st, sc, si, T, C, D, split, op, param.data_ptr(), out.ptr(), s)
    assert rc == 0, _native.last_error()
    return out.take()


def data(T, C, D, seed=0):
    """AR(1)-like draws with a per-chain offset and scale, so that rhat and ess are not trivial."""
    rs = np.random.RandomState(3000 + seed)
    x = DR.ar1(0.6, T, C, D, seed=4000 + seed)
    return np.ascontiguousarray(x * (1.0 + 0.1 * rs.standard_normal((1, C, D))) + 0.3 * rs.standard_normal((1, C, D)))


def check_summary(got, want, what, eq=same_bits):
    for k in RR.FIELDS:
        assert eq(getattr(got, k).cpu().numpy(), want[k]), (what, k)


def run_shape(device, T, C, D, seed, max_lag):
    x = data(T, C, D, seed)
    S2, S1 = 2 * (T // 2) * C, T * C
    view, whole = carve(x, device, before=GUARD + (seed % 2))
    before = whole.cpu().numpy().copy()
    # the C ABI, both splits
    for split, S in ((2, S2), (1, S1)):
        srt, z = abi_rank(device, view, split, odd=bool(seed % 2))
        want_sorted = RR.sorted_pooled(x, split)
        assert same_bits(srt, want_sorted), ('sorted', split)
        assert same_bits(z, RR.rank_normalise(x, split, host_table(S))), ('z', split)
        only_sorted, none = abi_rank(device, view, split, want_z=False)
        assert none is None and same_bits(only_sorted, want_sorted)
        none, only_z = abi_rank(device, view, split, want_sorted=False)
        assert none is None and same_bits(only_z, z)
        q = abi_quantiles(device, srt, PROBS, odd=True)
        assert same_bits(q, RR.quantiles_sorted(want_sorted, PROBS)), ('quantiles', split)
        assert same_bits(q, np.quantile(RR.split_record(x, split).reshape(-1, D), PROBS, axis=0))
        for op in (RR.FOLD, RR.LE):
            assert same_bits(abi_map(device, view, split, op, q[4], odd=(op == RR.LE)), RR.draws_map(x, split, op, q[4]))
    # Python
    assert same_bits(diagnostics.rank_normalise(view).cpu().numpy(), RR.rank_normalise(x, 2, host_table(S2)))
    assert same_bits(diagnostics.quantiles(view, PROBS).cpu().numpy(), RR.quantiles(x, PROBS))
    got = diagnostics.rank_summary(view, max_lag=max_lag)
    check_summary(got, RR.rank_summary(x, host_table(S2), max_lag=max_lag), (T, C, D))
    assert same_bits(whole.cpu().numpy(), before)                          # the draws are read only
    return got


@pytest.mark.parametrize('T,C,D', [(4, 1, 1), (5, 1, 3), (8, 3, 2), (64, 2, 5), (66, 2, 9)])
def test_small_records_and_padding(device, T, C, D):
    """Odd T (the middle draw dropped), S no power of two, S an exact power of two (8, 128,
    256 with split 2; 4, 64 ... with split 1), 1, 2, 4 and 8 dimensions per workgroup of the load."""
    run_shape(device, T, C, D, seed=T + D, max_lag=None)


@pytest.mark.parametrize('T,C,D', [(8190, 1, 1), (8192, 1, 2), (128, 64, 3)])
def test_lds_tier_boundary(device, T, C, D):
    """S = 8190 and 8192: the largest record that one workgroup sorts whole."""
    run_shape(device, T, C, D, seed=T + D, max_lag=6)


@pytest.mark.parametrize('T,C,D', [(8194, 1, 1), (16384, 1, 2), (1026, 128, 2)])
def test_global_tier(device, T, C, D):
    """S = 8194 and 16384 (P = 16384: one pass over the workspace per stage) and 131328
    (P = 262144: stages of one to five strides above the tile, passes of one, two and three)."""
    run_shape(device, T, C, D, seed=T + D, max_lag=6)


# ---------------------------------------------------------------------------
# ties and IEEE edges
# ---------------------------------------------------------------------------
def edge_record():
    T, C, D = 30, 4, 10
    rng = np.random.default_rng(21)
    x = data(T, C, D, seed=13)
    x[:, :, 0] = rng.integers(0, 5, size=(T, C)).astype(np.float64)        # integers from {0..4}
    x[:, :, 1] = 2.5                                                        # constant everywhere
    x[:, :, 2] = np.where(rng.random((T, C)) < 0.5, 0.0, -0.0)              # +-0.0 mixed ...
    x[::5, :, 2] = rng.standard_normal((6, C))                              # ... among numbers of either sign
    x[3, 1, 3], x[17, 0, 3], x[18, 2, 3], x[29, 3, 3] = np.inf, -np.inf, np.inf, -np.inf
    x[:, :, 4] = rng.integers(-20, 20, size=(T, C)) * 4.9406564584124654e-324   # subnormals around zero
    x[:, :, 5] = 1.0 + rng.integers(0, 3, size=(T, C)) * 2.0 ** -52        # neighbours one ulp apart
    x[:, :, 6] = -np.abs(x[:, :, 6]) - 1.0                                  # negative throughout
    x[11, 2, 7] = np.nan                                                    # one NaN ...
    x[12, 2, 7] = -np.nan                                                   # ... and one of the other sign
    x[:, :, 8] = np.where(rng.random((T, C)) < 0.3, -0.0, x[:, :, 8])
    return np.ascontiguousarray(x)


def test_ties_and_ieee_edges_fall_as_the_restatement_says(device):
    x = edge_record()
    T, C, D = x.shape
    S = T * C
    view, _ = carve(x, device)
    srt, z = abi_rank(device, view, 2)
    want_sorted, want_z = RR.sorted_pooled(x, 2), RR.rank_normalise(x, 2, host_table(S))
    assert same_ieee(srt, want_sorted) and same_ieee(z, want_z)
    assert np.all(z[:, :, 1] == 0.0) and not np.signbit(z[:, :, 1]).any()           # constant: every rank (S + 1) / 2
    assert np.isnan(z[:, :, 7]).all() and np.isnan(srt[7, -2:]).all() and not np.isnan(srt[7, :-2]).any()
    assert not np.isnan(np.delete(z, 7, axis=2)).any()
    zeros = srt[2][srt[2] == 0.0]
    assert np.signbit(zeros).any() and not np.signbit(zeros).all()
    assert np.array_equal(np.signbit(zeros), np.sort(np.signbit(zeros))[::-1])       # every -0.0 before every +0.0
    assert srt[3, 0] == -np.inf and srt[3, 1] == -np.inf and srt[3, -1] == np.inf
    q = abi_quantiles(device, srt, PROBS)
    assert same_ieee(q, RR.quantiles_sorted(want_sorted, PROBS))
    assert np.isnan(q[:, 7]).all() and not np.isnan(np.delete(q, [3, 7], axis=1)).any()
    for op in (RR.FOLD, RR.LE):
        assert same_ieee(abi_map(device, view, 2, op, q[4]), RR.draws_map(x, 2, op, q[4]))
    got = diagnostics.rank_summary(view, max_lag=9)
    want = RR.rank_summary(x, host_table(S), max_lag=9)
    check_summary(got, want, 'edges', eq=same_ieee)
    assert np.isnan(want['rhat'][1]) and np.isnan(want['rhat'][7]) and np.all(np.isfinite(want['rhat'][[0, 5, 6, 8, 9]]))
    # the other dimensions keep their bits beside the NaN
    clean = RR.rank_summary(np.ascontiguousarray(x[:, :, 8:]), host_table(S), max_lag=9)
    for k in RR.FIELDS:
        assert same_bits(getattr(got, k).cpu().numpy()[..., 8:], clean[k]), k


def test_combine_hands_nan_on_and_ors_the_flags(device):
    L, s = _native.lib(), _native.stream_handle(device)
    nan, inf = np.nan, np.inf
    a = np.array([1.0, 1.2, nan, 1.0, nan, inf, 1.0, 0.0, 3.0])
    b = np.array([1.1, 1.0, 1.0, nan, nan, 1.0, -inf, 0.0, 3.0])
    flags = [np.array([(i >> f) & 1 for i in range(9)], dtype=np.uint8) for f in range(4)]
    D = a.shape[0]
    dev = lambda v: torch.from_numpy(v).to(device)
    ins = [dev(a), dev(b), dev(b), dev(a)] + [dev(f) for f in flags]
    rhat, ess, tr = Guarded((D,), device, odd=True), Guarded((D,), device), Guarded((D,), device, dtype=torch.uint8, odd=True)
    rc = L.binf_rank_diag_combine_f64(*([t.data_ptr() for t in ins] + [D, rhat.ptr(), ess.ptr(), tr.ptr(), s]))
    assert rc == 0, _native.last_error()
    want = RR.combine(a, b, b, a, flags)
    assert same_ieee(rhat.take(), want[0]) and same_ieee(ess.take(), want[1]) and same_bits(tr.take(), want[2])
    assert list(want[2]) == [0] + [1] * 8


# ---------------------------------------------------------------------------
# views
# ---------------------------------------------------------------------------
def test_views_are_read_where_they_lie(device):
    """[..., :K] of a wider slot, every 3rd chain of a ladder, a chain-major (transposed) record
    and a view at an odd element offset: each inside a sentinel buffer, through the C ABI and
    through binf_amd.diagnostics."""
    T, C, D = 41, 6, 7
    x = data(T, C, D, seed=5)
    S = 40 * C
    want = RR.rank_summary(x, host_table(S), max_lag=7)
    want_sorted, want_z = RR.sorted_pooled(x, 2), RR.rank_normalise(x, 2, host_table(S))
    cases = {'plain': dict(), 'odd offset': dict(before=GUARD + 1), 'columns of 11': dict(sc=11),
             'every 3rd chain': dict(sc=3 * D, st=3 * D * C + 5), 'chain-major': dict(st=D, sc=T * D + 3)}
    for name, kw in cases.items():
        view, whole = carve(x, device, **kw)
        assert (view.data_ptr() % 16 == 8) == (name == 'odd offset')
        before = whole.cpu().numpy().copy()
        srt, z = abi_rank(device, view, 2)
        assert same_bits(srt, want_sorted) and same_bits(z, want_z), name
        assert same_bits(abi_map(device, view, 2, RR.FOLD, want['quantiles'][1]),
                         RR.draws_map(x, 2, RR.FOLD, want['quantiles'][1])), name
        check_summary(diagnostics.rank_summary(view, max_lag=7), want, name)
        assert same_bits(diagnostics.quantiles(view, PROBS).cpu().numpy(), RR.quantiles(x, PROBS)), name
        assert same_bits(whole.cpu().numpy(), before), name
    wide = torch.full((T, C * 3, D + 4), SENT, dtype=torch.float64, device=device)
    wide[:, 1::3, :D] = torch.from_numpy(x).to(device)
    v = wide[:, 1::3, :D]
    assert not v.is_contiguous()
    check_summary(diagnostics.rank_summary(v, max_lag=7), want, 'torch slicing')
    text = str(diagnostics.rank_summary(v, max_lag=7))
    assert text.splitlines()[0].split() == ['dim', 'mean', 'sd', 'rhat', 'ess_bulk', 'ess_tail', 'mcse', 'q5', 'q50', 'q95']
    assert len(text.splitlines()) >= 1 + D


def test_draw_stride_beyond_2_31_elements(device):
    """Element offsets past 2**31 (a draw stride of 2**29 + 3 inside a 17 GB buffer that is never
    filled): every offset is formed in 64 bits."""
    free, _ = torch.cuda.mem_get_info(device)
    if free < 24 * GIB:
        pytest.skip('needs 24 GiB of free HBM, %.0f free' % (free / GIB))
    T, C, D = 5, 3, 5
    st, sc = (1 << 29) + 3, 7
    span = (T - 1) * st + (C - 1) * sc + D
    assert (T - 1) * st > 1 << 31
    x = DR.ar1(0.4, T, C, D, seed=78)
    whole = torch.empty(1 + span, dtype=torch.float64, device=device)
    view = got = z = q = m = None
    try:
        view = whole[1:].as_strided((T, C, D), (st, sc, 1))
        view.copy_(torch.from_numpy(x))
        got = diagnostics.rank_summary(view, max_lag=1)
        check_summary(got, RR.rank_summary(x, host_table(4 * C), max_lag=1), 'large stride')
        z = diagnostics.rank_normalise(view, split=1)
        assert same_bits(z.cpu().numpy(), RR.rank_normalise(x, 1, host_table(T * C)))
        q = diagnostics.quantiles(view, PROBS)
        assert same_bits(q.cpu().numpy(), RR.quantiles(x, PROBS))
        m = _native.draws_map(view, 1, _native.DRAWS_MAP_LE, q[4].contiguous())
        assert same_bits(m.cpu().numpy(), RR.draws_map(x, 1, RR.LE, RR.quantiles(x, PROBS)[4]))
    finally:
        del whole, view, got, z, q, m
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------
# grouping
# ---------------------------------------------------------------------------
def test_result_does_not_depend_on_the_grouping(device):
    T, C, D = 37, 5, 6
    x = data(T, C, D, seed=17)
    view, _ = carve(x, device, sc=D + 3)
    whole = diagnostics.rank_summary(view, probs=PROBS, max_lag=11)
    one = diagnostics.rank_summary(view, probs=PROBS, max_lag=11, max_scratch_bytes=1)     # a dimension at a time
    some = diagnostics.rank_summary(view, probs=PROBS, max_lag=11, max_scratch_bytes=8 * (2 * T * C + 1) + 4 * (
        16 * T * C + 12 * 256 + 256))                                                      # groups of 4 and 2
    want = RR.rank_summary(x, host_table(36 * C), probs=PROBS, max_lag=11)
    for got, what in ((whole, 'whole'), (one, 'one'), (some, 'some')):
        check_summary(got, want, what)
        assert got.probs == PROBS


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
def test_refusals_come_before_anything_is_touched(device):
    L, s = _native.lib(), _native.stream_handle(device)
    E_ARG, E_ALIAS, E_UNS = _native.E_ARG, _native.E_ALIAS, _native.E_UNSUPPORTED
    T, C, D = 10, 3, 4
    S = T * C
    x = data(T, C, D)
    view, whole = carve(x, device)
    before = whole.cpu().numpy().copy()
    p = view.data_ptr()
    need = L.binf_rank_sort_workspace_bytes(S, D)
    ws, srt, z = Guarded((need // 8,), device), Guarded((D, S), device), Guarded((T, C, D), device)
    ztab = diagnostics.rank_z_table(S, device)

    def rank(p_=p, st=C * D, sc=D, si=1, T_=T, C_=C, D_=D, split=2, ztab_=ztab.data_ptr(), srt_=srt.ptr(), z_=z.ptr(),
             ws_=ws.ptr(), bytes_=need):
        return L.binf_rank_normalise_f64(p_, st, sc, si, T_, C_, D_, split, ztab_, srt_, z_, ws_, bytes_, s)
    assert rank(srt_=None, z_=None) == E_ARG and 'neither' in _native.last_error()
    assert rank(ztab_=None) == E_ARG and 'ztab' in _native.last_error()
    assert rank(ws_=None) == E_ARG and rank(bytes_=need - 1) == E_ARG and 'workspace' in _native.last_error()
    assert rank(ws_=ws.ptr() + 4) == E_ARG
    assert rank(p_=None) == E_ARG and rank(split=3) == E_ARG and rank(si=2) == E_ARG and rank(T_=3) == E_ARG
    assert rank(C_=0) == E_ARG and rank(D_=0) == E_ARG and rank(st=-1) == E_ARG and rank(st=D) == E_ARG
    assert rank(z_=p + 8) == E_ALIAS and rank(srt_=ws.ptr() + 64) == E_ALIAS and rank(srt_=z.ptr() + 16) == E_ALIAS
    assert rank(ws_=ztab.data_ptr()) == E_ALIAS and rank(z_=ztab.data_ptr() + 8 * S) == E_ALIAS
    # a pooled set beyond 2**30 values: a view that is never read
    assert rank(T_=(1 << 30) + 2, C_=1, D_=1, st=1, sc=1, split=1) == E_UNS and '2^30' in _native.last_error()
    assert rank(T_=(1 << 31) + 2, C_=1, D_=1, st=1, sc=1, split=2) == E_UNS
    assert L.binf_rank_sort_workspace_bytes((1 << 30) + 1, 1) == 0 and L.binf_rank_sort_workspace_bytes(1, 1) == 0
    assert L.binf_rank_sort_workspace_bytes(1 << 30, 1) == 12 * (1 << 30) + 256

    probs = (_native.ctypes.c_double * 17)(*([0.5] * 17))
    q = Guarded((17, D), device)
    sp = srt.ptr()

    def quant(sorted_=sp, S_=S, D_=D, probs_=probs, Q=3, out=q.ptr()):
        return L.binf_sorted_quantiles_f64(sorted_, S_, D_, probs_, Q, out, s)
    assert quant(Q=17) == E_ARG and '16' in _native.last_error()
    assert quant(Q=0) == E_ARG and quant(S_=0) == E_ARG and quant(D_=0) == E_ARG
    assert quant(sorted_=None) == E_ARG and quant(probs_=None) == E_ARG and quant(out=None) == E_ARG
    for bad in (1.0000001, -1e-300, float('nan'), float('inf')):
        assert quant(probs_=(_native.ctypes.c_double * 3)(0.5, bad, 0.1)) == E_ARG and 'outside' in _native.last_error()
    assert quant(out=sp + 8 * (S * D - 1)) == E_ALIAS
    with pytest.raises(ValueError):
        diagnostics.quantiles(view, (0.5, 1.5))
    with pytest.raises(ValueError):
        diagnostics.quantiles(view, [0.5] * 17)

    param = torch.zeros(D, dtype=torch.float64, device=device)
    m = Guarded((T, C, D), device)

    def dmap(p_=p, split=2, op=RR.FOLD, param_=param.data_ptr(), out=m.ptr(), si=1):
        return L.binf_draws_map_f64(p_, C * D, D, si, T, C, D, split, op, param_, out, s)
    assert dmap(op=2) == E_ARG and dmap(op=-1) == E_ARG and dmap(param_=None) == E_ARG and dmap(out=None) == E_ARG
    assert dmap(split=0) == E_ARG and dmap(si=0) == E_ARG and dmap(p_=None) == E_ARG
    assert dmap(out=p + 8 * (T * C * D - 1)) == E_ALIAS and dmap(out=param.data_ptr()) == E_ALIAS

    v = [torch.ones(D, dtype=torch.float64, device=device) for _ in range(4)]
    f = [torch.zeros(D, dtype=torch.uint8, device=device) for _ in range(4)]
    o = [Guarded((D,), device), Guarded((D,), device), Guarded((D,), device, dtype=torch.uint8)]

    def comb(**kw):
        a = [t.data_ptr() for t in v + f] + [D] + [g.ptr() for g in o] + [s]
        for k, val in kw.items():
            a[int(k[1:])] = val
        return L.binf_rank_diag_combine_f64(*a)
    assert comb(a8=0) == E_ARG
    for k in (0, 3, 4, 7, 9, 10, 11):
        assert comb(**{'a%d' % k: None}) == E_ARG, k
    assert comb(a9=v[1].data_ptr()) == E_ALIAS and comb(a11=f[2].data_ptr() + 1) == E_ALIAS
    assert comb(a10=o[0].ptr() + 8) == E_ALIAS

    torch.cuda.synchronize(device)
    for g in (ws, srt, z, q, m) + tuple(o):
        g.take(written=False)
    assert same_bits(whole.cpu().numpy(), before) and bool((param == 0.0).all())


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------
def test_hmc_record_through_the_store(device):
    """64 chains x 6 dimensions of the unit Gaussian: the store's rank_summary of four of its
    columns is rank_summary of the slice, is the restatement's; the rank R^ says converged and
    the 5 % / 50 % / 95 % quantiles are the normal's within their Monte-Carlo error."""
    C, D, n = 64, 6, 120
    start = torch.from_numpy(np.random.RandomState(4).standard_normal((C, D))).to(device)
    s = HMCSampler(IsotropicGaussian(1.0, 0.0), start, 0.05, 20, variable_name='x', rng=DeviceRNG(23, device))
    store = SampleStore(n + 5, C, D, device=device)
    store.buffer.fill_(SENT)
    store.extend(s.sample_n(n))
    got = store.rank_summary(columns=slice(1, 5), max_lag=20)
    kept = store.local()[..., 1:5]
    assert not kept.is_contiguous()
    again = diagnostics.rank_summary(kept, max_lag=20)
    x = kept.cpu().numpy()
    want = RR.rank_summary(x, host_table(n * C), max_lag=20)
    check_summary(got, want, 'store')
    check_summary(again, want, 'slice')
    print(got.table(names=['x%d' % i for i in range(1, 5)]))
    assert np.all(want['rhat'] < 1.05) and np.all(want['ess_tail'] > 100.0)
    assert np.all(np.abs(want['quantiles'] - np.array([[-1.6449], [0.0], [1.6449]])) < 0.15)
    assert bool((store.buffer[n:] == SENT).all())
    everything = store.rank_summary()
    assert same_bits(everything.rhat.cpu().numpy()[1:5], want['rhat'])


@pytest.mark.parametrize('args', [['--rank', '--chains', '256', '--dims', '4', '--short', '8', '--long', '60'],
                                  ['--rank', '--ladder', '--ladders', '16', '--rounds', '24']])
def test_example_prints_the_rank_table(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'convergence.py')] + args,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    text = r.stdout.decode('utf-8', 'replace')
    assert r.returncode == 0, text
    assert text.count('ess_tail') == 2 and text.count('q50') == 2, text
