"""Convergence diagnostics on the device (``csrc/diagnostics.hip``, ``binf_amd/diagnostics.py``)
against the host restatement ``tests/diagnostics_ref.py``, bit for bit: the three entry points
through the C ABI with every output carved out of a sentinel buffer, strided views read where
they lie, IEEE edges, gather == whole, a sampler's record end to end, the example.

The autocovariance kernel's tile: a thread owns 16 consecutive lags (``DIAG_LT``) and advances
16 draws per step of its register window; a step is straight-line code while
``i0 + k0 + 30 < n`` and tests every product after that (the last two or three steps); a
workgroup is one block of 64 split chains x 1, 2, 4 or 8 dimensions x one lag tile.
The shapes below sit on either side of each of those edges."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import diagnostics_ref as DR
from binf_amd import _native, diagnostics
from binf_amd.dist import SampleStore
from binf_amd.pdf import IsotropicGaussian
from binf_amd.samplers.hmc import HMCSampler
from binf_amd.samplers.rng import DeviceRNG
from conftest import ROOT

pytestmark = pytest.mark.gpu

SENT = -7.25
GUARD = 66                         # sentinel elements on either side of every output (even: 16-byte aligned views)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_ieee(a, b):
    """Bit for bit where the values are numbers; NaN where the other is NaN (the sign and
    payload of a generated NaN belong to the machine, not to the contract)."""
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


def abi_run(device, view, split, K, odd=False, rhat_only=False):
    """moments -> autocov -> summary through the C ABI; returns a dict of numpy results."""
    L = _native.lib()
    s = _native.stream_handle(device)
    T, C, D = view.shape
    st, sc, si = view.stride()
    if D == 1:
        si = 1
    n, M = T // split, split * C
    mean, m2 = Guarded((M, D), device, odd=odd), Guarded((M, D), device)
    rc = L.binf_chain_moments_f64(view.data_ptr(), st, sc, si, T, C, D, split, mean.ptr(), m2.ptr(), s)
    assert rc == 0, _native.last_error()
    out = dict(chain_mean=mean.take(), chain_m2=m2.take())
    if M < 2:
        return out
    part = None
    if not rhat_only:
        nb = (M + 63) // 64
        assert L.binf_chain_autocov_workspace_bytes(M, D, K) == nb * (K + 1) * D * 8
        part = Guarded((nb, K + 1, D), device, odd=odd)
        rc = L.binf_chain_autocov_f64(view.data_ptr(), st, sc, si, T, C, D, split, mean.ptr(), K, part.ptr(),
                                      part.n * 8, s)
        assert rc == 0, _native.last_error()
        out['partials'] = part.take()
    names = ('post_mean', 'varplus', 'sd', 'W', 'rhat', 'ess', 'mcse')
    g = {k: Guarded((D,), device, odd=(odd and j % 2 == 0)) for j, k in enumerate(names)}
    g['truncated'] = Guarded((D,), device, dtype=torch.uint8, odd=True)
    need = L.binf_diag_summary_workspace_bytes(M, D)
    ws = Guarded((need // 8,), device)
    rc = L.binf_diag_summary_f64(mean.ptr(), m2.ptr(), None if part is None else part.ptr(), n, M, D, K,
                                 g['post_mean'].ptr(), g['varplus'].ptr(), g['sd'].ptr(), g['W'].ptr(),
                                 g['rhat'].ptr(), g['ess'].ptr(), g['mcse'].ptr(), g['truncated'].ptr(),
                                 ws.ptr(), need, s)
    assert rc == 0, _native.last_error()
    ws.take()
    for k in g:
        out[k] = g[k].take(written=not (rhat_only and k in ('ess', 'mcse', 'truncated')))
    mean.take(), m2.take()                                       # inputs of the later calls: untouched since
    assert same_bits(mean.take(), out['chain_mean'])
    return out


FULL = ('chain_mean', 'chain_m2', 'partials', 'post_mean', 'varplus', 'sd', 'W', 'rhat', 'ess', 'mcse', 'truncated')


def check(got, want, what, eq=same_bits):
    for k in FULL:
        if k in got:
            w = DR.autocov_partials(want['a']) if k == 'partials' else want[k]
            assert eq(got[k], w), (what, k)


def data(T, C, D, seed=0):
    """AR(1)-like draws with a per-chain offset and scale, so that rhat and ess are not trivial."""
    rs = np.random.RandomState(1000 + seed)
    x = DR.ar1(0.6, T, C, D, seed=2000 + seed)
    return np.ascontiguousarray(x * (1.0 + 0.1 * rs.standard_normal((1, C, D))) + 0.3 * rs.standard_normal((1, C, D)))


def run_case(device, T, C, D, split, K, odd=False, seed=0):
    x = data(T, C, D, seed)
    view, whole = carve(x, device, before=GUARD + (1 if odd else 0))
    got = abi_run(device, view, split, K, odd=odd)
    assert same_bits(view.cpu().numpy(), x)                               # the draws are read only
    if split * C < 2:
        mo = DR.moments(x, split)
        assert same_bits(got['chain_mean'], mo['mean']) and same_bits(got['chain_m2'], mo['m2'])
        return
    check(got, DR.diagnose(x, split, K), (T, C, D, split, K, odd))


BASE = (65, 65, 65, 9)


@pytest.mark.parametrize('T', [2, 3, 4, 5, 7, 65, 130])
def test_sweep_of_the_draw_count(device, T):
    """Both splits from T = 4; T = 2, 3 with split = 1; T = 3 with split = 2 is refused."""
    _, C, D, K = BASE
    for split in (1, 2):
        n = T // split
        if n < 2:
            L = _native.lib()
            x = torch.zeros((T, C, D), dtype=torch.float64, device=device)
            rc = L.binf_chain_moments_f64(x.data_ptr(), C * D, D, 1, T, C, D, split, x.data_ptr(), x.data_ptr(),
                                          _native.stream_handle(device))
            assert rc == _native.E_ARG and 'n >= 2' in _native.last_error()
            continue
        run_case(device, T, C, D, split, min(K, n - 1), seed=T)


@pytest.mark.parametrize('C', [1, 2, 63, 64, 65, 130])
def test_sweep_of_the_chain_count(device, C):
    """The 64-chain block edge for M = C and for M = 2 C; one chain has moments only (split =
    1) and a two-chain summary (split = 2)."""
    T, _, D, K = BASE
    for split in (1, 2):
        run_case(device, T, C, D, split, K, odd=(split == 2), seed=C)
    if C == 1:
        L = _native.lib()
        p = torch.zeros(4 * D, dtype=torch.float64, device=device).data_ptr()
        rc = L.binf_diag_summary_f64(p, p, None, T, 1, D, 0, p, p, p, p, p, None, None, None, p, 8 * 4 * D, None)
        assert rc == _native.E_ARG and 'M >= 2' in _native.last_error()


@pytest.mark.parametrize('D', [1, 7, 63, 64, 65, 200])
def test_sweep_of_the_dimension(device, D):
    T, C, _, K = BASE
    for split in (1, 2):
        run_case(device, T, C, D, split, K, odd=(D % 2 == 1), seed=D)


@pytest.mark.parametrize('K', [0, 1, 7, 8, 9, 15, 16, 17, 31])
def test_sweep_of_max_lag(device, K):
    """n = 32 (split = 2) and n = 65 (split = 1) around the 16-lag tile; K = 31 is n - 1 of the
    split run; the unsplit run's n - 1 = 64 rides along with it."""
    T, C, D, _ = BASE
    run_case(device, T, C, D, 2, K, seed=K)
    run_case(device, T, C, D, 1, 64 if K == 31 else K, seed=100 + K)


@pytest.mark.parametrize('T,C,D,split,K', [
    (4, 1, 1, 2, 1), (4, 2, 1, 1, 3), (130, 130, 200, 1, 17), (130, 130, 1, 1, 129), (130, 3, 2, 2, 64),
    (63, 5, 3, 1, 62), (62, 5, 3, 2, 30), (31, 70, 9, 1, 0), (47, 2, 5, 1, 16), (94, 2, 4, 2, 33)])
def test_corners(device, T, C, D, split, K):
    """Smallest and largest of every axis together; n = 31, 47, 63: the register window's last
    step ends exactly on the last draw; 1, 2, 4 and 8 dimensions per workgroup."""
    run_case(device, T, C, D, split, K, odd=True, seed=T + C)


def test_rhat_alone_leaves_the_ess_outputs_alone(device):
    x = data(20, 70, 5)
    view, _ = carve(x, device)
    got = abi_run(device, view, 2, 0, rhat_only=True)
    want = DR.diagnose(x, 2, 0)
    for k in ('post_mean', 'varplus', 'sd', 'W', 'rhat'):
        assert same_bits(got[k], want[k]), k


# ---------------------------------------------------------------------------
# views
# ---------------------------------------------------------------------------
def test_views_are_read_where_they_lie(device):
    """The store's own buffer (partly filled), [..., :K] of a wider slot, [:, r::R, :] of a
    ladder, a chain-major (transposed) record and a view at an odd element offset: each inside
    a sentinel buffer, through the C ABI and through binf_amd.diagnostics."""
    T, C, D = 40, 66, 7
    x = data(T, C, D, seed=5)
    want = DR.diagnose(x, 2, 12)
    cases = {'plain': dict(), 'odd offset': dict(before=GUARD + 1), 'columns of 11': dict(sc=11),
             'every 3rd chain': dict(sc=3 * D, st=3 * D * C + 5), 'chain-major': dict(st=D, sc=T * D + 3)}
    for name, kw in cases.items():
        view, whole = carve(x, device, **kw)
        assert (view.data_ptr() % 16 == 8) == (name == 'odd offset')
        before = whole.cpu().numpy().copy()
        check(abi_run(device, view, 2, 12), want, name)
        s = diagnostics.summary(view, max_lag=12)
        for k, w in (('mean', 'post_mean'), ('sd', 'sd'), ('rhat', 'rhat'), ('ess', 'ess'), ('mcse', 'mcse'),
                     ('truncated', 'truncated')):
            assert same_bits(getattr(s, k).cpu().numpy(), want[w]), (name, k)
        assert same_bits(whole.cpu().numpy(), before), name
    # the same through torch's own slicing, and the store
    wide = torch.full((T, C * 3, D + 4), SENT, dtype=torch.float64, device=device)
    wide[:, 1::3, :D] = torch.from_numpy(x).to(device)
    v = wide[:, 1::3, :D]
    assert not v.is_contiguous()
    assert same_bits(diagnostics.split_rhat(v).cpu().numpy(), want['rhat'])
    assert same_bits(diagnostics.effective_sample_size(v, max_lag=12).cpu().numpy(), want['ess'])
    mo = diagnostics.chain_moments(v, split=2)
    assert mo.n == 20 and same_bits(mo.mean.cpu().numpy(), want['chain_mean'])
    assert same_bits(mo.m2.cpu().numpy(), want['chain_m2'])
    store = SampleStore(T + 9, C, D + 4, device=device)
    store.buffer.fill_(SENT)
    block = torch.full((T, C, D + 4), 3.5, dtype=torch.float64, device=device)
    block[:, :, :D] = torch.from_numpy(x).to(device)
    store.extend(block)
    s = store.summary(columns=slice(0, D), max_lag=12)
    assert same_bits(s.rhat.cpu().numpy(), want['rhat']) and same_bits(s.ess.cpu().numpy(), want['ess'])
    assert same_bits(s.mcse.cpu().numpy(), want['mcse'])
    full = store.summary()                                                  # default max_lag = min(n - 1, 64) = 19
    assert same_bits(full.ess.cpu().numpy()[:D], DR.diagnose(x, 2)['ess'])
    assert np.all(np.isnan(full.rhat.cpu().numpy()[D:]))                    # constant columns
    assert bool((store.buffer[T:] == SENT).all())
    text = str(s)
    assert text.splitlines()[0].split() == ['dim', 'mean', 'sd', 'rhat', 'ess', 'mcse'] and len(text.splitlines()) >= 1 + D


# ---------------------------------------------------------------------------
# IEEE edges
# ---------------------------------------------------------------------------
def test_ieee_edges_fall_as_the_restatement_says(device):
    """Dimension 0 constant in every chain (NaN rhat, by the contract), 1 with one NaN draw, 2
    with +inf, 3 with -inf, 4 near DBL_MAX (d * d overflows), 5 constant in ONE chain, 6 and 7
    ordinary: the ordinary ones and each other are untouched, the rest fall as numpy's do."""
    T, C, D = 36, 70, 8
    x = data(T, C, D, seed=9)
    x[:, :, 0] = 2.5
    x[7, 3, 1] = np.nan
    x[30, 65, 2] = np.inf
    x[0, 0, 3] = -np.inf
    x[:, :, 4] *= 3.0e307
    x[:, 2, 5] = -1.0
    clean = DR.diagnose(np.ascontiguousarray(x[:, :, 5:]), 2, 17)
    want = DR.diagnose(x, 2, 17)
    assert np.isnan(want['rhat'][0]) and np.isnan(want['rhat'][1]) and np.all(np.isfinite(want['rhat'][5:]))
    assert np.all(np.isinf(want['chain_m2'][:, 4]) | np.isnan(want['chain_m2'][:, 4]))
    assert same_bits(want['ess'][5:], clean['ess'])
    view, _ = carve(x, device)
    got = abi_run(device, view, 2, 17)
    check(got, want, 'ieee', eq=same_ieee)
    for k in ('post_mean', 'rhat', 'ess', 'mcse', 'truncated'):
        assert same_bits(got[k][5:], clean[k]), k
    s = diagnostics.summary(view, max_lag=17)
    assert same_ieee(s.rhat.cpu().numpy(), want['rhat']) and same_ieee(s.ess.cpu().numpy(), want['ess'])


# ---------------------------------------------------------------------------
# gather == whole
# ---------------------------------------------------------------------------
def test_summary_of_assembled_shards_equals_the_whole(device):
    T, C, D = 50, 100, 6
    x = data(T, C, D, seed=11)
    whole = torch.from_numpy(x).to(device)
    a, b = whole[:, :37].contiguous(), whole[:, 37:].contiguous()
    gathered = torch.cat([a, b], dim=1)                # what SampleStore.gather() hands back
    assert gathered.data_ptr() != whole.data_ptr()
    s0, s1 = diagnostics.summary(whole), diagnostics.summary(gathered)
    want = DR.diagnose(x, 2)
    for k, w in zip(s0._fields, ('post_mean', 'sd', 'rhat', 'ess', 'mcse', 'truncated')):
        assert same_bits(getattr(s0, k).cpu().numpy(), getattr(s1, k).cpu().numpy()), k
        assert same_bits(getattr(s0, k).cpu().numpy(), want[w]), k


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------
def test_hmc_record_converges_by_rhat(device):
    """128 chains x 8 dimensions of the unit Gaussian from a start spread over +-10: split-R^
    of the first 8 kept draws is above that of draws 200 .. 400, and the latter is below 1.05
    (the stationary law is known: consecutive draws of this trajectory length are correlated
    by cos(1) = 0.54, so R^ - 1 is about (tau - 1) / (2 n) = 0.012 at n = 100)."""
    C, D = 128, 8
    start = torch.from_numpy(np.random.RandomState(3).uniform(-10.0, 10.0, size=(C, D))).to(device)
    s = HMCSampler(IsotropicGaussian(1.0, 0.0), start, 0.05, 20, variable_name='x', rng=DeviceRNG(17, device))
    draws = s.sample_n(400)
    early = diagnostics.split_rhat(draws[:8]).cpu().numpy()
    late = diagnostics.summary(draws[200:])
    rhat = late.rhat.cpu().numpy()
    print('rhat of draws 0..8: %s\nrhat of draws 200..400: %s\ness: %s' % (early, rhat, late.ess.cpu().numpy()))
    assert np.all(early > rhat)
    assert np.all(rhat < 1.05)
    x = draws[200:].cpu().numpy()
    assert same_bits(rhat, DR.diagnose(x, 2)['rhat'])
    assert np.all(np.abs(late.mean.cpu().numpy()) < 6.0 * late.mcse.cpu().numpy() + 0.05)


@pytest.mark.parametrize('args', [['--chains', '256', '--dims', '4', '--short', '8', '--long', '60'],
                                  ['--ladder', '--ladders', '16', '--rounds', '24']])
def test_example_runs(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'convergence.py')] + args,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    text = r.stdout.decode('utf-8', 'replace')
    assert r.returncode == 0, text
    assert text.count('rhat') == 2 and 'nan' not in text.lower(), text
