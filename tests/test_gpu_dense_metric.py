"""The dense-metric layer on the device (``csrc/dense_metric.hip``, ``HMCSampler(dense_metric=...)``)
against the host restatement ``tests/dense_metric_ref.py``, bit for bit: the five entry points
through the C ABI with every buffer carved out of a sentinel buffer, then the sampler and the
graph.

The leapfrog kernels tile the dimensions by 64, 128 or 256 (D <= 64, <= 128, beyond) with 4, 2
or 1 chain slots of up to 4 chains each, and the drift reads L through LDS tiles of 32, 16 or 8
columns: the shapes sit on every side of those, and beyond 128 dimensions on every regime that
``wide_regimes`` names (one to four i-tiles, ragged last tiles, 4, 3 and 2 chains per block), up
to the work-stride pass beyond 2^20 blocks.  The co-moments sum blocks of 64 chains of a group,
eight blocks per round (one to three rounds here), over 8 x 8 tiles of the lower triangle (up to
128 per side); the factor kernel is one workgroup of 16 waves per group (D up to 1024)."""
import numpy as np
import pytest
import torch

import dense_metric_ref as DM
import metric_ref as MR
from binf_amd import _native
from binf_amd.pdf import IsotropicGaussian
from binf_amd.samplers.hmc import HMCSampler
from oracle import c_oracle

pytestmark = pytest.mark.gpu

SENT = -7.25
GUARD = 66


def bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def ieee(a, b):
    """Bit for bit where both are numbers, NaN where the other is NaN."""
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and bool(np.array_equal(na, nb)) and bits(np.where(na, 0.0, a), np.where(nb, 0.0, b))


class Buf(object):
    """numpy ``x`` on the device inside a sentinel-filled buffer (``odd``: 8 bytes off 16-byte
    alignment); ``take()`` checks the guard zones and returns the values."""

    def __init__(self, x, device, odd=False, dtype=np.float64):
        x = np.ascontiguousarray(x, dtype=dtype)
        self.shape, self.n = x.shape, x.size
        self.before = GUARD + (1 if odd else 0)
        self.sent = SENT if dtype == np.float64 else -7
        self.whole = torch.full((self.before + self.n + GUARD,), self.sent, dtype=torch.from_numpy(x).dtype, device=device)
        self.view = self.whole[self.before:self.before + self.n]
        self.view.copy_(torch.from_numpy(x.reshape(-1)))
        self.ptr = self.view.data_ptr()

    def take(self):
        w = self.whole.cpu().numpy()
        assert np.all(w[:self.before] == self.sent) and np.all(w[self.before + self.n:] == self.sent), 'guard zone'
        return w[self.before:self.before + self.n].reshape(self.shape)


def some_groups(C):
    """1, a proper divisor if there is one, C."""
    mid = [g for g in range(2, C) if C % g == 0]
    return sorted(set([1] + mid[:1] + [C]))


def lower(rs, G, D, above=np.nan):
    """[G x D x D] factors: a random lower triangle, ``above`` (NaN: never to be read) above."""
    chol = np.tril(rs.standard_normal((G, D, D)) * rs.uniform(0.2, 5.0, size=(G, D, 1)))
    chol[:, np.triu(np.ones((D, D), dtype=bool), 1)] = above
    return chol


def dense_calls(device, q, p, g, chol, dt, dtc, mode, odd=False):
    """kick (half off / on), drift, kick_drift through the C ABI; {name: arrays}."""
    L, st = _native.lib(), _native.stream_handle(device)
    C, D = q.shape
    G = chol.shape[0]
    cb, gb = Buf(chol, device, odd), Buf(g, device, odd)
    db = None if dtc is None else Buf(dtc, device, odd)
    dptr = None if db is None else db.ptr
    out = {}
    for half in (0, 1):
        pb = Buf(p, device, odd)
        rc = L.binf_leapfrog_kick_dense_f64(pb.ptr, gb.ptr, cb.ptr, G, dt, dptr, half, C, D, mode, st)
        assert rc == 0, _native.last_error()
        out['kick%d' % half] = pb.take()
    qb, pb = Buf(q, device, odd), Buf(p, device, odd)
    rc = L.binf_leapfrog_drift_dense_f64(qb.ptr, pb.ptr, cb.ptr, G, dt, dptr, C, D, mode, st)
    assert rc == 0, _native.last_error()
    out['drift'] = qb.take()
    assert ieee(pb.take(), p)
    qb, pb = Buf(q, device, odd), Buf(p, device, odd)
    rc = L.binf_leapfrog_kick_drift_dense_f64(qb.ptr, pb.ptr, gb.ptr, cb.ptr, G, dt, dptr, C, D, mode, st)
    assert rc == 0, _native.last_error()
    out['kd_q'], out['kd_p'] = qb.take(), pb.take()
    assert ieee(gb.take(), g) and ieee(cb.take(), chol)
    return out


def dense_want(q, p, g, chol, dt, dtc, fma):
    kq, kp = DM.kick_drift(q, p, g, chol, dt, dtc, fma)
    return {'kick0': DM.kick(p, g, chol, dt, dtc, False, fma), 'kick1': DM.kick(p, g, chol, dt, dtc, True, fma),
            'drift': DM.drift(q, p, chol, dt, dtc, fma), 'kd_q': kq, 'kd_p': kp}


# ---------------------------------------------------------------------------
# the three leapfrog kernels
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('D', [1, 2, 7, 16, 17, 63, 64, 65, 130])
@pytest.mark.parametrize('C', [1, 3, 5, 130])
@pytest.mark.parametrize('mode', [_native.MODE_EXACT, _native.MODE_FMA])
def test_dense_kernels_equal_the_restatement(device, C, D, mode):
    """Scalar and per-chain steps, both kicks, G = 1, a divisor, C; NaN above every diagonal."""
    rs = np.random.RandomState(C * 1000 + D)
    q, p, g = rs.standard_normal((3, C, D))
    dtc = rs.uniform(0.01, 0.4, size=C)
    for G in some_groups(C):
        chol = lower(rs, G, D)
        for dt, dc in ((0.173, None), (0.0, dtc)):
            got = dense_calls(device, q, p, g, chol, dt, dc, mode)
            want = dense_want(q, p, g, chol, dt, dc, mode == _native.MODE_FMA)
            for k in want:
                assert np.isfinite(got[k]).all() and bits(got[k], want[k]), (k, G, dc is not None)


@pytest.mark.parametrize('mode', [_native.MODE_EXACT, _native.MODE_FMA])
def test_bases_eight_bytes_off_alignment(device, mode):
    rs = np.random.RandomState(5)
    C, D, G = 6, 66, 2
    q, p, g = rs.standard_normal((3, C, D))
    chol, dtc = lower(rs, G, D), rs.uniform(0.01, 0.4, size=C)
    got = dense_calls(device, q, p, g, chol, 0.0, dtc, mode, odd=True)
    want = dense_want(q, p, g, chol, 0.0, dtc, mode == _native.MODE_FMA)
    for k in want:
        assert bits(got[k], want[k]), k


def test_the_largest_dimension_and_the_first_refused(device):
    rs = np.random.RandomState(6)
    C, D = 2, 1024
    q, p, g = rs.standard_normal((3, C, D))
    chol = lower(rs, 1, D) / 32.0
    got = dense_calls(device, q, p, g, chol, 0.05, None, _native.MODE_EXACT)
    want = dense_want(q, p, g, chol, 0.05, None, False)
    for k in want:
        assert bits(got[k], want[k]), k
    L, st = _native.lib(), _native.stream_handle(device)
    D = 1025
    big = torch.zeros(D * D, dtype=torch.float64, device=device)
    v = [torch.ones(C * D, dtype=torch.float64, device=device) for _ in range(3)]
    assert L.binf_leapfrog_kick_dense_f64(v[0].data_ptr(), v[1].data_ptr(), big.data_ptr(), 1, 0.1, None, 0, C, D, 0,
                                          st) == _native.E_UNSUPPORTED
    assert L.binf_leapfrog_drift_dense_f64(v[0].data_ptr(), v[1].data_ptr(), big.data_ptr(), 1, 0.1, None, C, D, 0,
                                           st) == _native.E_UNSUPPORTED
    assert L.binf_leapfrog_kick_drift_dense_f64(v[0].data_ptr(), v[1].data_ptr(), v[2].data_ptr(), big.data_ptr(), 1, 0.1,
                                                None, C, D, 0, st) == _native.E_UNSUPPORTED
    with pytest.raises(NotImplementedError):
        _native.leapfrog_kick_dense(v[0].view(C, D), v[1].view(C, D), big.view(D, D), 0.1)
    torch.cuda.synchronize()
    assert all(bool((t == 1.0).all()) for t in v)                       # refused before anything is touched


# ---------------------------------------------------------------------------
# D = 129 ... 1024: i-tiles of 256 dimensions, one chain slot, R = CW = min(4, 2048 // D) chains
# per block, the drift's LDS tiles 8 columns wide
# ---------------------------------------------------------------------------
# (D, C, the values of G, bases 8 bytes off 16-byte alignment)
WIDE = [(129, 5, (1, 5), False), (191, 9, (1, 3, 9), False), (192, 4, (1, 2, 4), False), (193, 6, (1, 2, 6), False),
        (255, 6, (1, 2, 6), False), (256, 8, (1, 2, 8), False), (257, 9, (1, 3, 9), False), (300, 9, (1, 3, 9), True),
        (319, 4, (1, 2, 4), False), (320, 4, (1, 2, 4), True), (321, 5, (1, 5), False), (511, 5, (1, 5), False),
        (512, 9, (1, 3, 9), False), (513, 7, (1, 7), False), (682, 6, (1, 3), True), (683, 5, (1, 5), False),
        (769, 3, (1, 3), False), (1023, 7, (1, 7), False), (1024, 5, (1, 5), False)]


def wide_regimes(D, C, G, odd):
    """What the shape puts the launcher's geometry through, restated from ``csrc/dense_metric.hip``:
    a wave owns 64 consecutive dimensions jw .. jw + 63 of an i-tile, its kick walks the rows
    jw .. jd - 1 (jd = min(jw + 64, D)) under a predicate and the rows jd .. D - 1 in eights."""
    assert 128 < D <= 1024 and C % G == 0
    R, Cg, tiles = min(4, 2048 // D), C // G, -(-D // 256)
    last = D - 256 * (tiles - 1)
    met = {'%d i-tiles' % tiles, 'last i-tile of %d' % last}
    if last <= 192:
        met.add('a wave without a live lane')                   # the wave at 192 of the last i-tile
    if Cg > R and Cg % R:
        met.add('R = %d, a last block of fewer chains' % R)
    met.add('G = 1' if G == 1 else ('G = C' if G == C else 'G a proper divisor'))
    for jw in range(256, D, 64):                                # the waves of the second and later i-tiles
        jd = min(jw + 64, D)
        if jd < D:
            met.add('eight-row loop, %d rows left over' % ((D - jd) % 8))
    if odd and D > 256 and D % 2 == 0:
        met.add('bases off alignment')
    return met


WIDE_REGIMES = ['1 i-tiles', '2 i-tiles', '3 i-tiles', '4 i-tiles', 'last i-tile of 1', 'last i-tile of 63',
                'last i-tile of 64', 'last i-tile of 65', 'last i-tile of 255', 'a wave without a live lane',
                'R = 4, a last block of fewer chains', 'R = 3, a last block of fewer chains',
                'R = 2, a last block of fewer chains', 'G = 1', 'G a proper divisor', 'G = C',
                'eight-row loop, 0 rows left over', 'eight-row loop, 1 rows left over',
                'eight-row loop, 7 rows left over', 'bases off alignment']


def test_the_wide_shapes_meet_every_regime():
    """Every shape of WIDE runs in both modes and with both kinds of step, so a regime that one
    of them meets is met in all four."""
    met = set()
    for D, C, groups, odd in WIDE:
        for G in groups:
            met |= wide_regimes(D, C, G, odd)
    assert [r for r in WIDE_REGIMES if r not in met] == []


@pytest.mark.parametrize('D,C,groups,odd', WIDE, ids=['%dx%d' % (D, C) for D, C, _, _ in WIDE])
@pytest.mark.parametrize('mode', [_native.MODE_EXACT, _native.MODE_FMA])
def test_wide_dense_kernels_equal_the_restatement(device, D, C, groups, odd, mode):
    """Both kicks, drift and kick_drift with a scalar and a per-chain step; the factors scaled by
    1 / sqrt(D) (outputs stay finite), NaN above every diagonal."""
    rs = np.random.RandomState(C * 1000 + D)
    q, p, g = rs.standard_normal((3, C, D))
    dtc = rs.uniform(0.01, 0.4, size=C)
    for G in groups:
        chol = lower(rs, G, D) / np.sqrt(D)
        for dt, dc in ((0.173, None), (0.0, dtc)):
            got = dense_calls(device, q, p, g, chol, dt, dc, mode, odd=odd)
            want = dense_want(q, p, g, chol, dt, dc, mode == _native.MODE_FMA)
            for k in want:
                assert np.isfinite(got[k]).all() and bits(got[k], want[k]), \
                    (k, G, dc is not None, sorted(wide_regimes(D, C, G, odd)))


@pytest.mark.parametrize('mode', [_native.MODE_EXACT, _native.MODE_FMA])
def test_a_gradient_that_is_p_in_a_wide_kick(device, mode):
    """The one overlap that is served, ``grad == p`` exactly, where a block walks two i-tiles and
    writes p tile by tile: D = 300, C = 9 (R = 4; three blocks under G = 1, the last of one chain)."""
    L, st = _native.lib(), _native.stream_handle(device)
    C, D = 9, 300
    rs = np.random.RandomState(300)
    p = rs.standard_normal((C, D))
    dtc = rs.uniform(0.01, 0.4, size=C)
    for G in some_groups(C):
        chol = lower(rs, G, D) / np.sqrt(D)
        cb, db = Buf(chol, device), Buf(dtc, device)
        for dt, dc in ((0.173, None), (0.0, dtc)):
            for half in (0, 1):
                pb = Buf(p, device)
                rc = L.binf_leapfrog_kick_dense_f64(pb.ptr, pb.ptr, cb.ptr, G, dt, None if dc is None else db.ptr, half,
                                                    C, D, mode, st)
                assert rc == 0, _native.last_error()
                got = pb.take()
                want = DM.kick(p, p, chol, dt, dc, bool(half), mode == _native.MODE_FMA)
                assert np.isfinite(got).all() and bits(got, want), (G, dc is not None, half)
        assert ieee(cb.take(), chol) and bits(db.take(), dtc)


# ---------------------------------------------------------------------------
# more than 2^20 work items: the grid stops at 2^20 blocks and strides
# ---------------------------------------------------------------------------
def one_dimension_want(q, p, g, chol, dt, dtc, fma):
    """The contract at D = 1, one product per chain, over all chains at once (the restatement
    loops over the groups in Python): t = L g, p - d t; v = L p, q + v d; L = chol[c % G]."""
    C = q.shape[0]
    Lc = chol[np.arange(C) % chol.shape[0], 0]                  # [C x 1]
    d = np.full((C, 1), np.float64(dt)) if dtc is None else np.asarray(dtc, dtype=np.float64)[:, None]

    def kick(p, d):
        t = Lc * g
        return c_oracle.fma(-d, t, p) if fma else p - d * t

    def drift(q, p, d):
        v = Lc * p
        return c_oracle.fma(v, d, q) if fma else q + v * d
    pn = kick(p, d)
    return {'kick0': pn, 'kick1': kick(p, np.float64(0.5) * d), 'drift': drift(q, p, d), 'kd_q': drift(q, pn, d),
            'kd_p': pn}


@pytest.mark.parametrize('fma', [False, True])
def test_the_one_dimension_short_form_is_the_restatement(fma):
    rs = np.random.RandomState(48)
    C = 48
    q, p, g = rs.standard_normal((3, C, 1))
    dtc = rs.uniform(0.01, 0.4, size=C)
    for G in (1, 3, 48):
        chol = lower(rs, G, 1)
        for dt, dc in ((0.173, None), (0.0, dtc)):
            a, b = one_dimension_want(q, p, g, chol, dt, dc, fma), dense_want(q, p, g, chol, dt, dc, fma)
            for k in b:
                assert bits(a[k], b[k]), (k, G, dc is not None)


_stride_inputs = {}


def stride_inputs(C, G):
    """One set of inputs per shape, shared by the modes (16 M normals take their time)."""
    if (C, G) not in _stride_inputs:
        rs = np.random.RandomState(C % 1000 + G % 1000)
        q, p, g = rs.standard_normal((3, C, 1))
        _stride_inputs[C, G] = q, p, g, lower(rs, G, 1), rs.uniform(0.01, 0.4, size=C)
    return _stride_inputs[C, G]


@pytest.mark.parametrize('C,G,steps', [(2 ** 20 + 5, 2 ** 20 + 5, ('scalar', 'chain')), (16 * 2 ** 20 + 7, 1, ('chain',))],
                         ids=['one-chain-groups', 'one-group'])
@pytest.mark.parametrize('mode', [_native.MODE_EXACT, _native.MODE_FMA])
def test_the_work_stride_takes_a_second_pass(device, C, G, steps, mode):
    """D = 1: four chain slots of four chains, CW = 16.  2^20 + 5 groups of one chain are as many
    work items; 16 * 2^20 + 7 chains of one group are 2^20 + 1 blocks, the last of 7 chains."""
    D, CW = 1, 16
    nwork = G * -(-(C // G) // CW)
    assert nwork > 2 ** 20
    q, p, g, chol, dtc = stride_inputs(C, G)
    for step in steps:
        dt, dc = (0.173, None) if step == 'scalar' else (0.0, dtc)
        got = dense_calls(device, q, p, g, chol, dt, dc, mode)
        want = one_dimension_want(q, p, g, chol, dt, dc, mode == _native.MODE_FMA)
        for k in want:
            assert got[k].shape == (C, D) and np.isfinite(got[k]).all() and bits(got[k], want[k]), (k, step)


def test_the_upper_triangle_is_never_read(device):
    rs = np.random.RandomState(7)
    C, D, G = 6, 70, 2
    q, p, g = rs.standard_normal((3, C, D))
    clean = lower(rs, G, D, above=0.0)
    dirty = clean.copy()
    dirty[:, np.triu(np.ones((D, D), dtype=bool), 1)] = np.nan
    for mode in (_native.MODE_EXACT, _native.MODE_FMA):
        a = dense_calls(device, q, p, g, clean, 0.1, None, mode)
        b = dense_calls(device, q, p, g, dirty, 0.1, None, mode)
        for k in a:
            assert np.isfinite(b[k]).all() and bits(a[k], b[k]), k


@pytest.mark.parametrize('C,D', [(3, 7), (4, 64), (5, 130), (2, 300)])
@pytest.mark.parametrize('mode', [_native.MODE_EXACT, _native.MODE_FMA])
def test_identity_factor_equals_the_unscaled_entry_points(device, C, D, mode):
    rs = np.random.RandomState(D)
    q, p, g = (torch.from_numpy(a).to(device) for a in rs.standard_normal((3, C, D)))
    dtc = torch.from_numpy(rs.uniform(0.01, 0.4, size=C)).to(device)
    eye = torch.eye(D, dtype=torch.float64, device=device)
    for dt, dc in ((0.173, None), (0.0, dtc)):
        for half in (False, True):
            a, b = p.clone(), p.clone()
            _native.leapfrog_kick(a, g, dt, dc, half=half, mode=mode)
            _native.leapfrog_kick_dense(b, g, eye, dt, dc, half=half, mode=mode)
            assert torch.equal(a, b)
        a, b = q.clone(), q.clone()
        _native.leapfrog_drift(a, p, dt, dc, mode=mode)
        _native.leapfrog_drift_dense(b, p, eye.repeat(C, 1, 1), dt, dc, mode=mode)
        assert torch.equal(a, b)
        qa, pa, qb, pb = q.clone(), p.clone(), q.clone(), p.clone()
        _native.leapfrog_kick_drift(qa, pa, g, dt, dc, mode=mode)
        _native.leapfrog_kick_drift_dense(qb, pb, g, eye[None], dt, dc, mode=mode)
        assert torch.equal(qa, qb) and torch.equal(pa, pb)


def test_a_nan_stays_where_the_contract_puts_it(device):
    """A NaN in row r of L (column k <= r): t_k of the kick, v_r of the drift, in the chains of
    that group; after a kick_drift the new p_k is NaN and feeds v_i for every i >= k.  A NaN
    gradient element stays in its own chain."""
    rs = np.random.RandomState(9)
    C, D, G = 6, 10, 2
    q, p, g = rs.standard_normal((3, C, D))
    chol = lower(rs, G, D, above=0.0)
    clean = dense_calls(device, q, p, g, chol, 0.1, None, _native.MODE_EXACT)
    r, k = 6, 3
    bad = chol.copy()
    bad[1, r, k] = np.nan
    got = dense_calls(device, q, p, g, bad, 0.1, None, _native.MODE_EXACT)
    grp = np.zeros((C, 1), dtype=bool)
    grp[1::2] = True
    col, row, tail = (np.zeros((1, D), dtype=bool) for _ in range(3))
    col[0, k], row[0, r], tail[0, k:] = True, True, True
    hits = {'kick0': grp & col, 'kick1': grp & col, 'drift': grp & row, 'kd_p': grp & col, 'kd_q': grp & tail}
    for name, hit in hits.items():
        assert np.array_equal(np.isnan(got[name]), hit), name
        assert bits(np.where(hit, 0.0, got[name]), np.where(hit, 0.0, clean[name])), name
    g2 = g.copy()
    g2[4, 5] = np.nan
    got = dense_calls(device, q, p, g2, chol, 0.1, None, _native.MODE_EXACT)
    for name in ('kick0', 'kick1', 'kd_p', 'kd_q'):
        nan = np.isnan(got[name])
        assert nan[4].any() and not np.delete(nan, 4, axis=0).any(), name
        assert bits(np.delete(got[name], 4, axis=0), np.delete(clean[name], 4, axis=0)), name
    assert bits(got['drift'], clean['drift'])


def test_alias_refusals_leave_the_buffers_alone(device):
    L, st = _native.lib(), _native.stream_handle(device)
    C, D = 4, 8
    buf = torch.arange(4096, dtype=torch.float64, device=device)
    keep = buf.clone()
    base = buf.data_ptr()
    n, nl = C * D * 8, D * D * 8
    q, p, g, chol = base, base + 2 * n, base + 4 * n, base + 8 * n
    E = _native.E_ALIAS
    assert L.binf_leapfrog_kick_dense_f64(p, g, p + n - 8, 1, 0.1, None, 0, C, D, 0, st) == E
    assert L.binf_leapfrog_kick_dense_f64(p, p + 8, chol, 1, 0.1, None, 0, C, D, 0, st) == E
    assert L.binf_leapfrog_kick_dense_f64(p, g, chol, 1, 0.1, p + 16, 0, C, D, 0, st) == E
    assert L.binf_leapfrog_drift_dense_f64(q, q + 8, chol, 1, 0.1, None, C, D, 0, st) == E
    assert L.binf_leapfrog_drift_dense_f64(q, p, q - nl + 8, 1, 0.1, None, C, D, 0, st) == E
    assert L.binf_leapfrog_kick_drift_dense_f64(q, p, q, chol, 1, 0.1, None, C, D, 0, st) == E
    assert L.binf_leapfrog_kick_drift_dense_f64(q, q + n - 8, g, chol, 1, 0.1, None, C, D, 0, st) == E
    assert L.binf_metric_comoments_f64(q, q + n - 8, p, chol, 1, C, D, 1, st) == E
    assert L.binf_metric_factor_f64(q, chol, 3, C, D, 1, 1, chol + 8, p, None, st) == E
    assert L.binf_metric_factor_f64(q, chol, 3, C, D, 1, 1, g, g + nl - 8, None, st) == E
    # a gradient that IS p (exactly) is the one overlap that is served
    pg = torch.from_numpy(np.random.RandomState(1).standard_normal((C, D))).to(device)
    eye = torch.eye(D, dtype=torch.float64, device=device)
    want = pg - 0.1 * pg
    assert L.binf_leapfrog_kick_dense_f64(pg.data_ptr(), pg.data_ptr(), eye.data_ptr(), 1, 0.1, None, 0, C, D, 0, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(pg, want) and torch.equal(buf, keep)


# ---------------------------------------------------------------------------
# co-moments, factor
# ---------------------------------------------------------------------------
def check_comoments(device, Cg, G, dims):
    """Five draws with the `first` toggles, then a new window; what lies above the diagonal of
    s2 stays as it was."""
    C = Cg * G
    L, st = _native.lib(), _native.stream_handle(device)
    for D in dims:
        rs = np.random.RandomState(Cg * 7 + G + D)
        x = 10.0 + rs.standard_normal((5, C, D)) * rs.uniform(0.1, 20.0, size=(1, 1, D)) + rs.standard_normal((1, C, D))
        want = DM.CoMoments(G, above=3.5)
        k0, s1 = Buf(np.full((G, D), 3.5), device), Buf(np.full((G, D), 3.5), device, odd=True)       # no initialisation needed
        s2 = Buf(np.full((G, D, D), 3.5), device)
        for t in range(5):
            xb = Buf(x[t], device, odd=t % 2 == 1)
            rc = L.binf_metric_comoments_f64(xb.ptr, k0.ptr, s1.ptr, s2.ptr, int(t == 0), C, D, G, st)
            assert rc == 0, _native.last_error()
            want.add(x[t], first=t == 0)
            if t + 1 in (1, 2, 5):                                                                # n = 1, 2, 5
                assert bits(xb.take(), x[t])
                assert bits(k0.take(), want.k0) and bits(s1.take(), want.s1) and bits(s2.take(), want.s2), (D, t + 1)
        # a new window: `first` forgets the old one, above the diagonal stays untouched
        xb = Buf(x[2], device)
        assert L.binf_metric_comoments_f64(xb.ptr, k0.ptr, s1.ptr, s2.ptr, 1, C, D, G, st) == 0
        want.add(x[2], first=True)
        assert bits(k0.take(), want.k0) and bits(s1.take(), want.s1) and bits(s2.take(), want.s2)


# eight waves sum eight blocks of 64 chains per round, wave 0 carries the total on: 512 is one full
# round, 513 a second round of one block (of one chain), 577 of two blocks, 1100 three rounds
# (18 blocks) with a last block of 12 chains
@pytest.mark.parametrize('Cg', [1, 2, 63, 64, 65, 130, 330, 512, 513, 577, 1100])
@pytest.mark.parametrize('G', [1, 3])
def test_comoments_equal_the_restatement(device, Cg, G):
    check_comoments(device, Cg, G, (1, 7, 65))


# 17 and 33 tiles of 8 x 8 per side, then the most there can be: 128 per side, 8256 workgroups
@pytest.mark.parametrize('Cg,G,D', [(3, 1, 129), (3, 2, 129), (70, 1, 129), (70, 2, 129), (3, 1, 257), (3, 2, 257),
                                    (70, 1, 257), (70, 2, 257), (3, 1, 1024)])
def test_comoments_equal_the_restatement_at_wide_dimensions(device, Cg, G, D):
    check_comoments(device, Cg, G, (D,))


def moments_for(rs, n, C, D, G):
    """(s1, s2) of a correlated record, s2 with NaN above the diagonal."""
    A = rs.standard_normal((D, D)) * rs.uniform(0.2, 3.0, size=(D, 1))
    x = 4.0 + rs.standard_normal((n, C, D)) @ A.T
    m = DM.CoMoments(G, above=np.nan)
    for xt in x:
        m.add(xt)
    return m.s1, m.s2


def run_factor(device, s1, s2, n, C, reg, prev, with_status=True):
    L, st = _native.lib(), _native.stream_handle(device)
    G, D = s1.shape
    b1, b2, cb = Buf(s1, device), Buf(s2, device, odd=True), Buf(prev, device)
    wb, sb = Buf(np.full((G, D, D), 9.5), device, odd=True), Buf(np.full(G, 77), device, dtype=np.int32)
    rc = L.binf_metric_factor_f64(b1.ptr, b2.ptr, n, C, D, G, reg, cb.ptr, wb.ptr, sb.ptr if with_status else None, st)
    assert rc == 0, _native.last_error()
    assert ieee(b1.take(), s1) and ieee(b2.take(), s2)
    return cb.take(), wb.take(), sb.take()


def moments_direct(rs, N, D, G, flat=None):
    """(s1, s2) of N pooled draws, written down instead of streamed (the factor is a function of
    s1, s2, n and C alone): s2 = (N - 1) Sigma + s1 s1^T / N with Sigma = B B^T / D + I, eigenvalues
    in [1, 5] or so; NaN above the diagonal.  ``flat = (group, i)``: row and column i of that
    group's Sigma are zero, and the second term is formed as the contract subtracts it, so the
    covariance of dimension i with every dimension is 0.0 exactly."""
    B, I = rs.standard_normal((G, D, D)), np.eye(D)[None].repeat(G, 0)
    if flat is not None:
        B[flat[0], flat[1], :] = 0.0
        I[flat[0], flat[1], flat[1]] = 0.0
    sigma = B @ B.transpose(0, 2, 1) / D + I
    s1 = rs.standard_normal((G, D)) * (2.0 * np.sqrt(N))
    s2 = np.float64(N - 1) * sigma + (s1[:, :, None] * s1[:, None, :]) / np.float64(N)
    s2[:, np.triu(np.ones((D, D), dtype=bool), 1)] = np.nan
    return s1, s2


def check_factor(device, D, G, reg):
    rs = np.random.RandomState(D + reg)
    Cg, n = 5, 2 * D + 3
    C = G * Cg
    s1, s2 = moments_for(rs, n, C, D, G) if D <= 130 else moments_direct(rs, n * Cg, D, G)
    prev = rs.standard_normal((G, D, D))
    want_chol, want_work, want_status = DM.factor(s1, s2, n, C, bool(reg), prev)
    assert want_status.tolist() == [0] * G
    chol, work, status = run_factor(device, s1, s2, n, C, reg, prev)
    assert bits(chol, want_chol) and bits(work, want_work) and bits(status, want_status)
    up = np.triu(np.ones((D, D), dtype=bool), 1)
    assert np.all(chol[:, up] == 0.0) and not np.signbit(chol[:, up]).any()                 # +0.0 above
    assert np.all(chol[:, np.eye(D, dtype=bool)] > 0.0)
    cov = DM.covariance(s1, s2, n, C, bool(reg))
    assert np.allclose(np.tril(chol[0] @ chol[0].T), cov[0], rtol=1e-9, atol=1e-12)
    assert bits(run_factor(device, s1, s2, n, C, reg, prev, with_status=False)[0], want_chol)   # status may be NULL


# up to 130 the moments are streamed through the restatement, beyond they are written down
@pytest.mark.parametrize('D', [1, 2, 3, 8, 33, 64, 65, 130, 131, 257, 513])
@pytest.mark.parametrize('reg', [0, 1])
def test_factor_equals_the_restatement(device, D, reg):
    check_factor(device, D, 2, reg)


def test_factor_equals_the_restatement_at_the_largest_dimension(device):
    check_factor(device, 1024, 1, 1)


def test_a_group_without_a_factor_keeps_its_own(device):
    rs = np.random.RandomState(17)
    G, Cg, n, D = 2, 6, 9, 12
    C = G * Cg
    A = rs.standard_normal((D, D))
    x = rs.standard_normal((n, C, D)) @ A.T
    prev = rs.standard_normal((G, D, D))
    # a constant dimension in group 1: variance 0 without the shrinkage, 1e-3 * 5 / (N + 5) with it
    xc = x.copy()
    xc[:, 1::2, 4] = 1.25
    flat, m = DM.comoments(xc, G), DM.comoments(x, G)
    # a NaN moment in group 0 only
    s2 = m.s2.copy()
    s2[0, 7, 2] = np.nan
    check_kept_factors(device, flat.s1, flat.s2, m.s1, s2, n, C, prev)


def test_a_wide_group_without_a_factor_keeps_its_own(device):
    """D = 257: 16 waves share 257 rows, the column of a step goes through LDS in one piece."""
    rs = np.random.RandomState(18)
    G, Cg, n, D = 2, 6, 100, 257
    C = G * Cg
    prev = rs.standard_normal((G, D, D))
    f1, f2 = moments_direct(rs, n * Cg, D, G, flat=(1, 200))
    s1, s2 = moments_direct(rs, n * Cg, D, G)
    s2[0, 250, 3] = np.nan
    check_kept_factors(device, f1, f2, s1, s2, n, C, prev)


def check_kept_factors(device, f1, f2, s1, s2, n, C, prev):
    """(f1, f2): a dimension of variance zero in group 1 -- reg 0 flags it, reg 1 does not;
    (s1, s2): a NaN moment in group 0.  Flags, kept factor and work buffer are the restatement's."""
    D = f1.shape[1]
    for reg, flags in ((0, [0, 1]), (1, [0, 0])):
        want = DM.factor(f1, f2, n, C, bool(reg), prev)
        assert want[2].tolist() == flags
        chol, work, status = run_factor(device, f1, f2, n, C, reg, prev)
        assert bits(chol, want[0]) and ieee(work, want[1]) and bits(status, want[2])
        if reg == 0:
            assert bits(chol[1], prev[1]) and not bits(chol[0], prev[0])
    want = DM.factor(s1, s2, n, C, True, prev)
    assert want[2].tolist() == [1, 0]
    chol, work, status = run_factor(device, s1, s2, n, C, 1, prev)
    assert bits(chol, want[0]) and ieee(work, want[1]) and bits(status, want[2])
    assert bits(chol[0], prev[0]) and np.isfinite(chol[1]).all()
    up = np.triu(np.ones((D, D), dtype=bool), 1)
    assert np.all(work[:, up] == 0.0) and not np.signbit(work[:, up]).any()


# ---------------------------------------------------------------------------
# the sampler
# ---------------------------------------------------------------------------
def draws(n, C, D, seed):
    rs = np.random.RandomState(seed)
    return rs.standard_normal((n, C, D)), rs.uniform(size=(n, C))


def well_conditioned(rs, G, D):
    chol = np.tril(rs.standard_normal((G, D, D))) * (0.3 / np.sqrt(D))
    chol[:, np.eye(D, dtype=bool)] = rs.uniform(0.5, 1.5, size=(G, D))
    return chol


def check_sampler(device, mode, graph, C, D, G):
    nT = 4
    rs = np.random.RandomState(11)
    q0 = rs.standard_normal((C, D)) * 1.5
    chol = well_conditioned(rs, G, D)
    p0, u = draws(nT, C, D, 12)
    ref = DM.DenseHMC(MR.GaussTarget(2.5, 0.25), q0, 0.11, 4, chol, adaption_limit=10, fma=mode == 'fma')
    junk = torch.from_numpy(chol + np.triu(np.full((D, D), 7.0), 1)).to(device)              # above: ignored
    s = HMCSampler(IsotropicGaussian(k=2.5, x0=0.25), torch.from_numpy(q0).to(device), 0.11, 4,
                   timestep_adaption_limit=10, variable_name='x', mode=mode, record_energies=True, graph=graph,
                   dense_metric=junk)
    assert bits(s.metric_chol.cpu().numpy(), chol) and s._fused_spec('x', D, C) is None
    assert torch.equal(s.inverse_mass, s.metric_chol @ s.metric_chol.transpose(1, 2))
    for t in range(nT):
        x = s.sample(p0=torch.from_numpy(p0[t]).to(device), u=torch.from_numpy(u[t]).to(device))
        want = ref.sample(p0[t], u[t])
        assert bits(x.cpu().numpy(), want), t
        assert np.array_equal(s.last_move_accepted.cpu().numpy(), ref.accepted)
        assert bits(s.last_e_before.cpu().numpy(), ref.e_before) and bits(s.last_e_after.cpu().numpy(), ref.e_after)
        assert bits(s.timestep.cpu().numpy(), ref.dt_chain) and s.counter == ref.counter
        assert np.array_equal(s.n_accepted.cpu().numpy(), ref.n_accepted)
    if graph:
        assert s._graph_captures == 1
        # a window end rewrites the factor in place: same address, no new capture, new bits
        s.set_dense_metric(torch.from_numpy(chol * 1.25).to(device))
        ref.chol = chol * 1.25
        p1, u1 = draws(1, C, D, 13)
        x = s.sample(p0=torch.from_numpy(p1[0]).to(device), u=torch.from_numpy(u1[0]).to(device))
        assert bits(x.cpu().numpy(), ref.sample(p1[0], u1[0])) and s._graph_captures == 1
    d = s.state_dict()
    assert torch.equal(d['metric_chol'], s.metric_chol) and 'metric_scale' not in d


@pytest.mark.parametrize('mode', ['exact', 'fma'])
@pytest.mark.parametrize('graph', [False, 'always'])
def test_sampler_equals_the_restated_transition(device, mode, graph):
    check_sampler(device, mode, graph, 6, 33, 3)


@pytest.mark.parametrize('mode', ['exact', 'fma'])
@pytest.mark.parametrize('graph', [False, 'always'])
def test_sampler_equals_the_restated_transition_on_a_wide_tile(device, mode, graph):
    """D = 193: one i-tile of 256 with a ragged fourth wave; three groups of three chains, R = 4."""
    check_sampler(device, mode, graph, 9, 193, 3)


def test_identity_metric_equals_the_per_step_tier_without_one(device):
    C, D, nT = 5, 40, 3
    q0 = torch.from_numpy(np.random.RandomState(1).standard_normal((C, D))).to(device)
    p0, u = draws(nT, C, D, 2)
    a = HMCSampler(IsotropicGaussian(), q0.clone(), 0.2, 5, 10, variable_name='x', record_energies=True,
                   dense_metric=torch.eye(D, dtype=torch.float64, device=device))
    b = HMCSampler(IsotropicGaussian(), q0.clone(), 0.2, 5, 10, variable_name='x', record_energies=True)
    b.fused_transition = False
    for t in range(nT):
        pt, ut = torch.from_numpy(p0[t]).to(device), torch.from_numpy(u[t]).to(device)
        assert torch.equal(a.sample(p0=pt, u=ut), b.sample(p0=pt, u=ut))
        assert torch.equal(a.last_e_after, b.last_e_after) and torch.equal(a.timestep, b.timestep)


def test_sample_n_equals_single_calls(device):
    C, D, n = 4, 16, 5
    rs = np.random.RandomState(3)
    q0 = torch.from_numpy(rs.standard_normal((C, D))).to(device)
    chol = torch.from_numpy(well_conditioned(rs, 2, D)).to(device)
    p0, u = draws(n, C, D, 5)
    a = HMCSampler(IsotropicGaussian(), q0.clone(), 0.2, 3, variable_name='x', dense_metric=chol)
    b = HMCSampler(IsotropicGaussian(), q0.clone(), 0.2, 3, variable_name='x', dense_metric=chol)
    rec = a.sample_n(n, thin=2, p0=torch.from_numpy(p0).to(device), u=torch.from_numpy(u).to(device))
    singles = [b.sample(p0=torch.from_numpy(p0[t]).to(device), u=torch.from_numpy(u[t]).to(device)) for t in range(n)]
    assert torch.equal(rec, torch.stack([singles[1], singles[3]])) and torch.equal(a.state, b.state)
    assert torch.equal(a.n_accepted, b.n_accepted)


def test_reversibility_inside_a_propagated_rounding_bound(device):
    """L_ steps, negate r, L_ steps returns to the start.  Target N(0, I) (gradient = q, exact),
    so a kick is r -= d L^T q and a drift q += d L r: linear maps of infinity-norm at most
    1 + a, a = d * max(|L|_inf, |L|_1) (absolute row and column sums).  One update commits, per
    element, at most D roundings in the dot product (gamma_D relative to sum |L||x| <= (a / d) M),
    the product with d and the sum: a local error of at most (gamma_D + 2 u (1 + gamma_D)) (1 + a) M
    <= (D + 3) u (1 + a) M, M the largest |q|, |r| on the way.  Forth and back are
    2 (2 L_ + 1) updates, each local error grows by at most (1 + a) per later update:
        |return - start| <= 2 (2 L_ + 1) (D + 3) u (1 + a) M (1 + a)^(2 (2 L_ + 1))."""
    C, D, L_, dt = 7, 66, 4, 0.1
    rs = np.random.RandomState(21)
    chol = np.tril(rs.standard_normal((1, D, D))) * (0.1 / np.sqrt(D))              # weak couplings: a stays small
    chol[:, np.eye(D, dtype=bool)] = rs.uniform(0.5, 1.5, size=(1, D))
    q0, p0 = rs.standard_normal((2, C, D))
    s = HMCSampler(IsotropicGaussian(), torch.from_numpy(q0).to(device), dt, L_, variable_name='x',
                   dense_metric=torch.from_numpy(chol).to(device))
    q, p = torch.from_numpy(q0).to(device), torch.from_numpy(p0).to(device)
    s._leapfrog(q, p, dt, L_)
    mid = max(float(q.abs().max()), float(p.abs().max()))
    assert float((q - torch.from_numpy(q0).to(device)).abs().max()) > 0.1            # it went somewhere
    p.neg_()
    s._leapfrog(q, p, dt, L_)
    a = dt * max(float(np.abs(chol[0]).sum(axis=1).max()), float(np.abs(chol[0]).sum(axis=0).max()))
    M = 2.0 * max(mid, float(np.abs(q0).max()), float(np.abs(p0).max()))             # H-bounded orbit, with room
    nu = 2 * (2 * L_ + 1)
    bound = nu * (D + 3) * 2.0 ** -53 * (1 + a) * M * (1 + a) ** nu
    err = max(float((q.cpu() - torch.from_numpy(q0)).abs().max()), float((-p.cpu() - torch.from_numpy(p0)).abs().max()))
    print('reversibility: error %.3g, bound %.3g' % (err, bound))
    assert bound < 1e-9 and err <= bound


def test_the_two_metrics_exclude_each_other(device):
    D = 4
    q0 = torch.zeros(2, D, dtype=torch.float64, device=device)
    one, eye = torch.ones(D, dtype=torch.float64, device=device), torch.eye(D, dtype=torch.float64, device=device)
    with pytest.raises(ValueError):
        HMCSampler(IsotropicGaussian(), q0, 0.1, 2, variable_name='x', metric=one, dense_metric=eye)
    s = HMCSampler(IsotropicGaussian(), q0, 0.1, 2, variable_name='x', metric=one)
    with pytest.raises(ValueError):
        s.set_dense_metric(eye)
    s = HMCSampler(IsotropicGaussian(), q0, 0.1, 2, variable_name='x', dense_metric=eye)
    with pytest.raises(ValueError):
        s.set_metric(one)
    for bad in (one, eye[:3], eye.float(), torch.eye(D, dtype=torch.float64), eye.repeat(3, 1, 1)):
        with pytest.raises(ValueError):
            s.set_dense_metric(bad)
    s.set_dense_metric(None)
    assert s.metric_chol is None and s.inverse_mass is None
    s.set_metric(one)                                                   # free again
