"""csrc/free_energy.hip on the device: the work record bit for bit against the host
restatement (tests/free_energy_ref.py), the BAR estimator against the restatement within
derived bounds and against exact arithmetic, its determinism, its edge contract, the
sampler's record, and the harmonic ladder end to end.

Bounds.  The two sides run the same additions in the same order and differ in exp / log
only, each within an ulp (2^-52 relative) of the true value on either side.
  * delta_forward / delta_reverse = (M + log(total)) - log n: ``FE.average_bound`` =
    16 * 2^-52 * (1 + |value| + log n) + n * 2^-52, the additive form: the n terms exp(x - m)
    <= 1 and the chunk factors, an ulp apart on the two sides, move total >= 1 and with it
    log(total) by n * 2^-52 absolute at the most; the additions, the two logs and the three
    roundings of values <= 1 + |value| + log n give the small multiple (derivation with
    ``FE.average_bound``; the restatement is held to the same bound against mpmath on the CPU).
  * delta: an error e_g in g moves the root by e_g / S (``FE.g_error_bound``, derived in
    tests/test_free_energy.py, which also holds the restatement inside ONE ``FE.delta_bound``
    of the exact root); the device is allowed the same, so the two sides differ by at most
    2 * delta_bound, S from the restatement.
  * info = S: 2 n terms <= 1/4, each off by 4 ulp between the sides (one exp, 1 + t, its
    square, one divide), plus the move of delta times |dS/dD| <= S: ``FE.info_bound`` =
    n * 8 * 2^-52 + 2 * delta_bound * S.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

import free_energy_ref as FE
import replica_exchange as RX
from binf_amd import _native, checkpoint, free_energy
from binf_amd.samplers.hmc import HMCSampler
from binf_amd.samplers.replica import ReplicaExchangeSampler
from binf_amd.samplers.rng import DeviceRNG
from conftest import ROOT
from test_gpu_replica_exchange import (Harmonic, R_S, ROUNDS, build_inner, carve, dev, draws, guards_intact,
                                       ptr, same_bits, SENT)

pytestmark = pytest.mark.gpu

FLOATS = ('delta', 'delta_forward', 'delta_reverse', 'info')


def bits(t):
    """The bytes of a tensor (NaNs compare by their bits)."""
    return t.contiguous().cpu().numpy().tobytes()


def chunk():
    c = _native.free_energy_chunk()
    assert c == FE.header_chunk()
    return c


# ---------------------------------------------------------------------------
# the work row through the C ABI
# ---------------------------------------------------------------------------
def call_work(L, lp_own, lp_sw, w, C, R, parity, device):
    return L.binf_replica_work_f64(ptr(lp_own), ptr(lp_sw), ptr(w), C, R, parity, _native.stream_handle(device))


@pytest.mark.parametrize('n_ladders', [1, 3])
@pytest.mark.parametrize('R', [1, 2, 3, 4, 5])
def test_work_row_bits_against_the_restatement(device, R, n_ladders):
    L = _native.lib()
    C = R * n_ladders
    rs = np.random.RandomState(100 * R + n_ladders)
    lp_own, lp_sw = rs.standard_normal(C) * 3.0 - 20.0, rs.standard_normal(C) * 3.0 - 20.0
    lp_own[rs.randint(C)] = -np.inf
    lp_sw[rs.randint(C)] = -np.inf
    for parity in (0, 1):
        want = FE.work_row(lp_own, lp_sw, R, parity)
        wd, whole = carve(np.full(C, SENT), device, before=5, after=4)
        assert call_work(L, dev(lp_own, device), dev(lp_sw, device), wd, C, R, parity, device) == 0, _native.last_error()
        got = wd.cpu().numpy()
        assert guards_intact(whole, 5, C)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        unpaired = FE.partner_or_minus_one(C, R, parity) < 0
        assert np.all(np.isnan(got[unpaired])) and unpaired.sum() == np.isnan(FE.work_row(np.zeros(C), np.zeros(C), R, parity)).sum()
        ok = ~np.isnan(want)
        assert same_bits(got[ok], want[ok]), (R, n_ladders, parity)


def test_work_row_refusals_leave_the_row_untouched(device):
    L = _native.lib()
    C, R = 6, 3
    lp = dev(np.zeros(C), device)
    lp2 = dev(np.ones(C), device)
    w = dev(np.full(C, SENT), device)
    for args in [(lp, lp2, w, C, 4, 0), (lp, lp2, w, C, R, 2), (lp, lp2, w, C, R, -1), (lp, lp2, w, C, 0, 0),
                 (None, lp2, w, C, R, 0), (lp, None, w, C, R, 0), (lp, lp2, w, -1, R, 0)]:
        assert call_work(L, *args, device) == _native.E_ARG, args[3:]
        torch.cuda.synchronize()
        assert np.all(w.cpu().numpy() == SENT)
    assert call_work(L, lp, lp2, None, C, R, 0, device) == _native.E_ARG
    assert call_work(L, w, lp2, w, C, R, 0, device) == _native.E_ALIAS
    assert call_work(L, None, None, None, 0, R, 0, device) == 0
    assert np.all(w.cpu().numpy() == SENT)


# ---------------------------------------------------------------------------
# the estimator against the restatement
# ---------------------------------------------------------------------------
def random_record(T, C, R, first_round, seed, stride=None):
    """A record as the sampler writes it (NaN at unpaired positions, overlapping u and v
    populations), on the host, inside rows of ``stride`` elements (sentinel between rows)."""
    rs = np.random.RandomState(seed)
    stride = C if stride is None else stride
    whole = np.full((max(T, 1), stride), np.nan)
    rec = whole[:T, :C]
    shift = 0.7 * (np.arange(C) % R)
    for t in range(T):
        p = FE.partner_or_minus_one(C, R, (first_round + t) & 1)
        row = rs.standard_normal(C) * 1.5 + np.where(np.arange(C) % 2 == 0, -1.0, 0.4) - shift
        rec[t] = np.where(p >= 0, row, np.nan)
    return whole, rec


def compare(got, want, what):
    """Integers and status equal; floats inside the bounds of the module docstring."""
    got = dict((k, v.cpu().numpy()) for k, v in got.items())
    for k in ('n', 'n_invalid', 'status'):
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    G, P = want['n'].shape
    for g in range(G):
        for r in range(P):
            n, st = int(want['n'][g, r]), int(want['status'][g, r])
            for k in FLOATS:
                a, b = float(got[k][g, r]), float(want[k][g, r])
                if not np.isfinite(b):
                    assert (np.isnan(a) and np.isnan(b)) or a == b, (what, g, r, k, a, b)
            if st != FE.OK:
                continue
            for k in ('delta_forward', 'delta_reverse'):
                a, b = float(got[k][g, r]), float(want[k][g, r])
                tol = FE.average_bound(n, b)
                assert abs(a - b) <= tol, (what, g, r, k, a, b, tol)
            S = float(want['info'][g, r])
            tol = 2.0 * FE.delta_bound(n, S, float(want['delta'][g, r]), chunk()) if S > 0 else 0.0
            a, b = float(got['delta'][g, r]), float(want['delta'][g, r])
            assert abs(a - b) <= tol, (what, g, r, 'delta', a, b, tol)
            tol_s = FE.info_bound(n, S, tol)
            assert abs(float(got['info'][g, r]) - S) <= tol_s, (what, g, r, 'info')
    return got


@pytest.mark.parametrize('R', [2, 3, 6])
@pytest.mark.parametrize('n_ladders', [1, 3])
def test_small_shapes_against_the_restatement(device, R, n_ladders):
    C = R * n_ladders
    for T in (1, 2, 7):
        for first_round in (0, 1):
            for stride in (C, C + 5):
                whole, rec = random_record(T, C, R, first_round, 1000 * R + 10 * T + first_round, stride)
                view = dev(whole, device)[:T, :C]
                assert view.is_contiguous() == (stride == C or T <= 1)
                for G in sorted({1, n_ladders}):
                    want = FE.bar(rec, R, first_round, G)
                    got = _native.free_energy_bar(view, R, first_round, G)
                    compare(got, want, (T, first_round, stride, G))


def two_slot_record(n, seed):
    """C = R = 2: pair 0 lives in the even rows of a record started at round 0; n samples need
    2 n - 1 rows."""
    whole, rec = random_record(2 * n - 1, 2, 2, 0, seed)
    return rec


@pytest.mark.parametrize('offset', [-1, 0, 1, None])
def test_sample_counts_around_the_chunk(device, offset):
    n = 2 * chunk() + 1 if offset is None else chunk() + offset
    rec = two_slot_record(n, 50 + n % 7)
    assert rec.nbytes < 2 ** 19
    want = FE.bar(rec, 2, 0, 1)
    assert want['n'][0, 0] == n and want['status'][0, 0] == FE.OK
    got = compare(_native.free_energy_bar(dev(rec, device), 2, 0, 1), want, n)
    print('n %d: delta %.17g (restated %.17g), forward %.6f, reverse %.6f'
          % (n, got['delta'][0, 0], want['delta'][0, 0], got['delta_forward'][0, 0], got['delta_reverse'][0, 0]))


def test_delta_brackets_the_exact_root(device):
    """Independent of the restatement: mpmath's g changes sign inside [delta - tol, delta +
    tol], tol = e_g / S + 2 ulp with S from mpmath at the device's delta."""
    R, n_ladders, T = 3, 3, 40
    _, rec = random_record(T, R * n_ladders, R, 1, 4242)
    rec[3, 0] = -np.inf                                   # a sample of weight 0 among them
    for G in (1, 3):
        got = _native.free_energy_bar(dev(rec, device), R, 1, G)
        delta = got['delta'].cpu().numpy()
        assert np.all(got['status'].cpu().numpy() == FE.OK)
        for g in range(G):
            for r in range(R - 1):
                u, v = FE.problem_samples(rec, R, 1, G, g, r)
                d = float(delta[g, r])
                S = float(FE.exact_g(u, v, d)[1])
                tol = FE.delta_bound(u.shape[0], S, d, chunk())
                mp = FE._mp()
                g_lo = FE.exact_g(u, v, mp.mpf(d) - mp.mpf(tol))[0]
                g_hi = FE.exact_g(u, v, mp.mpf(d) + mp.mpf(tol))[0]
                assert g_lo < 0 < g_hi, (G, g, r, d, tol)


def test_groups_strides_and_places_give_the_same_bits(device):
    R, n_ladders, T, G = 3, 6, 9, 3
    C = R * n_ladders
    whole, rec = random_record(T, C, R, 0, 99, stride=C + 3)
    strided = dev(whole, device)[:T, :C]
    packed = dev(rec, device)
    a = _native.free_energy_bar(strided, R, 0, G)
    b = _native.free_energy_bar(packed, R, 0, G)
    for k in a:
        assert same_bits(a[k].cpu().numpy(), b[k].cpu().numpy()), k
    Lg = n_ladders // G
    for g in range(G):
        alone = np.ascontiguousarray(rec[:, g * Lg * R:(g + 1) * Lg * R])
        one = _native.free_energy_bar(dev(alone, device), R, 0, 1)
        for k in a:
            assert same_bits(a[k][g].cpu().numpy(), one[k][0].cpu().numpy()), (g, k)


def test_edge_contract(device):
    R, n_ladders, T = 3, 2, 6
    C = R * n_ladders
    _, rec = random_record(T, C, R, 0, 7)
    # ladder 0 (group 0 of 2): pair 0 has -inf samples among finite ones, pair 1 a NaN and a +inf
    rec[0, 0] = -np.inf
    rec[2, 1] = -np.inf
    rec[1, 1] = np.nan
    rec[3, 2] = np.inf
    # ladder 1 (group 1): pair 0 has no finite u, pair 1 no finite sample at all
    rec[0::2, 3] = -np.inf
    rec[1::2, 4] = -np.inf
    rec[1::2, 5] = -np.inf
    want = FE.bar(rec, R, 0, 2)
    assert want['status'].tolist() == [[FE.OK, FE.INVALID], [FE.ONE_SIDED, FE.NO_FINITE]]
    got = compare(_native.free_energy_bar(dev(rec, device), R, 0, 2), want, 'edges')
    assert got['n_invalid'].tolist() == [[0, 2], [0, 0]]
    assert all(np.isnan(got[k][0, 1]) for k in FLOATS) and np.isfinite(got['delta'][0, 0])
    assert got['delta_forward'][1, 0] == -np.inf and got['delta'][1, 0] == -np.inf and got['info'][1, 0] == 0.0
    assert np.isfinite(got['delta_reverse'][1, 0])
    assert got['delta_forward'][1, 1] == -np.inf and got['delta_reverse'][1, 1] == np.inf and np.isnan(got['delta'][1, 1])
    # an unpaired position's NaN is never a sample: every other problem is fine above
    # T = 0 and a parity without rows: n = 0, NaN, a status of its own
    for T0 in (0, 1):
        e = _native.free_energy_bar(dev(rec[:T0], device), R, 0, 1)
        ne = FE.bar(rec[:T0], R, 0, 1)
        compare(e, ne, 'T=%d' % T0)
        assert int(e['status'][0, 1]) == FE.EMPTY and int(e['n'][0, 1]) == 0
        assert bool(torch.isnan(e['delta'][0, 1]))
    # R = 1: empty outputs, success
    e = _native.free_energy_bar(dev(np.zeros((4, 3)), device), 1, 0, 1)
    assert all(tuple(v.shape) == (1, 0) for v in e.values())
    # identical slots: exact zeros
    z = _native.free_energy_bar(dev(np.zeros((2 * chunk() + 2, 2)), device), 2, 0, 1)
    assert float(z['delta'][0, 0]) == 0.0 and float(z['delta_forward'][0, 0]) == 0.0
    assert float(z['delta_reverse'][0, 0]) == 0.0 and int(z['status'][0, 0]) == FE.OK
    assert float(z['info'][0, 0]) == 0.5 * (chunk() + 1)
    # both sides 2000 from the iterate: every sigma underflows, g is flat 0: a status of its own
    far = np.full((4, 2), -2000.0)
    f = compare(_native.free_energy_bar(dev(far, device), 2, 0, 1), FE.bar(far, 2, 0, 1), 'far')
    assert f['status'][0, 0] == FE.NO_OVERLAP and f['info'][0, 0] == 0.0 and f['delta'][0, 0] == 0.0
    assert abs(f['delta_forward'][0, 0] + 2000.0) <= FE.average_bound(2, 2000.0)
    # refusals
    for bad in [dict(groups=4), dict(groups=0), dict(n_replicas=4), dict(first_round=-1)]:
        kw = dict(n_replicas=R, first_round=0, groups=1)
        kw.update(bad)
        with pytest.raises(ValueError):
            _native.free_energy_bar(dev(rec, device), **kw)
    with pytest.raises(ValueError):
        _native.free_energy_bar(dev(rec, device).t().contiguous().t(), R)


# ---------------------------------------------------------------------------
# the sampler
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['gauss', 'poly'])
def test_sampler_records_the_restated_work_and_changes_nothing_else(device, kind):
    p0, u_h, u_s = draws(*build_inner(kind, device)[2:], ROUNDS)
    ref, name, C, D = build_inner(kind, device)
    plain = ReplicaExchangeSampler(ref, R_S)
    inner, _, _, _ = build_inner(kind, device)
    re = ReplicaExchangeSampler(inner, R_S, record_work=ROUNDS - 1)
    with pytest.raises(ValueError):
        plain.work
    with pytest.raises(ValueError):
        plain.free_energy()
    rows = []
    for i in range(ROUNDS - 1):
        kw = dict(u=dev(u_s[i], device), inner={'p0': dev(p0[i], device), 'u': dev(u_h[i], device)})
        # the restated row of this round, from the plain sampler's state after its transitions
        plain._transitions(kw['inner'])
        x = plain.state.cpu().numpy()
        lp_own = plain.pdf.log_prob(**{name: plain.state}).cpu().numpy().reshape(-1)
        lp_sw = plain.pdf.log_prob(**{name: dev(RX.gather(x, R_S, i & 1), device)}).cpu().numpy().reshape(-1)
        rows.append(FE.work_row(lp_own, lp_sw, R_S, i & 1))
        a = plain.swap(kw['u'])
        b = re.sample(**kw)
        # with and without the record: the same states, flags and counters
        assert torch.equal(a, b) and torch.equal(plain.last_swap_accepted, re.last_swap_accepted)
        assert torch.equal(plain.n_swap_attempted, re.n_swap_attempted)
        assert torch.equal(plain.n_swap_accepted, re.n_swap_accepted)
        got = re.work.cpu().numpy()
        assert got.shape == (i + 1, C) and re.work_first_round == 0
        assert same_bits(np.nan_to_num(got[i], nan=SENT), np.nan_to_num(rows[i], nan=SENT)), i
        assert np.array_equal(np.isnan(got[i]), FE.partner_or_minus_one(C, R_S, i & 1) < 0)
    assert re.work.data_ptr() == re._work.data_ptr()                     # a view, not a copy
    # a full record raises and leaves state and round unchanged
    before = (re.state.clone(), re.round, re.n_swap_attempted.clone(), re.work.clone(), inner.counter)
    for call in (re.sample, re.swap):
        with pytest.raises(RuntimeError):
            call()
        assert torch.equal(re.state, before[0]) and re.round == before[1] and inner.counter == before[4]
        assert torch.equal(re.n_swap_attempted, before[2]) and bits(re.work) == bits(before[3])
    fe = re.free_energy()
    assert fe.delta.shape == (R_S - 1,) and fe.cumulative.shape == (R_S,) and bool(torch.isnan(fe.stderr).all())
    # reset_work(): the record starts over at the current round
    re.reset_work()
    assert re.work.shape == (0, C) and re.work_first_round == ROUNDS - 1
    i = ROUNDS - 1
    kw = dict(u=dev(u_s[i], device), inner={'p0': dev(p0[i], device), 'u': dev(u_h[i], device)})
    a, b = plain.sample(**kw), re.sample(**kw)
    assert torch.equal(a, b) and re.work.shape == (1, C) and re.work_first_round == i
    assert np.array_equal(np.isnan(re.work[0].cpu().numpy()), FE.partner_or_minus_one(C, R_S, i & 1) < 0)
    want = FE.bar(re.work.cpu().numpy(), R_S, i, 1)
    compare(_native.free_energy_bar(re.work, R_S, re.work_first_round, 1), want, 'after reset')
    # sample_n: more rounds than free rows raises before the first of them
    before = (re.state.clone(), re.round, inner.counter, bits(re.work))
    with pytest.raises(RuntimeError):
        re.sample_n(ROUNDS - 1)
    assert torch.equal(re.state, before[0]) and re.round == before[1] and inner.counter == before[2]
    assert bits(re.work) == before[3] and re.work.shape == (1, C)


def test_checkpoint_carries_the_record(device, tmp_path):
    def build(record=8):
        inner, _, _, _ = build_inner('poly', device, rng=DeviceRNG(9, device), adapt=7)
        return ReplicaExchangeSampler(inner, R_S, record_work=record)

    a = build()
    for _ in range(8):
        a.sample()
    b = build()
    for _ in range(2):
        b.sample()
    b.reset_work()
    for _ in range(2):
        b.sample()
    a_late = a.work[2:]
    path = str(tmp_path / 're.pt')
    checkpoint.save(path, replica=b)
    c = build()
    checkpoint.load(path, replica=c)
    assert c.round == 4 and c.work.shape[0] == 2 and c.work_first_round == 2
    for _ in range(4):
        c.sample()
    assert torch.equal(a.state, c.state)
    assert a_late.shape == c.work.shape and bits(a_late) == bits(c.work)
    fa = free_energy.bar(a_late, R_S, 2)
    fc = c.free_energy()
    for name, x, y in zip(fa._fields, fa, fc):
        assert x.shape == y.shape and x.dtype == y.dtype and bits(x) == bits(y), name
    # a checkpoint written without a record (as before the record existed) still loads
    d = build(None)
    for _ in range(4):
        d.sample()
    assert 'work' not in d.state_dict()
    checkpoint.save(path, replica=d)
    e = build()
    checkpoint.load(path, replica=e)
    assert e.round == 4 and e.work.shape[0] == 0 and e.work_first_round == 4
    f = build(None)
    checkpoint.load(path, replica=f)
    assert f.round == 4
    # a record that does not fit is refused before anything of the sampler is overwritten
    small = build(1)
    kept = (small.state.clone(), small.round, small.n_swap_attempted.clone())
    sd = b.state_dict()
    with pytest.raises(ValueError):
        small.load_state_dict(sd)
    del sd['work_first_round']
    with pytest.raises(ValueError):
        build().load_state_dict(sd)
    assert torch.equal(small.state, kept[0]) and small.round == kept[1] == 0
    assert torch.equal(small.n_swap_attempted, kept[2]) and small.work.shape[0] == 0


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------
AUTOCORRELATION = 1.4           # measured ratios, pairs and total: see the docstring below
AUTOCORRELATION_TOTAL = 1.6


def test_harmonic_ladder_end_to_end(device):
    """R = 4, k = 1, 1/2, 1/4, 1/8, D = 8 (the ladder of the stationarity test), started in
    equilibrium, 300 recorded rounds of 128 ladders, 32 groups: every delta within 6
    group-spread standard errors of 4 ln(1/2), the total within 6 of 12 ln(1/2) (Student-t,
    31 degrees of freedom: a two-sided level near 1e-6).  The standard errors themselves must
    stay under a cap, so a wide spread cannot hide a wrong estimator: AUTOCORRELATION * 2 *
    the iid standard error sqrt(1 / S - 2 / n) that the host restatement gives on exact iid
    draws of the same ladder at the same n (computed on the CPU, no output of the code under
    test); 2 because the spread of 32 groups is known to 13 % only.

    The factors are the ratio group-spread stderr / iid stderr measured once on an MI355X
    (printed by this test): 1.32, 1.28, 1.40 for the three pairs -> AUTOCORRELATION = 1.4, cap
    2.8 iid standard errors; 1.61 for the total (neighbouring pairs share a slot's draws, one
    round apart) -> AUTOCORRELATION_TOTAL = 1.6, cap 3.2.  That run: delta -2.76778, -2.77677,
    -2.78542 (stderr 0.0094, 0.0091, 0.0100) against -2.77259; total -8.32997 (0.0199) against
    -8.31777.  On exact iid draws the restatement passes the same gate with factor 1
    (tests/test_free_energy.py).

    The order delta_reverse <= delta <= delta_forward is printed per pair and nothing is
    asserted about it: it is no property of the estimators.  All three are consistent for the
    same number, and at this ladder's even, good overlap (0.335 ... 0.337 for every pair)
    they differ by sampling noise of either sign: the measured run had two of the three
    pairs out of order at overlaps 0.3365 and 0.3353, the ordered one at 0.3361, so neither
    "unordered only below the ordered pairs' overlap" nor a fixed overlap value separates
    them, and an assertion on it would gate on noise."""
    R, n_ladders, D = 4, FE.E2E_LADDERS, FE.HARMONIC_D
    C = R * n_ladders
    k = torch.tensor(FE.HARMONIC_K, dtype=torch.float64, device=device).repeat(n_ladders)
    rng = DeviceRNG(2025, device)
    x0 = rng.normal((C, D), device) / k.sqrt()[:, None]
    inner = HMCSampler(Harmonic(k), x0, 0.3 / k.sqrt(), 8, variable_name='x', rng=rng)
    re = ReplicaExchangeSampler(inner, R, record_work=FE.E2E_ROUNDS)
    for _ in range(FE.E2E_ROUNDS):
        re.sample()
    fe = re.free_energy(groups=FE.E2E_GROUPS)
    print(fe)
    h = fe.cpu()
    y = FE.harmonic_yardstick()
    exact = FE.harmonic_exact()
    assert np.array_equal(h.n_samples.numpy(), [FE.E2E_ROUNDS // 2 * n_ladders] * (R - 1))
    assert np.all(h.status.numpy() == FE.OK)
    ratio = h.stderr.numpy() / y['iid_stderr']
    ratio_total = float(h.total_stderr) / y['iid_total_stderr']
    print('exact', exact, 'total', exact.sum())
    print('stderr / iid stderr per pair', ratio, 'total', ratio_total)
    order = (h.delta_reverse.numpy() <= h.delta.numpy()) & (h.delta.numpy() <= h.delta_forward.numpy())
    for r in range(R - 1):
        print('pair %d: reverse %.5f  delta %.5f  forward %.5f  overlap %.3f  ordered %s'
              % (r, h.delta_reverse[r], h.delta[r], h.delta_forward[r], h.overlap[r], bool(order[r])))
    assert np.all(np.abs(h.delta.numpy() - exact) <= FE.E2E_SIGMAS * h.stderr.numpy())
    assert abs(float(h.total) - exact.sum()) <= FE.E2E_SIGMAS * float(h.total_stderr)
    assert np.all(h.stderr.numpy() <= AUTOCORRELATION * 2.0 * y['iid_stderr'])
    assert float(h.total_stderr) <= AUTOCORRELATION_TOTAL * 2.0 * y['iid_total_stderr']
    # the short form equals the module's function on the record
    again = free_energy.bar(re.work, R, re.work_first_round, FE.E2E_GROUPS)
    assert torch.equal(again.delta, fe.delta) and torch.equal(again.group_delta, fe.group_delta)
    assert torch.equal(fe.cumulative[1:], -torch.cumsum(fe.delta, 0)) and float(fe.cumulative[0]) == 0.0


def test_example_runs(device):
    spec = importlib.util.spec_from_file_location('example_free_energy',
                                                  os.path.join(ROOT, 'examples', 'free_energy.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(rounds=60, n_ladders=32, quiet=True)
    assert set(out) == {'harmonic', 'double_well'}
    for name, (fe, exact) in out.items():
        assert fe.delta.shape == (len(exact),) and bool((fe.status == 0).all()), name
