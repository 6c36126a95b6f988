"""The diagonal-metric layer on the device (``csrc/metric.hip``, ``HMCSampler(metric=...)``,
``samplers/warmup.py``) against the host restatement ``tests/metric_ref.py``, bit for bit: the
five entry points through the C ABI with every buffer carved out of a sentinel buffer, then the
sampler, the graph, the checkpoint and the replica ladder.

The scaled kernels take 16-byte accesses for an even D on aligned bases and scalar ones
otherwise; a workgroup pass spans 1024 elements (512 scalar): the shapes sit on both sides.
The pool kernel sums blocks of 64 chains of a group, four blocks per round."""
import numpy as np
import pytest
import torch

import metric_ref as MR
from binf_amd import _native, checkpoint
from binf_amd.pdf import IsotropicGaussian
from binf_amd.samplers.hmc import HMCSampler
from binf_amd.samplers.replica import ReplicaExchangeSampler
from binf_amd.samplers.rng import DeviceRNG
from binf_amd.samplers.warmup import WindowedWarmup, warmup

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

    def __init__(self, x, device, odd=False):
        x = np.ascontiguousarray(x, dtype=np.float64)
        self.shape, self.n = x.shape, x.size
        self.before = GUARD + (1 if odd else 0)
        self.whole = torch.full((self.before + self.n + GUARD,), SENT, dtype=torch.float64, device=device)
        assert self.whole.data_ptr() % 16 == 0
        self.view = self.whole[self.before:self.before + self.n]
        self.view.copy_(torch.from_numpy(x.reshape(-1)))
        self.ptr = self.view.data_ptr()

    def take(self):
        w = self.whole.cpu().numpy()
        assert np.all(w[:self.before] == SENT) and np.all(w[self.before + self.n:] == SENT), 'guard zone'
        return w[self.before:self.before + self.n].reshape(self.shape)


def divisors(C):
    return [g for g in range(1, C + 1) if C % g == 0]


def scaled_calls(device, q, p, g, scale, dt, dtc, mode, odd=False):
    """kick (half off / on), drift, kick_drift through the C ABI; {name: arrays}."""
    L, st = _native.lib(), _native.stream_handle(device)
    C, D = q.shape
    G = scale.shape[0]
    sb, gb = Buf(scale, device, odd), Buf(g, device, odd)
    db = None if dtc is None else Buf(dtc, device)
    dptr = None if db is None else db.ptr
    out = {}
    for half in (0, 1):
        pb = Buf(p, device, odd)
        rc = L.binf_leapfrog_kick_scaled_f64(pb.ptr, gb.ptr, sb.ptr, G, dt, dptr, half, C, D, mode, st)
        assert rc == 0, _native.last_error()
        out['kick%d' % half] = pb.take()
    qb, pb = Buf(q, device, odd), Buf(p, device, odd)
    rc = L.binf_leapfrog_drift_scaled_f64(qb.ptr, pb.ptr, sb.ptr, G, dt, dptr, C, D, mode, st)
    assert rc == 0, _native.last_error()
    out['drift'] = qb.take()
    assert bits(pb.take(), p)
    qb, pb = Buf(q, device, odd), Buf(p, device, odd)
    rc = L.binf_leapfrog_kick_drift_scaled_f64(qb.ptr, pb.ptr, gb.ptr, sb.ptr, G, dt, dptr, C, D, mode, st)
    assert rc == 0, _native.last_error()
    out['kd_q'], out['kd_p'] = qb.take(), pb.take()
    assert bits(gb.take(), g) and ieee(sb.take(), scale)
    return out


def scaled_want(q, p, g, scale, dt, dtc, fma):
    kq, kp = MR.kick_drift(q, p, g, scale, dt, dtc, fma)
    return {'kick0': MR.kick(p, g, scale, dt, dtc, False, fma), 'kick1': MR.kick(p, g, scale, dt, dtc, True, fma),
            'drift': MR.drift(q, p, scale, dt, dtc, fma), 'kd_q': kq, 'kd_p': kp}


# (9, 114): 1026 elements of an even D -- past one 16-byte workgroup pass of 1024, with a tail
SHAPES = [(1, 1), (3, 7), (4, 8), (4, 256), (7, 146), (2, 513), (5, 128), (9, 114)]


@pytest.mark.parametrize('C,D', SHAPES)
@pytest.mark.parametrize('mode', [_native.MODE_EXACT, _native.MODE_FMA])
def test_scaled_kernels_equal_the_restatement(device, C, D, mode):
    rs = np.random.RandomState(C * 1000 + D)
    q, p, g = rs.standard_normal((3, C, D))
    dtc = rs.uniform(0.01, 0.4, size=C)
    for G in divisors(C):
        scale = rs.uniform(0.3, 30.0, size=(G, D))
        for dt, dc in ((0.173, None), (0.0, dtc)):
            got = scaled_calls(device, q, p, g, scale, dt, dc, mode)
            want = scaled_want(q, p, g, scale, dt, dc, mode == _native.MODE_FMA)
            for k in want:
                assert bits(got[k], want[k]), (k, G, dc is not None)


@pytest.mark.parametrize('mode', [_native.MODE_EXACT, _native.MODE_FMA])
def test_even_row_on_an_unaligned_base(device, mode):
    """An even D whose bases sit 8 bytes off 16-byte alignment: the scalar variant."""
    rs = np.random.RandomState(5)
    C, D = 4, 256
    q, p, g = rs.standard_normal((3, C, D))
    scale, dtc = rs.uniform(0.3, 30.0, size=(2, D)), rs.uniform(0.01, 0.4, size=C)
    got = scaled_calls(device, q, p, g, scale, 0.0, dtc, mode, odd=True)
    want = scaled_want(q, p, g, scale, 0.0, dtc, mode == _native.MODE_FMA)
    for k in want:
        assert bits(got[k], want[k]), k


def unscaled_calls(device, q, p, g, dt, dtc, mode, odd=False):
    """``scaled_calls`` for the three identity entry points."""
    L, st = _native.lib(), _native.stream_handle(device)
    C, D = q.shape
    gb = Buf(g, device, odd)
    db = None if dtc is None else Buf(dtc, device)
    dptr = None if db is None else db.ptr
    out = {}
    for half in (0, 1):
        pb = Buf(p, device, odd)
        rc = L.binf_leapfrog_kick_f64(pb.ptr, gb.ptr, dt, dptr, half, C, D, mode, st)
        assert rc == 0, _native.last_error()
        out['kick%d' % half] = pb.take()
    qb, pb = Buf(q, device, odd), Buf(p, device, odd)
    rc = L.binf_leapfrog_drift_f64(qb.ptr, pb.ptr, dt, dptr, C, D, mode, st)
    assert rc == 0, _native.last_error()
    out['drift'] = qb.take()
    assert bits(pb.take(), p)
    qb, pb = Buf(q, device, odd), Buf(p, device, odd)
    rc = L.binf_leapfrog_kick_drift_f64(qb.ptr, pb.ptr, gb.ptr, dt, dptr, C, D, mode, st)
    assert rc == 0, _native.last_error()
    out['kd_q'], out['kd_p'] = qb.take(), pb.take()
    assert bits(gb.take(), g) and (db is None or bits(db.take(), dtc))
    return out


@pytest.mark.parametrize('C,D,odd', [s + (False,) for s in SHAPES] + [(4, 256, True)])
@pytest.mark.parametrize('mode', [_native.MODE_EXACT, _native.MODE_FMA])
def test_unscaled_kernels_equal_the_restatement(device, C, D, odd, mode):
    """The identity entry points are the restatement with a scale of ones (``odd``: an even D
    on bases 8 bytes off 16-byte alignment, the scalar variant)."""
    rs = np.random.RandomState(C * 1000 + D + 1)
    q, p, g = rs.standard_normal((3, C, D))
    dtc = rs.uniform(0.01, 0.4, size=C)
    for dt, dc in ((0.173, None), (0.0, dtc)):
        got = unscaled_calls(device, q, p, g, dt, dc, mode, odd)
        want = scaled_want(q, p, g, np.ones((1, D)), dt, dc, mode == _native.MODE_FMA)
        for k in want:
            assert bits(got[k], want[k]), (k, dc is not None)


@pytest.mark.parametrize('C,D', [(3, 7), (4, 256), (2, 513)])
@pytest.mark.parametrize('mode', [_native.MODE_EXACT, _native.MODE_FMA])
def test_unit_scale_equals_the_unscaled_entry_points(device, C, D, mode):
    rs = np.random.RandomState(D)
    q, p, g = (torch.from_numpy(a).to(device) for a in rs.standard_normal((3, C, D)))
    dtc = torch.from_numpy(rs.uniform(0.01, 0.4, size=C)).to(device)
    one = torch.ones(C, D, dtype=torch.float64, device=device)
    for dt, dc in ((0.173, None), (0.0, dtc)):
        for half in (False, True):
            a, b = p.clone(), p.clone()
            _native.leapfrog_kick(a, g, dt, dc, half=half, mode=mode)
            _native.leapfrog_kick_scaled(b, g, one, dt, dc, half=half, mode=mode)
            assert torch.equal(a, b)
        a, b = q.clone(), q.clone()
        _native.leapfrog_drift(a, p, dt, dc, mode=mode)
        _native.leapfrog_drift_scaled(b, p, one[:1], dt, dc, mode=mode)
        assert torch.equal(a, b)
        qa, pa, qb, pb = q.clone(), p.clone(), q.clone(), p.clone()
        _native.leapfrog_kick_drift(qa, pa, g, dt, dc, mode=mode)
        _native.leapfrog_kick_drift_scaled(qb, pb, g, one[0], dt, dc, mode=mode)
        assert torch.equal(qa, qb) and torch.equal(pa, pb)


def test_a_nan_scale_element_touches_its_column_only(device):
    rs = np.random.RandomState(9)
    C, D, G = 6, 10, 2
    q, p, g = rs.standard_normal((3, C, D))
    scale = rs.uniform(0.5, 2.0, size=(G, D))
    clean = scaled_calls(device, q, p, g, scale, 0.1, None, _native.MODE_EXACT)
    scale[1, 3] = np.nan
    got = scaled_calls(device, q, p, g, scale, 0.1, None, _native.MODE_EXACT)
    hit = np.zeros((C, D), dtype=bool)
    hit[1::2, 3] = True
    for k in clean:
        assert np.array_equal(np.isnan(got[k]), hit), k
        assert bits(np.where(hit, 0.0, got[k]), np.where(hit, 0.0, clean[k])), k


# ---------------------------------------------------------------------------
# accumulate, pool
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 2, 5, 33])
@pytest.mark.parametrize('C,D,odd', [(5, 7, False), (4, 8, False), (3, 130, True)])
def test_accumulate_equals_chain_moments_of_the_record(device, n, C, D, odd):
    rs = np.random.RandomState(n + D)
    x = 50.0 + rs.standard_normal((n, C, D)) * rs.uniform(0.1, 20.0, size=(1, C, D))
    if n > 2:
        x[1, 0, 2], x[2, 1, 3] = np.nan, np.inf
    L, st = _native.lib(), _native.stream_handle(device)
    k0, s1, s2 = (Buf(np.full((C, D), 3.5), device, odd) for _ in range(3))       # no initialisation needed
    for t in range(n):
        xb = Buf(x[t], device, odd)
        rc = L.binf_metric_accumulate_f64(xb.ptr, k0.ptr, s1.ptr, s2.ptr, int(t == 0), C, D, st)
        assert rc == 0, _native.last_error()
        assert ieee(xb.take(), x[t])
    want = MR.accumulate(x)
    gk, g1, g2 = k0.take(), s1.take(), s2.take()
    assert ieee(gk, want.k0) and ieee(g1, want.s1) and ieee(g2, want.s2)
    with np.errstate(all='ignore'):
        mean, m2 = gk + g1 / np.float64(n), g2 - (g1 * g1) / np.float64(n)
    assert ieee(mean, want.mean()) and ieee(m2, want.m2())
    if n >= 2:                                                                    # the device's own chain_moments
        dm, d2 = _native.chain_moments(torch.from_numpy(x).to(device), split=1)
        assert ieee(mean, dm.cpu().numpy()) and ieee(m2, d2.cpu().numpy())


@pytest.mark.parametrize('Cg', [1, 2, 63, 64, 65, 130, 330])
@pytest.mark.parametrize('G', [1, 3])
def test_pool_equals_the_restatement(device, Cg, G):
    C, D = Cg * G, 67
    L, st = _native.lib(), _native.stream_handle(device)
    for n in (1, 2, 50):
        rs = np.random.RandomState(Cg * 7 + G + n)
        x = 10.0 + rs.standard_normal((n, C, D)) * rs.uniform(0.1, 20.0, size=(1, 1, D)) + rs.standard_normal((1, C, D))
        if n > 1:
            x[1, G - 1, 5] = np.nan                    # group G - 1, dimension 5
            x[0, 0, 66] = np.inf                       # group 0, dimension 66
            x[:, :, 9] = 1.25                          # constant everywhere: variance 0
        m = MR.accumulate(x)
        prev = rs.uniform(1.0, 2.0, size=(G, D))
        for reg in (0, 1):
            want = MR.pool(m.k0, m.s1, m.s2, n, G, bool(reg), prev)
            k0, s1, s2, sc = Buf(m.k0, device), Buf(m.s1, device), Buf(m.s2, device), Buf(prev, device, odd=True)
            rc = L.binf_metric_pool_f64(k0.ptr, s1.ptr, s2.ptr, n, C, D, G, reg, sc.ptr, st)
            assert rc == 0, _native.last_error()
            got = sc.take()
            assert bits(got, want), (n, reg)
            assert ieee(k0.take(), m.k0) and ieee(s1.take(), m.s1) and ieee(s2.take(), m.s2)
            kept = got == prev
            if n == 1 and Cg == 1:
                assert kept.all()                      # 0 / 0: the previous scale stays
            elif n > 1:
                assert kept[G - 1, 5] and kept[0, 66] and kept[:, 9].all() == (not reg)
                assert kept.sum() == 2 + (0 if reg else G)      # ... and nowhere else


# ---------------------------------------------------------------------------
# the sampler
# ---------------------------------------------------------------------------
def draws(n, C, D, seed):
    rs = np.random.RandomState(seed)
    return rs.standard_normal((n, C, D)), rs.uniform(size=(n, C))


@pytest.mark.parametrize('mode', ['exact', 'fma'])
@pytest.mark.parametrize('graph', [False, 'always'])
def test_sampler_equals_the_restated_transition(device, mode, graph):
    C, D, G, nT = 6, 33, 3, 4
    rs = np.random.RandomState(11)
    q0 = rs.standard_normal((C, D)) * 1.5
    scale = rs.uniform(0.5, 1.5, size=(G, D))
    p0, u = draws(nT, C, D, 12)
    ref = MR.MetricHMC(MR.GaussTarget(2.5, 0.25), q0, 0.11, 4, scale, adaption_limit=10, fma=mode == 'fma')
    s = HMCSampler(IsotropicGaussian(k=2.5, x0=0.25), torch.from_numpy(q0).to(device), 0.11, 4,
                   timestep_adaption_limit=10, variable_name='x', mode=mode, record_energies=True, graph=graph,
                   metric=torch.from_numpy(scale).to(device))
    assert torch.equal(s.inverse_mass, s.metric_scale ** 2)
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
        # a window end rewrites the scale in place: same address, no new capture, new bits
        s.set_metric(torch.from_numpy(scale * 1.25).to(device))
        ref.scale = scale * 1.25
        p1, u1 = draws(1, C, D, 13)
        x = s.sample(p0=torch.from_numpy(p1[0]).to(device), u=torch.from_numpy(u1[0]).to(device))
        assert bits(x.cpu().numpy(), ref.sample(p1[0], u1[0])) and s._graph_captures == 1


def test_unit_metric_equals_the_per_step_tier_without_one(device):
    C, D, nT = 5, 40, 3
    q0 = torch.from_numpy(np.random.RandomState(1).standard_normal((C, D))).to(device)
    p0, u = draws(nT, C, D, 2)
    a = HMCSampler(IsotropicGaussian(), q0.clone(), 0.2, 5, 10, variable_name='x', record_energies=True,
                   metric=torch.ones(D, dtype=torch.float64, device=device))
    b = HMCSampler(IsotropicGaussian(), q0.clone(), 0.2, 5, 10, variable_name='x', record_energies=True)
    b.fused_transition = False
    for t in range(nT):
        pt, ut = torch.from_numpy(p0[t]).to(device), torch.from_numpy(u[t]).to(device)
        assert torch.equal(a.sample(p0=pt, u=ut), b.sample(p0=pt, u=ut))
        assert torch.equal(a.last_e_after, b.last_e_after) and torch.equal(a.timestep, b.timestep)


def test_sample_n_equals_single_calls(device):
    C, D, n = 4, 16, 5
    q0 = torch.from_numpy(np.random.RandomState(3).standard_normal((C, D))).to(device)
    scale = torch.from_numpy(np.random.RandomState(4).uniform(0.5, 2.0, size=(2, D))).to(device)
    p0, u = draws(n, C, D, 5)
    a = HMCSampler(IsotropicGaussian(), q0.clone(), 0.2, 3, variable_name='x', metric=scale)
    b = HMCSampler(IsotropicGaussian(), q0.clone(), 0.2, 3, variable_name='x', metric=scale)
    rec = a.sample_n(n, thin=2, p0=torch.from_numpy(p0).to(device), u=torch.from_numpy(u).to(device))
    singles = [b.sample(p0=torch.from_numpy(p0[t]).to(device), u=torch.from_numpy(u[t]).to(device)) for t in range(n)]
    assert torch.equal(rec, torch.stack([singles[1], singles[3]])) and torch.equal(a.state, b.state)
    assert torch.equal(a.n_accepted, b.n_accepted)


def test_reversibility_inside_a_propagated_rounding_bound(device):
    """L steps, negate r, L steps returns to the start.  Target N(0, I) (gradient = q, exact),
    so in (q, r) every kick r -= a q and drift q += a r is a shear with a_i = dt s_i <= a and
    infinity-norm 1 + a.  An update commits three roundings (h, the product, the sum): a local
    error of at most 3 u (1 + a) M, M the largest |q|, |r| on the way.  Forth and back are
    2 (2 L + 1) updates, each local error grows by at most (1 + a) per later update:
        |return - start| <= 2 (2 L + 1) * 3 u (1 + a) M * (1 + a)^(2 (2 L + 1))."""
    C, D, L_, dt = 7, 146, 5, 0.15
    rs = np.random.RandomState(21)
    scale = rs.uniform(0.5, 2.0, size=(1, D))
    q0, p0 = rs.standard_normal((2, C, D))
    s = HMCSampler(IsotropicGaussian(), torch.from_numpy(q0).to(device), dt, L_, variable_name='x',
                   metric=torch.from_numpy(scale).to(device))
    q, p = torch.from_numpy(q0).to(device), torch.from_numpy(p0).to(device)
    s._leapfrog(q, p, dt, L_)
    mid = max(float(q.abs().max()), float(p.abs().max()))
    assert float((q - torch.from_numpy(q0).to(device)).abs().max()) > 0.1            # it went somewhere
    p.neg_()
    s._leapfrog(q, p, dt, L_)
    a = dt * float(scale.max())
    M = 2.0 * max(mid, float(np.abs(q0).max()), float(np.abs(p0).max()))             # H-bounded orbit, with room
    nu = 2 * (2 * L_ + 1)
    bound = nu * 3 * 2.0 ** -53 * (1 + a) * M * (1 + a) ** nu
    err = max(float((q.cpu() - torch.from_numpy(q0)).abs().max()), float((-p.cpu() - torch.from_numpy(p0)).abs().max()))
    print('reversibility: error %.3g, bound %.3g' % (err, bound))
    assert bound < 1e-10 and err <= bound


class Harmonic(object):
    """A user's torch PDF: log p_c(x) = -1/2 beta_c sum (x / sigma)^2."""

    def __init__(self, beta, sigma):
        self.beta, self.sigma = beta, sigma

    def log_prob(self, x):
        z = x / self.sigma
        return -0.5 * self.beta * (z * z).sum(dim=1)

    def gradient(self, x):
        return self.beta[:, None] * x / (self.sigma * self.sigma)


def _warm_run(device, graph=False):
    C, D = 8, 6
    sigma = torch.tensor([1.0, 3.0, 10.0, 0.3, 30.0, 2.0], dtype=torch.float64, device=device)
    rng = DeviceRNG(77, device)
    x0 = 2.0 * sigma * torch.from_numpy(np.random.RandomState(8).standard_normal((C, D))).to(device)
    s = HMCSampler(Harmonic(torch.ones(C, dtype=torch.float64, device=device), sigma), x0, 0.3, 4,
                   adaption_uprate=1.02, adaption_downrate=0.9, variable_name='x', rng=rng, graph=graph)
    return s, WindowedWarmup(s, 70, init_buffer=10, term_buffer=10, base_window=10)


@pytest.mark.parametrize('graph', [False, 'always'])
def test_checkpoint_in_the_middle_of_a_window(device, graph):
    """40 of 70 warm-up transitions (windows [10, 20), [20, 60): the second is open), the
    state of sampler and driver through the host into fresh objects, the rest and five kept
    draws equal the uninterrupted run bit for bit."""
    a, wa = _warm_run(device, graph)
    assert wa.windows == [(10, 20), (20, 60)] and a.timestep_adaption_limit == 71
    for _ in range(40):
        wa.step()
    ck = checkpoint.state_dict(sampler=a, warmup=wa)
    assert 'metric_scale' in ck['sampler'] and not ck['sampler']['metric_scale'].is_cuda
    b, wb = _warm_run(device, graph)
    checkpoint.load_state_dict(ck, sampler=b, warmup=wb)
    assert wb.t == 40 and wb.n_window == 20
    wa.run(), wb.run()
    assert wa.done and wb.done and a.counter == b.counter == 70
    assert torch.equal(a.metric_scale, b.metric_scale) and torch.equal(a.timestep, b.timestep)
    for _ in range(5):
        assert torch.equal(a.sample(), b.sample())
    assert not torch.equal(a.metric_scale, torch.ones_like(a.metric_scale))
    with pytest.raises(RuntimeError):
        wa.step()


def test_a_ladder_gets_one_scale_row_per_slot(device):
    """4 ladders x 3 slots at beta = 1, 1/4, 1/16: the inner sampler gets a [3 x D] scale, the
    rows differ, and a hotter slot's row is the wider one (sd ~ sigma / sqrt(beta))."""
    R, n_ladders, D = 3, 4, 5
    C = R * n_ladders
    sigma = torch.tensor([1.0, 2.0, 5.0, 0.5, 10.0], dtype=torch.float64, device=device)
    beta = torch.tensor([1.0, 0.25, 0.0625], dtype=torch.float64, device=device).repeat(n_ladders)
    rng = DeviceRNG(5, device)
    x0 = sigma * rng.normal((C, D), device) / beta.sqrt()[:, None]
    inner = HMCSampler(Harmonic(beta, sigma), x0, 0.3, 5, variable_name='x', rng=rng)
    rex = ReplicaExchangeSampler(inner, R)
    w = warmup(rex, 120, init_buffer=10, term_buffer=10, base_window=20)
    assert w.groups == R and w.hmc is inner and tuple(inner.metric_scale.shape) == (R, D)
    assert rex.round == 120 and inner.counter == 120
    sc = inner.metric_scale.cpu().numpy()
    assert np.isfinite(sc).all() and (sc > 0).all()
    for r in range(R - 1):
        assert not np.array_equal(sc[r], sc[r + 1])
        assert np.mean(np.log(sc[r + 1] / sc[r])) > 0.2            # expected log 2 = 0.69
    rex.sample()                                                    # goes on with the metric in place
