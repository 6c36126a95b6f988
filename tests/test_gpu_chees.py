"""Device tests of ChEES-HMC against its host restatement (``tests/chees_ref.py``).

The criterion kernels are driven through the C ABI, every array inside a sentinel buffer, and
compared bit for bit (alpha comes from the host: no exponential is involved).  The sampler is
compared transition by transition: states and step counts bit for bit, the host scalars within
a derived bound (see ``test_sampler_equals_the_restated_loop``).
"""
import math

import numpy as np
import pytest
import torch

import chees_ref as R
import nuts_ref as N
import stationarity as S
from binf_amd import _native, checkpoint, dist
from binf_amd.pdf import IsotropicGaussian
from binf_amd.samplers import ChEESSampler
from binf_amd.samplers.chees import halton
from binf_amd.samplers.hmc import HMCSampler
from binf_amd.samplers.replica import ReplicaExchangeSampler
from binf_amd.samplers.rng import DeviceRNG
from binf_amd.samplers.warmup import warmup

pytestmark = pytest.mark.gpu

f64 = np.float64
K_, X0 = 0.7, 0.3
FILL = -7.25
PAD = 64


def host_logp(q):
    with np.errstate(all='ignore'):
        return (f64(-0.5) * f64(K_)) * np.sum((q - f64(X0)) ** 2, axis=1)


def host_grad(q):
    with np.errstate(all='ignore'):
        return f64(K_) * (q - f64(X0))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=f64), np.ascontiguousarray(b, dtype=f64)
    return a.shape == b.shape and bool(np.all((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))))


class Guarded(object):
    """fp64 arrays, each inside its own sentinel buffer (``PAD`` bytes of 0xA5 on both sides);
    ``odd``: bases 8 bytes past a 16-byte boundary (the 8-byte access path)."""

    def __init__(self, device, odd=False):
        self.device, self.odd, self.bufs, self.t = device, odd, {}, {}

    def add(self, name, shape, value=None):
        n = int(np.prod(shape)) * 8
        start = PAD + (8 if self.odd else 0)
        buf = torch.full((start + n + PAD,), 0xA5, dtype=torch.uint8, device=self.device)
        assert buf.data_ptr() % 16 == 0
        view = buf[start:start + n].view(torch.float64).view(shape)
        if value is None:
            view.fill_(FILL)
        else:
            view.copy_(torch.from_numpy(np.ascontiguousarray(value, dtype=f64)))
        self.bufs[name], self.t[name] = (buf, start, n), view
        return view

    def guards_intact(self):
        return all(bool((buf[:start] == 0xA5).all()) and bool((buf[start + n:] == 0xA5).all())
                   for buf, start, n in self.bufs.values())

    def host(self, name):
        return self.t[name].cpu().numpy()


def kernel_inputs(C, D, variant, seed):
    rs = np.random.RandomState(seed)
    q = rs.standard_normal((C, D)) * 2.0 + 0.5
    q_prop = q + 0.7 * rs.standard_normal((C, D))
    v = rs.standard_normal((C, D))
    alpha = np.minimum(1.0, rs.uniform(0.02, 1.3, size=C))           # some are exactly 1
    if variant == 'some_zero':
        alpha[::3] = 0.0
        q_prop[::3] = np.nan                                          # a diverged trajectory's proposal
        v[::3] = np.nan
    elif variant == 'all_zero':
        alpha[:] = 0.0
        q_prop[1::2] = np.inf
    elif variant == 'overflow':
        alpha[0] = 0.5
        q_prop[0] = q[0] + 1000.0
        v[0] = 1e308                                                  # s overflows for this chain only
    return q, q_prop, v, alpha


def run_kernels(device, q, q_prop, v, alpha, odd):
    C, D = q.shape
    a = Guarded(device, odd)
    for name, x in (('q', q), ('q_prop', q_prop), ('v', v), ('alpha', alpha)):
        a.add(name, x.shape, x)
    need = _native.lib().binf_chees_workspace_bytes(C, D)
    assert need == ((C + 63) // 64) * max(2 * D, 4) * 8
    a.add('slab', (need // 8,))
    for name, shape in (('mean_q', (D,)), ('mean_prop', (D,)), ('g', (C,)), ('out', (4,))):
        a.add(name, shape)
    t = a.t
    _native.chees_means(t['q'], t['q_prop'], t['alpha'], t['slab'], t['mean_q'], t['mean_prop'])
    _native.chees_terms(t['q'], t['q_prop'], t['v'], t['alpha'], t['mean_q'], t['mean_prop'], t['g'])
    _native.chees_sums(t['alpha'], t['g'], t['slab'], t['out'])
    torch.cuda.synchronize()
    return a


@pytest.mark.parametrize('D', [1, 5, 127, 128, 130, 1025])
@pytest.mark.parametrize('C', [1, 2, 63, 64, 65, 129, 1000])
def test_criterion_kernels_bit_for_bit(device, C, D):
    """means, terms and sums through the C ABI against the restatement, bit for bit, for plain
    inputs, inputs with alpha == 0 rows whose proposal is NaN (bases 8 bytes past a 16-byte
    boundary), all alpha == 0, and a row whose g overflows; inputs and guard bytes untouched."""
    for i, variant in enumerate(('plain', 'some_zero', 'all_zero', 'overflow')):
        q, q_prop, v, alpha = kernel_inputs(C, D, variant, 100 * C + D + i)
        a = run_kernels(device, q, q_prop, v, alpha, odd=variant == 'some_zero')
        mq, mp, g, out = R.criterion(q, q_prop, v, alpha)
        for name, want in (('mean_q', mq), ('mean_prop', mp), ('g', g), ('out', out)):
            assert same_bits(a.host(name), want), (name, variant)
        for name, want in (('q', q), ('q_prop', q_prop), ('v', v), ('alpha', alpha)):
            assert same_bits(a.host(name), want), (name, variant)
        assert a.guards_intact(), variant
        got = a.host('g')
        assert not np.signbit(got[alpha == 0.0]).any() and (got[alpha == 0.0] == 0.0).all()
        if C == 1:
            assert (got == 0.0).all()                                 # one chain is its own mean
        if variant == 'all_zero':
            assert same_bits(a.host('out'), np.array([0.0, 0.0, np.inf, 0.0]))
        if variant == 'some_zero':
            assert a.host('out')[2] == np.inf and a.host('out')[3] == 0.0 and np.isfinite(a.host('mean_prop')).all()
        if variant == 'overflow' and C > 1 and D >= 5:
            assert a.host('out')[3] == 1.0 and not np.isfinite(got[0]) and np.isfinite(a.host('out')[0])


def test_accept_prob(device):
    """Within 1 ulp of numpy's clipped exponential on finite differences; exact at the edges."""
    rs = np.random.RandomState(5)
    n = 5000
    eb = rs.standard_normal(n) * 30.0
    ea = eb + np.concatenate([rs.uniform(0.0, 40.0, n // 2), rs.uniform(0.0, 1e-3, n - n // 2)])
    edge_b = np.array([1.5, 2.0, 7.0, 1.0, 1.0, 1.0, np.nan, np.inf, -1000.0, 0.0, np.inf, -np.inf])
    edge_a = np.array([1.5, 1.0, -900.0, np.nan, np.inf, -np.inf, 1.0, 1.0, 0.0, 5000.0, np.inf, 3.0])
    eb, ea = np.concatenate([eb, edge_b]), np.concatenate([ea, edge_a])
    a = Guarded(device)
    a.add('eb', eb.shape, eb), a.add('ea', ea.shape, ea), a.add('alpha', eb.shape)
    _native.chees_accept_prob(a.t['eb'], a.t['ea'], a.t['alpha'])
    got, want = a.host('alpha'), R.accept_prob(eb, ea)
    assert a.guards_intact() and same_bits(a.host('eb'), eb) and same_bits(a.host('ea'), ea)
    assert (np.abs(got - want) <= np.spacing(want)).all()
    assert ((got >= 0.0) & (got <= 1.0)).all() and (got[:n] > 0.0).all() and (got[:n // 2] < 1.0).any()
    e = got[n:]
    assert e[0] == 1.0 and e[1] == 1.0 and e[2] == 1.0                 # difference 0, positive, huge
    assert same_bits(e[3:7], np.zeros(4))                              # e_after not finite, the difference NaN: +0.0
    assert e[7] == 1.0                                                 # e_before = +inf alone: a positive difference
    assert same_bits(e[10:11], np.zeros(1))                            # inf - inf
    clip = float(np.exp(-308.0))
    assert abs(e[8] - clip) <= np.spacing(clip) and e[8] == e[9] and e[9] == e[11] and e[8] > 0.0   # below the clip
    # in place over e_after
    _native.chees_accept_prob(a.t['eb'], a.t['ea'], a.t['ea'])
    assert same_bits(a.host('ea'), got)


# ---------------------------------------------------------------------------
# the sampler
# ---------------------------------------------------------------------------
def _metric(kind, D, seed):
    rs = np.random.RandomState(seed)
    if kind == 'diag':
        return 2.0 ** rs.uniform(-1.0, 1.0, size=(1, D))
    if kind == 'dense':
        L = np.tril(0.2 * rs.standard_normal((1, D, D)))
        i = np.arange(D)
        L[:, i, i] = 2.0 ** rs.uniform(-1.0, 1.0, size=(1, D))
        return L
    return None


U = 2.0 ** -53


@pytest.mark.parametrize('kind', ['identity', 'diag', 'dense'])
def test_sampler_equals_the_restated_loop(device, kind):
    """12 adapting and 4 frozen transitions with supplied p0, u on ``IsotropicGaussian(0.7, 0.3)``,
    65 chains x 5 dimensions, from T = 2, eps = 0.3: the states and the step counts L_t are those of
    the restatement, bit for bit; T and eps agree within the bound below after every transition,
    and the restatement then continues from the device's scalars (as ``test_gpu_nuts.py`` does for
    its step sizes: an ulp in eps would otherwise move every later state).

    The bound.  The device's alpha is within 1 ulp (2u, u = 2^-53) of numpy's; means and g do not
    depend on alpha's value, so they are the same bits.  A sum of n terms through the tree of depth
    6 and ``nch`` chunk additions carries at most d = 6 + nch roundings per computation.  With
    kappa = sum |alpha g| / |sum alpha g| (asserted <= 1e3 on the restatement):
      out[0]: relative (4 + 2 d) u kappa   (alpha: 2u, the product's rounding twice: 2u, sums: 2 d u)
      out[1]: (2 + 2 d) u;   out[2]: (4 + 2 d) u   (1 / alpha: alpha's 2u and the division twice)
      g^ = (L eps) out[0] / out[1]: dg = (4 + 2 d) u kappa + (2 + 2 d) u
      Adam, beta1 = 0: the step is lr g^ / (sqrt(m2^) + 1e-8) with m2^ >= (1 - beta2) g^2, so it is at
      most lr / sqrt(1 - beta2) = 0.1118 and moves by at most twice dg of itself (numerator and
      second moment): |d log T| <= 0.2236 dg
      dual averaging: stat = C / out[2] <= 1; d hbar = w1 d stat, d log eps = k1 w1 d stat, and
      k1 w1 = sqrt(t) / (gamma (t + t0)) <= 3.2 (its maximum, at t = t0 = 10): |d log eps| <= 3.2 (4 + 2 d) u
      the clip of T into [eps, L_max eps] passes eps's difference on; averages and the freeze are
      convex combinations of values within these bounds.  4u more for the host's own roundings.
    Conditions asserted on the restatement (not tolerances): tau_t / eps further than 1e-9 from an
    integer, kappa <= 1e3, |u - alpha| > 1e-9."""
    C, D, n_adapt, n_frozen = 65, 5, 12, 4
    rs = np.random.RandomState(0)
    q0 = X0 + rs.standard_normal((C, D)) / np.sqrt(K_)
    param = _metric(kind, D, 1)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)
    kw = {'metric': up(param)} if kind == 'diag' else {'dense_metric': up(param)} if kind == 'dense' else {}
    s = ChEESSampler(IsotropicGaussian(k=K_, x0=X0), up(q0), 0.3, timestep_adaption_limit=n_adapt + 1,
                     variable_name='x', **kw)
    s.trajectory_length = 2.0
    from binf_amd.samplers.chees import TrajectoryAdaption
    ad = TrajectoryAdaption(0.3)
    ad.log_T = math.log(2.0)
    ref = R.ChEES(host_logp, host_grad, q0, ad, R.Integrator(kind, param), adaption_limit=n_adapt + 1)
    d = 6 + (C + 63) // 64
    worst, steps = 0.0, []
    for i in range(n_adapt + n_frozen):
        p0, u = rs.standard_normal((C, D)), rs.uniform(size=C)
        assert s.adapting == (i < n_adapt)
        want = ref.sample(p0, u)
        got = s.sample(p0=up(p0), u=up(u))
        assert same_bits(got.cpu().numpy(), want), i
        assert s.last_n_leapfrog == ref.steps == s.nsteps, i
        assert np.array_equal(s.last_move_accepted.cpu().numpy(), ref.accepted), i
        steps.append(ref.steps)
        if i < n_adapt:
            alpha = s.last_accept_prob.cpu().numpy()
            assert (np.abs(alpha - ref.alpha) <= np.spacing(ref.alpha)).all(), i
            assert same_bits(s._ws['g'].cpu().numpy(), ref.g) and same_bits(s._ws['mean_prop'].cpu().numpy(), ref.mean_prop)
            kappa = float(np.sum(np.abs(ref.alpha * ref.g))) / abs(float(ref.out[0]))
            dg = ((4 + 2 * d) * kappa + (2 + 2 * d)) * U
            b_eps = (3.2 * (4 + 2 * d) + 4) * U
            b_T = 0.2236 * dg + b_eps + 4 * U
            e_eps = abs(s.timestep - ad.eps) / ad.eps
            e_T = abs(s.trajectory_length - ad.T) / ad.T
            print('transition %d: L %d kappa %.1f  eps off %.2e of %.2e  T off %.2e of %.2e'
                  % (i, ref.steps, kappa, e_eps, b_eps, e_T, b_T))
            worst = max(worst, e_eps / b_eps, e_T / b_T)
            assert e_eps <= b_eps and e_T <= b_T, i
            ad.load_state_dict(s.adaption.state_dict())              # continue from the device's scalars
        else:
            assert s.timestep == ad.eps and s.trajectory_length == ad.T and s.adaption.frozen and ad.frozen
    assert s.adaption.index == n_adapt + n_frozen and s.n_leapfrog_total == sum(steps)
    assert s.mean_leapfrog_steps == max(1, int(math.ceil(ad.T / (2.0 * ad.eps)))) and s.counter == len(steps)
    assert len(set(steps)) >= 4                                      # the count did change
    assert ref.min_ceil_margin > 1e-9 and ref.max_cancellation <= 1e3 and ref.min_accept_margin > 1e-9
    print('worst error / bound %.3f' % worst)


def test_frozen_sampler_is_plain_hmc(device):
    """No metric, a PDF with a whole-transition kernel, supplied draws: every frozen transition
    is ``HMCSampler(..., nsteps=L_t)``'s, bit for bit; without jitter ``sample_n`` is n single calls."""
    C, D = 130, 33
    rs = np.random.RandomState(2)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)
    pdf = IsotropicGaussian(k=K_, x0=X0)
    q0 = up(X0 + rs.standard_normal((C, D)) / np.sqrt(K_))
    s = ChEESSampler(pdf, q0.clone(), 0.2, variable_name='x')
    s.trajectory_length = 1.5
    assert not s.adapting and s._fused_spec('x', D, C) is not None
    seen = []
    for i in range(6):
        p0, u = up(rs.standard_normal((C, D))), up(rs.uniform(size=C))
        L = max(1, int(math.ceil(halton(i + 1) * s.trajectory_length / 0.2)))
        h = HMCSampler(pdf, s.state.clone(), 0.2, L, variable_name='x')
        want = h.sample(p0=p0, u=u)
        got = s.sample(p0=p0, u=u)
        assert s.nsteps == L == s.last_n_leapfrog and torch.equal(got, want), i
        assert torch.equal(s.last_move_accepted, h.last_move_accepted)
        seen.append(L)
    assert abs(s.trajectory_length - 1.5) < 1e-15 and s.timestep == 0.2 and len(set(seen)) >= 4 and s.adaption.frozen
    a = ChEESSampler(pdf, q0.clone(), 0.2, variable_name='x', jitter=False)
    b = ChEESSampler(pdf, q0.clone(), 0.2, variable_name='x', jitter=False)
    a.trajectory_length = b.trajectory_length = 1.5
    n = 5
    p0, u = up(rs.standard_normal((n, C, D))), up(rs.uniform(size=(n, C)))
    rec = a.sample_n(n, thin=2, p0=p0, u=u)
    each = [b.sample(p0=p0[i], u=u[i]).clone() for i in range(n)]
    assert a.nsteps == b.nsteps == 4 and rec.shape == (2, C, D)        # ceil(1.5 / 0.4)
    assert torch.equal(rec[0], each[1]) and torch.equal(rec[1], each[3]) and torch.equal(a.state, each[4])
    assert a.counter == b.counter == n and a.n_leapfrog_total == b.n_leapfrog_total == 4 * n


class TorchGauss(object):
    """A user's torch PDF: log p(x) = -1/2 x' P x."""

    def __init__(self, precision):
        self.P = precision

    def log_prob(self, x):
        return -0.5 * (x * (x @ self.P)).sum(dim=1)

    def gradient(self, x):
        return x @ self.P


class TorchDiagGauss(object):
    """A user's torch PDF, element-wise: log p(x) = -1/2 sum x^2 / sigma^2."""

    def __init__(self, precision):
        self.prec = precision

    def log_prob(self, x):
        return -0.5 * (x * x * self.prec).sum(dim=1)

    def gradient(self, x):
        return x * self.prec


def _adapted(device, sigma, seed, n=300, C=64):
    sigma = np.asarray(sigma, dtype=f64)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)
    x0 = sigma * np.random.RandomState(seed).standard_normal((C, sigma.size))
    s = ChEESSampler(TorchDiagGauss(up(1.0 / sigma ** 2)), up(x0), 0.1, timestep_adaption_limit=n + 1,
                     variable_name='x', rng=DeviceRNG(seed, device))
    for _ in range(n):
        s.sample()
    assert not s.adapting and s.adaption.frozen and s.counter == n
    return s


WIDE_T = (15.7809, 8.7153, 19.2294, 10.5385, 14.7732)


def test_adaption_finds_the_scale_of_the_target(device):
    """sigma = linspace(1, 10, 16), 64 chains, 300 adapting transitions from T0 = eps0 = 0.1 on the
    device's own draws.  The restatement (``chees_ref.run_gaussian`` at the same settings) freezes at
    T = 15.7809, 8.7153, 19.2294, 10.5385, 14.7732 (eps 1.27 ... 1.32) over seeds 0-4; the device's T must
    lie in [min / 1.5, 1.5 max] = [5.81, 28.84], the factor for a different draw stream.  On sigma = 1
    (restatement: T = 1.60 ... 3.36, eps 0.78 ... 0.80) it must end at a smaller T."""
    lo, hi = min(WIDE_T) / 1.5, 1.5 * max(WIDE_T)
    assert not lo <= 0.1 <= hi                                         # or the test shows nothing
    wide = _adapted(device, np.linspace(1.0, 10.0, 16), 0)
    unit = _adapted(device, np.ones(16), 0)
    print('wide: T %.4f eps %.4f mean L %d;  unit: T %.4f eps %.4f mean L %d' % (
        wide.trajectory_length, wide.timestep, wide.mean_leapfrog_steps,
        unit.trajectory_length, unit.timestep, unit.mean_leapfrog_steps))
    assert isinstance(wide.mean_leapfrog_steps, int) and wide.mean_leapfrog_steps > unit.mean_leapfrog_steps >= 1
    assert lo <= wide.trajectory_length <= hi
    assert unit.trajectory_length < wide.trajectory_length
    assert wide.adaption.n_updates > 250 and isinstance(wide.timestep, float) and 0.1 < wide.timestep < 2.0
    # the documented route to graph replay of the learnt configuration
    h = HMCSampler(wide.pdf, wide.state.clone(), wide.timestep, wide.mean_leapfrog_steps, variable_name='x',
                   graph=True, rng=DeviceRNG(1, device))
    e = HMCSampler(wide.pdf, wide.state.clone(), wide.timestep, wide.mean_leapfrog_steps, variable_name='x',
                   rng=DeviceRNG(1, device))
    for _ in range(4):
        assert torch.equal(h.sample(), e.sample())
    assert h._graph_captures == 1


def _run(device, n, load=None, limit=5, seed=11):
    C, D = 40, 9
    q0 = X0 + np.random.RandomState(seed).standard_normal((C, D)) / np.sqrt(K_)
    s = ChEESSampler(IsotropicGaussian(k=K_, x0=X0), torch.from_numpy(q0).to(device), 0.3,
                     timestep_adaption_limit=limit, variable_name='x', rng=DeviceRNG(seed, device))
    s.trajectory_length = 1.7
    if load is not None:
        checkpoint.load_state_dict(load, sampler=s)
    return s, (torch.stack([s.sample().clone() for _ in range(n)]) if n else None)


def test_checkpoint_across_the_freeze_resumes_bit_for_bit(device, tmp_path):
    """3 transitions, save, load into a fresh sampler, 3 more = 6 transitions; the fourth is the
    last adapting one (the freeze), so the checkpoint carries a live adaption."""
    whole, xs = _run(device, 6)
    first, _ = _run(device, 3)
    assert first.adapting and not first.adaption.frozen
    path = str(tmp_path / 'chees.pt')
    checkpoint.save(path, sampler=first)
    resumed, _ = _run(device, 0)
    checkpoint.load(path, sampler=resumed)
    tail = torch.stack([resumed.sample().clone() for _ in range(3)])
    assert torch.equal(tail, xs[3:])
    assert resumed.adaption.state_dict() == whole.adaption.state_dict() and whole.adaption.frozen
    assert resumed.adaption.index == 6 and resumed.counter == whole.counter == 6
    assert resumed.timestep == whole.timestep and resumed.trajectory_length == whole.trajectory_length
    assert resumed.n_leapfrog_total == whole.n_leapfrog_total and torch.equal(resumed.n_accepted, whole.n_accepted)
    assert torch.equal(resumed.last_accept_prob, whole.last_accept_prob)


def test_windowed_warmup_drives_the_sampler(device):
    """``warmup(ChEESSampler(...), 60, dense=True)``: runs, restarts the step averaging at the
    window's end, leaves a frozen sampler with a learnt factor that goes on sampling."""
    import dense_metric_ref as DM
    S_, P, Ls = DM.rotated_target()
    D, C = S_.shape[0], 32
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)
    start = np.random.RandomState(0).standard_normal((C, D)) @ Ls.T
    s = ChEESSampler(TorchGauss(up(P)), up(start), 0.05, variable_name='x', rng=DeviceRNG(0, device))
    calls, restart = [], s.restart_step_adaption
    s.restart_step_adaption = lambda: (calls.append(s.counter), restart())
    w = warmup(s, 60, dense=True)
    assert len(w.windows) >= 1 and calls == [stop for _, stop in w.windows]       # after each window's last transition
    assert s.counter == 60 and not s.adapting and s.adaption.frozen and s.metric_chol is not None
    assert not torch.equal(s.metric_chol[0], torch.eye(D, dtype=torch.float64, device=device))
    T, eps = s.trajectory_length, s.timestep
    x = s.sample_n(5)
    assert x.shape == (5, C, D) and bool(torch.isfinite(x).all())
    assert (s.trajectory_length, s.timestep) == (T, eps) and s.adaption.index == 65


def test_frozen_jittered_sampler_keeps_the_target(device):
    """The stationarity check of ``test_gpu_nuts.py`` (N(0, diag(1, 2, 3, 5, 10)^2), 4000 chains from exact
    draws, 3 transitions, pooled chi^2, pooled mean and DKW at the suite's level) for the frozen
    sampler with jitter: eps = 0.9, T = 12, so the three transitions take 7, 4 and 10 steps."""
    case = N.Case('identity')
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)
    C = N.STATIONARITY_C
    x0 = case.sample(np.random.RandomState(3), C)
    s = ChEESSampler(TorchGauss(up(case.precision)), up(x0), 0.9, variable_name='x', rng=DeviceRNG(3, device))
    s.trajectory_length = 12.0
    taken = []
    for _ in range(N.STATIONARITY_N):
        x = s.sample()
        taken.append(s.last_n_leapfrog)
    assert taken == [7, 4, 10]
    checks = N.stationarity_checks(case, x.cpu().numpy(), S.ALPHA / 3)
    for c in checks:
        print(S.describe(c))
    assert all(S.inside(c) for c in checks), [S.describe(c) for c in checks]
    assert 0.3 < float(s.acceptance_rate.mean()) < 1.0


def test_refusals(device, monkeypatch):
    pdf = IsotropicGaussian(k=K_, x0=X0)
    x = torch.zeros((8, 3), dtype=torch.float64, device=device)
    with pytest.raises(ValueError, match='graph'):
        ChEESSampler(pdf, x, 0.1, variable_name='x', graph=True)
    with pytest.raises(ValueError, match='nsteps'):
        ChEESSampler(pdf, x, 0.1, variable_name='x', nsteps=3)
    s = ChEESSampler(pdf, x.clone(), 0.1, variable_name='x', timestep_adaption_limit=10)
    s.graph = True
    with pytest.raises(ValueError, match='graph'):
        s.sample()
    s.graph = False
    # adapting pools all chains: not on a shard of a distributed run, not inside a ladder
    monkeypatch.setattr(dist, 'world', lambda: (0, 2))
    with pytest.raises(NotImplementedError):
        s.sample()
    frozen = ChEESSampler(pdf, x.clone(), 0.1, variable_name='x')
    frozen.sample()                                                   # a frozen sampler works on a shard as it is
    monkeypatch.undo()
    with pytest.raises(TypeError, match='adapting'):
        ReplicaExchangeSampler(s, 2)
    ladder = ReplicaExchangeSampler(frozen, 2)
    frozen.timestep_adaption_limit = 100
    with pytest.raises(TypeError, match='adapting'):
        ladder.sample()
    assert s.counter == 0 and s.adaption.index == 0                   # the refused calls began nothing
    s.sample()
    assert s.counter == 1 and s.adaption.index == 1
    # outputs that overlap an input or each other
    buf = torch.zeros(64, dtype=torch.float64, device=device)
    q, v = torch.zeros((8, 3), dtype=torch.float64, device=device), torch.zeros((8, 3), dtype=torch.float64, device=device)
    slab = _native.chees_workspace(8, 3, device)
    with pytest.raises(ValueError, match='overlaps'):
        _native.chees_means(q, v, buf[:8], slab, buf[8:11], buf[10:13])
    with pytest.raises(ValueError, match='overlaps'):
        _native.chees_terms(q, v, v.clone(), buf[:8], buf[8:11], buf[11:14], buf[7:15])
    with pytest.raises(ValueError, match='overlaps'):
        _native.chees_sums(buf[:8], buf[8:16], slab, buf[15:19])
    with pytest.raises(ValueError, match='overlaps'):
        _native.chees_accept_prob(buf[:8], buf[8:16], buf[1:9])
    assert bool((buf == 0.0).all())
