"""The chain-resident kernels of a linear forward model on the GPU
(``binf_hmc_sample_linear_f64``, ``binf_gibbs_linear_sample_n_f64``;
csrc/linear_chain_kernel.hpp) and the kind ``'linear_resident'`` that takes a model
built with ``resident=True`` through them.

Against numpy: every tolerance is a derived bound (tests/linear_resident_ref.py on top of
tests/linear_bounds.py and tests/poly_bounds.py).  Against themselves: bit for bit."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import linear_resident_ref as RR
import poly_bounds as PB
from binf_amd import _native, checkpoint
from binf_amd.example.likelihood import GaussianErrorModel
from binf_amd.example.samplers import make_hmc_sampler, make_sampler
from binf_amd.model import linear_resident
from binf_amd.model.linear import LinearForwardModel
from binf_amd.pdf.likelihoods import Likelihood
from binf_amd.samplers import BinfState
from binf_amd.samplers.hmc import HMCSampler
from binf_amd.samplers.rng import DeviceRNG, HostLegacyRNG
from conftest import GOLDEN_DIR
from test_gpu_guards import Guarded, plain
from test_gpu_linear import Spy, dev_t, exact_chains, fourier_case, posterior_of, random_case

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (4, 20), (7, 37), (9, 200), (16, 128), (16, 129), (3, 513), (5, 920), (16, 1024)]
CHAINS = [1, 5, 300, 4100]
GP_SHAPE, GP_RATE = 2.0, 0.2          # the GammaPrior term of a conditional (a constant of the move)


def gamma_term(tau):
    return (GP_SHAPE - 1.0) * np.log(tau) - tau * GP_RATE


def u8(n, device):
    return torch.empty(n, dtype=torch.uint8, device=device)


def hmc_launch(device, A, ys, theta, p0, u, tau, dt, L, var=None, prior_first=True, pre=None, post=None,
               mode=_native.MODE_EXACT, t=None, q_out=None):
    """One call of binf_hmc_sample_linear_f64; tau / dt scalars or [C] arrays."""
    t = t or (lambda a: dev_t(a, device))
    C, K = theta.shape
    q0 = t(theta)
    q_out = q0 if q_out == 'alias' else t(np.zeros((C, K)))
    acc = t(np.zeros(C, dtype=np.uint8), torch.uint8) if t.__class__ is Guarded else u8(C, device)
    eb, ea = t(np.zeros(C)), t(np.zeros(C))
    dtc = None if np.isscalar(dt) else t(dt)
    _native.hmc_sample_linear(
        q0, t(p0), t(u), q_out, acc, None, eb, ea, t(A), t(ys), tau if np.isscalar(tau) else t(tau),
        None if var is None else t(np.zeros(K)), None if var is None else t(np.full(K, float(var))),
        prior_first, None if pre is None else t(pre), None if post is None else t(post),
        float(dt) if np.isscalar(dt) else 0.0, dtc, L, False, 1.05, 0.95, mode)
    torch.cuda.synchronize()
    return q_out.cpu().numpy(), acc.cpu().numpy().astype(bool), eb.cpu().numpy(), ea.cpu().numpy()


# ---------------------------------------------------------------------------
# 1. one transition against the numpy trajectory
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('v', range(4))
@pytest.mark.parametrize('i', range(len(SHAPES)))
def test_one_transition_lies_inside_the_bounds_of_the_numpy_trajectory(device, i, v):
    K, N = SHAPES[i]
    C = CHAINS[(i + v) % 4]
    per_chain_tau, per_chain_dt = bool(v & 1), bool(v & 2)
    mode = _native.MODE_FMA if (i + v) % 2 else _native.MODE_EXACT
    var, prior_first = [(None, True), (5.0, True), (5.0, False)][(i + v) % 3]
    gp_where = (i + 2 * v) % 3                     # GammaPrior term absent / before / after
    L = 10
    A, ys, theta, tau = random_case(K, N, C)
    rs = np.random.RandomState(9)
    p0, u = rs.standard_normal((C, K)), rs.uniform(size=C)
    tau_v = tau if per_chain_tau else 2.5
    dt0 = RR.stable_dt(A, 4.0)
    dt_v = dt0 * rs.uniform(0.7, 1.0, size=C) if per_chain_dt else dt0
    taus = np.broadcast_to(np.asarray(tau_v, dtype=np.float64), (C,))
    dts = np.broadcast_to(np.asarray(dt_v, dtype=np.float64), (C,))
    const = gamma_term(taus)
    pre = const if gp_where == 1 else None
    post = const if gp_where == 2 else None
    q, acc, eb, ea = hmc_launch(device, A, ys, theta, p0, u, tau_v, dt_v, L, var, prior_first, pre, post, mode)
    case = RR.Case(A, ys, var, prior_first)
    worst = dict(q=0.0, eb=0.0, ea=0.0)
    for c in sorted(set(exact_chains(C) + [C // 3, (2 * C) // 3])):
        t = case.transition(theta[c], p0[c], taus[c], dts[c], L, None if pre is None else pre[c],
                            None if post is None else post[c])
        if acc[c]:
            err = np.abs(q[c] - t['q'])
            assert np.all(err <= t['bq']), (c, float(np.max(err / t['bq'])))
            worst['q'] = max(worst['q'], float(np.max(err / t['bq'])))
        else:
            assert np.array_equal(q[c], theta[c]), c
        worst['eb'] = max(worst['eb'], abs(eb[c] - t['e_before']) / t['b_before'])
        worst['ea'] = max(worst['ea'], abs(ea[c] - t['e_after']) / t['b_after'])
        assert abs(eb[c] - t['e_before']) <= t['b_before'], (c, eb[c], t['e_before'], t['b_before'])
        assert abs(ea[c] - t['e_after']) <= t['b_after'], (c, ea[c], t['e_after'], t['b_after'])
    print('K=%d N=%d C=%d: error / bound: state %.3g, E_before %.3g, E_after %.3g'
          % (K, N, C, worst['q'], worst['eb'], worst['ea']))
    assert np.all(np.isfinite(q)) and np.all(np.isfinite(eb)) and np.all(np.isfinite(ea))


# ---------------------------------------------------------------------------
# 2. accept flags
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('K,N,C,dt,L', [(4, 20, 400, 0.2, 10), (7, 37, 400, 0.13, 10)])
def test_accept_flags_follow_numpy_wherever_the_test_is_decided(device, K, N, C, dt, L):
    A, ys, theta, tau = random_case(K, N, C)
    rs = np.random.RandomState(9)
    p0, u = rs.standard_normal((C, K)), rs.uniform(size=C)
    q, acc, eb, ea = hmc_launch(device, A, ys, theta, p0, u, tau, dt, L, 5.0, True)
    case = RR.Case(A, ys, 5.0, True)
    want, dec, B = np.zeros(C, dtype=bool), np.zeros(C, dtype=bool), np.zeros(C)
    for c in range(C):
        t = case.transition(theta[c], p0[c], tau[c], dt, L)
        B[c] = t['b_before'] + t['b_after']
        dec[c] = RR.decided(t['dE'], u[c], B[c])
        want[c] = RR.accept_numpy(t['dE'], u[c])
    print('K=%d N=%d: undecided %d of %d, acceptance %.3f, largest B %.3g'
          % (K, N, int((~dec).sum()), C, want[dec].mean(), B.max()))
    assert np.array_equal(acc[dec], want[dec])
    assert (~dec).sum() <= 0.01 * C
    assert want[dec].mean() >= 0.2 and (~want[dec]).mean() >= 0.2


# ---------------------------------------------------------------------------
# 3. self-consistency, bit for bit
# ---------------------------------------------------------------------------
class Sweeps(object):
    """Buffers and arguments of binf_gibbs_linear_sample_n_f64 for one batch."""

    def __init__(self, device, K, N, C, n, move='hmc', seed=3, thin=1, L=6, t=None, **kw):
        self.device, self.K, self.N, self.C, self.n, self.thin, self.move = device, K, N, C, n, thin, move
        A, ys, theta, tau = random_case(K, N, C, seed=seed + 1000 * K + N)
        self.A, self.ys, self.theta, self.tau = A, ys, theta, tau
        self.t = t or (lambda a, dtype=torch.float64: plain(a, device, dtype))
        self.Ad, self.yd = self.t(A), self.t(ys)
        self.gamma_shape = 0.5 * N + 1.0
        self.base = dict(prior_means=self.t(np.zeros(K)), prior_vars=self.t(np.full(K, 5.0)), prior_first=True,
                         gp_where=2, gp_shape=1.0, gp_rate=0.2, gamma_shape=self.gamma_shape, gamma_rate=0.2)
        if move == 'hmc':
            self.base.update(move=_native.MOVE_HMC, nsteps=L, timestep=RR.stable_dt(A, 8.0))
        else:
            self.base.update(move=_native.MOVE_RWMC, stepsize=0.3 / np.sqrt(max(N, 1)))
        self.base.update(kw)

    def run(self, theta, tau, n, thin=1, rows=None, **kw):
        """n sweeps from (theta, tau) (device tensors); returns a dict of device tensors."""
        t, C, K = self.t, theta.shape[0], self.K
        o = dict(theta=t(np.zeros((C, K))), tau=t(np.zeros(C)), rc=t(np.zeros((n // thin, C, K))),
                 rt=t(np.zeros((n // thin, C))), acc=t(np.zeros((n, C), dtype=np.uint8), torch.uint8),
                 nacc=t(np.zeros(C, dtype=np.int64), torch.int64), eb=t(np.zeros((n, C))), ea=t(np.zeros((n, C))))
        args = dict(self.base)
        args.update(kw)
        if self.move != 'hmc':
            for k in ('eb', 'ea'):
                o.pop(k)
        _native.gibbs_linear_sample_n(
            theta, tau, o['theta'], o['tau'], self.Ad, self.yd, n, thin, rec_coefficients=o['rc'],
            rec_precision=o['rt'], accepted=o['acc'], n_accepted=o['nacc'], e_before=o.get('eb'),
            e_after=o.get('ea'), **args)
        return o


def equal(a, b, keys=None):
    for k in keys or a:
        if k in a and k in b:
            assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize('move', ['hmc', 'rwmc'])
@pytest.mark.parametrize('K,N,C', [(4, 20, 37), (9, 200, 300), (16, 129, 21), (3, 513, 9), (16, 1024, 5),
                                   (7, 37, 4100), (5, 920, 7)])
def test_n_sweeps_in_one_launch_are_n_launches_of_one_sweep(device, move, K, N, C):
    n, thin = 7, 2
    s = Sweeps(device, K, N, C, n, move)
    streams = ((11, 40, 130), (11, 41, 130), (11, 42, 130))
    th0, tau0 = dev_t(s.theta, device), dev_t(s.tau, device)
    adapt = dict(uprate=1.07, downrate=0.9) if move == 'hmc' else {}
    dt0 = lambda: torch.full((C,), float(s.base.get('timestep', 0.0)), dtype=torch.float64, device=device)
    dta, dtb = dt0(), dt0()
    n_adapt = 4                                     # the adaption window ends inside the launch
    one = s.run(th0, tau0, n, thin, streams=streams, dt_chain=dta if move == 'hmc' else None,
                n_adapt=n_adapt if move == 'hmc' else 0, **adapt)
    th, tau = th0, tau0
    nacc = torch.zeros(C, dtype=torch.int64, device=device)
    for i in range(n):
        st = tuple((seed, off + i * stride, stride) for seed, off, stride in streams)
        o = s.run(th, tau, 1, 1, streams=st, dt_chain=dtb if move == 'hmc' else None,
                  n_adapt=1 if (move == 'hmc' and i < n_adapt) else 0, **adapt)
        th, tau = o['theta'], o['tau']
        nacc += o['nacc']
        assert torch.equal(o['acc'][0], one['acc'][i]), i
        if move == 'hmc':
            assert torch.equal(o['eb'][0], one['eb'][i]) and torch.equal(o['ea'][0], one['ea'][i]), i
        if (i + 1) % thin == 0:
            r = (i + 1) // thin - 1
            assert torch.equal(o['theta'], one['rc'][r]) and torch.equal(o['tau'], one['rt'][r]), i
    assert torch.equal(th, one['theta']) and torch.equal(tau, one['tau']) and torch.equal(nacc, one['nacc'])
    if move == 'hmc':
        # the adaption window (4 of the 7 sweeps) left the same per-chain steps, and moved them:
        # no product of four factors 1.07 / 0.9 is 1
        assert torch.equal(dta, dtb) and not bool((dta == dt0()).any())
    assert bool(torch.isfinite(one['theta']).all()) and bool((one['tau'] > 0).all())


@pytest.mark.parametrize('move,zig', [('hmc', True), ('hmc', False), ('rwmc', True)])
def test_generated_draws_are_the_generator_kernels_output(device, move, zig):
    K, N, C, n, coff = 7, 37, 53, 4, 17
    s = Sweeps(device, K, N, C, n, move)
    streams = ((5, 100, 130), (5, 101, 130), (5, 102, 130))
    th0, tau0 = dev_t(s.theta, device), dev_t(s.tau, device)
    gen = s.run(th0, tau0, n, streams=streams, chain_offset=coff, zig=zig)
    p0 = torch.empty((n, C, K), dtype=torch.float64, device=device)
    u = torch.empty((n, C), dtype=torch.float64, device=device)
    g = torch.empty((n, C), dtype=torch.float64, device=device)
    for i in range(n):
        if move == 'hmc':
            _native.rng_fill('normal_zig' if zig else 'normal', p0[i], 5, 100 + 130 * i, elem_offset=coff * K)
        else:
            _native.rng_fill('uniform', p0[i], 5, 100 + 130 * i, elem_offset=coff * K)
            w = s.base['stepsize']
            p0[i] = -w + (w - -w) * p0[i]
        _native.rng_fill('uniform', u[i], 5, 101 + 130 * i, elem_offset=coff)
        _native.rng_fill('gamma', g[i], 5, 102 + 130 * i, shape=s.gamma_shape, elem_offset=coff)
    fed = s.run(th0, tau0, n, p0=p0, u=u, g=g)
    equal(gen, fed)


def test_rows_of_a_batch_do_not_depend_on_the_batch(device):
    K, N, C, n = 9, 200, 4100, 3
    s = Sweeps(device, K, N, C, n, 'hmc')
    streams = ((2, 7, 130), (2, 8, 130), (2, 9, 130))
    th0, tau0 = dev_t(s.theta, device), dev_t(s.tau, device)
    full = s.run(th0, tau0, n, streams=streams)
    # generated draws are keyed by the global chain index: a shard names its first chain
    for start, m in ((0, 1), (4099, 1), (33, 7), (4093, 7), (0, 64), (2001, 64), (5, 4090)):
        rows = slice(start, start + m)
        part = s.run(th0[rows].contiguous(), tau0[rows].contiguous(), n, streams=streams, chain_offset=start)
        for k in ('theta', 'tau', 'nacc'):
            assert torch.equal(part[k], full[k][rows]), (k, start, m)
        for k in ('rc', 'rt', 'acc', 'eb', 'ea'):
            assert torch.equal(part[k], full[k][:, rows]), (k, start, m)
    # supplied draws: a permuted batch
    rs = np.random.RandomState(4)
    p0, u = dev_t(rs.standard_normal((n, C, K)), device), dev_t(rs.uniform(size=(n, C)), device)
    g = dev_t(rs.gamma(s.gamma_shape, size=(n, C)), device)
    straight = s.run(th0, tau0, n, p0=p0, u=u, g=g)
    perm = torch.randperm(C, generator=torch.Generator().manual_seed(1)).to(device)
    moved = s.run(th0[perm].contiguous(), tau0[perm].contiguous(), n, p0=p0[:, perm].contiguous(),
                  u=u[:, perm].contiguous(), g=g[:, perm].contiguous())
    for k in ('theta', 'tau', 'nacc'):
        assert torch.equal(moved[k], straight[k][perm]), k
    for k in ('rc', 'rt', 'acc', 'eb', 'ea'):
        assert torch.equal(moved[k], straight[k][:, perm]), k
    # the single-transition entry point: a scalar precision is the per-chain arithmetic
    A, ys = s.A, s.ys
    p1, u1 = rs.standard_normal((C, K)), rs.uniform(size=C)
    dt = RR.stable_dt(A, 4.0)
    a = hmc_launch(device, A, ys, s.theta, p1, u1, 2.5, dt, 6, 5.0)
    b = hmc_launch(device, A, ys, s.theta, p1, u1, np.full(C, 2.5), np.full(C, dt), 6, 5.0)
    c = hmc_launch(device, A, ys, s.theta[40:47], p1[40:47], u1[40:47], 2.5, dt, 6, 5.0)
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x, y) and np.array_equal(x[40:47], z)


# ---------------------------------------------------------------------------
# 4. through the samplers: a user's model with resident=True
# ---------------------------------------------------------------------------
class Fourier(LinearForwardModel):
    def __init__(self, xs, n_modes, resident=False):
        self.xs, self.n_modes = np.asarray(xs, dtype=np.float64), n_modes
        rows = [np.ones_like(self.xs)]
        for m in range(1, n_modes + 1):
            rows += [np.cos(m * self.xs), np.sin(m * self.xs)]
        super(Fourier, self).__init__('fourier', np.vstack(rows), resident=resident)


LAUNCHES = ('hmc_sample_linear', 'gibbs_linear_sample_n', 'poly_leapfrog', 'linear_gauss_logp')


def spies(monkeypatch):
    return {n: Spy(monkeypatch, n) for n in LAUNCHES}


def fourier_posterior(resident, n_modes=3, N=40):
    xs, ys, A = fourier_case(N=N, n_modes=n_modes)
    lik = Likelihood('points', Fourier(xs, n_modes, resident=resident), GaussianErrorModel(ys))
    return posterior_of(lik, 2 * n_modes + 1), A, ys


def gibbs(device, resident, move, rng, C=300, L=8, n_modes=3, **kw):
    post, A, ys = fourier_posterior(resident, n_modes)
    K = 2 * n_modes + 1
    rs = np.random.RandomState(2)
    start = BinfState(dict(coefficients=dev_t(0.3 * rs.standard_normal((C, K)), device),
                           precision=dev_t(1.0 + rs.uniform(size=C), device)))
    if move == 'hmc':
        if rng is not None:
            kw['rng'] = rng
        return make_hmc_sampler(post, 0.03, L, start, record_energies=True, **kw)
    return make_sampler(post, 0.05, start, rng=rng)


@pytest.mark.parametrize('rng', ['device', 'host', 'supplied'])
def test_hmc_sampler_sample_n_is_n_sample_calls(device, monkeypatch, rng):
    n, C, K, tau = 50, 300, 7, 2.5
    post, A, ys = fourier_posterior(True)
    cond = post.conditional_factory(precision=tau)
    assert cond.native_hmc_spec('coefficients')[0] == 'linear_resident'
    rs = np.random.RandomState(6)
    theta = rs.standard_normal((C, K))
    mk = lambda: HMCSampler(cond, dev_t(theta, device), 0.03, 8, variable_name='coefficients',
                            record_energies=True, timestep_adaption_limit=20,
                            rng={'device': DeviceRNG(3, device), 'host': HostLegacyRNG(),
                                 'supplied': DeviceRNG(3, device)}[rng])
    a, b = mk(), mk()
    draws = {}
    if rng == 'supplied':
        draws = dict(p0=dev_t(rs.standard_normal((n, C, K)), device), u=dev_t(rs.uniform(size=(n, C)), device))
    sp = spies(monkeypatch)
    np.random.seed(5)
    xs = [a.sample(**{k: v[i] for k, v in draws.items()}).clone() for i in range(n)]
    assert sp['hmc_sample_linear'].calls == n and sp['gibbs_linear_sample_n'].calls == 0
    assert sp['poly_leapfrog'].calls == 0 and sp['linear_gauss_logp'].calls == 0
    np.random.seed(5)
    rec = b.sample_n(n, thin=5, **draws)
    assert sp['gibbs_linear_sample_n'].calls == 1 and sp['hmc_sample_linear'].calls == n
    assert sp['poly_leapfrog'].calls == 0 and sp['linear_gauss_logp'].calls == 0
    assert torch.equal(rec, torch.stack(xs)[4::5]) and torch.equal(b.state, xs[-1])
    assert torch.equal(a.n_accepted, b.n_accepted) and torch.equal(a.timestep, b.timestep)
    assert torch.equal(b.last_e_after[-1], a.last_e_after) and a.counter == b.counter == n
    if rng == 'device':
        assert a.rng.offset == b.rng.offset
    assert 0.3 < float(b.acceptance_rate.mean()) <= 1.0


@pytest.mark.parametrize('move,rng', [('hmc', 'device'), ('hmc', 'host'), ('rwmc', 'device'), ('rwmc', 'host')])
def test_gibbs_sampler_sample_n_is_n_sample_calls(device, monkeypatch, move, rng):
    n = 50
    mk = lambda: gibbs(device, True, move, (DeviceRNG(1, device) if rng == 'device' else
                                            (HostLegacyRNG() if move == 'hmc' else None)))
    a, b = mk(), mk()
    sp = spies(monkeypatch)
    np.random.seed(8)
    cs, ts = [], []
    for _ in range(n):
        st = a.sample()
        cs.append(st.variables['coefficients'].clone())
        ts.append(st.variables['precision'].clone())
    assert sp['gibbs_linear_sample_n'].calls == n          # every sweep one resident launch
    np.random.seed(8)
    rec = b.sample_n(n, thin=10)
    assert sp['gibbs_linear_sample_n'].calls == n + 1      # ... and 50 sweeps one launch
    assert sp['poly_leapfrog'].calls == 0 and sp['linear_gauss_logp'].calls == 0
    assert sp['hmc_sample_linear'].calls == 0
    assert torch.equal(rec['coefficients'], torch.stack(cs)[9::10])
    assert torch.equal(rec['precision'], torch.stack(ts)[9::10])
    assert torch.equal(b.state.variables['coefficients'], cs[-1])
    assert torch.equal(b.state.variables['precision'], ts[-1])
    sa, sb = a.subsamplers['coefficients'], b.subsamplers['coefficients']
    assert torch.equal(sa.acceptance_rate, sb.acceptance_rate)
    if rng == 'device':
        assert sa.rng.offset == sb.rng.offset
    if move == 'hmc':
        assert torch.equal(sb.last_e_after, sa.last_e_after)
        if rng == 'device':
            assert sa.rng.offset == 130 * n             # one generator serves the three draws
        # the per-variable loop of the same model (no sweep-level hook) moves the coefficients
        # with the same resident transition and the same draws; its precision draw goes through
        # the per-step log-prob, whose chi^2 is the MFMA tier's (rounding-level differences)
        c = mk()
        c.fused_sweep = False
        np.random.seed(8)
        assert torch.equal(c.sample().variables['coefficients'], cs[0])


def test_a_model_without_the_flag_makes_todays_calls(device, monkeypatch):
    n, L = 6, 8
    g = gibbs(device, False, 'hmc', DeviceRNG(1, device), L=L)
    sp = spies(monkeypatch)
    g.sample_n(n)
    assert sp['gibbs_linear_sample_n'].calls == 0 and sp['hmc_sample_linear'].calls == 0
    assert sp['poly_leapfrog'].calls == n and sp['linear_gauss_logp'].calls == 3 * n


@pytest.mark.parametrize('why', ['K=17', 'threshold', 'switched off'])
def test_a_declined_shape_takes_todays_path_and_stays_inside_the_bounds(device, monkeypatch, why):
    K, N, C, L, tau = (17, 60, 40, 8, 2.5) if why == 'K=17' else (7, 37, 40, 8, 2.5)
    A, ys, theta, _ = random_case(K, N, C)
    rs = np.random.RandomState(9)
    p0, u = rs.standard_normal((C, K)), rs.uniform(size=C)
    dt = RR.stable_dt(A, tau)
    lik = Likelihood('points', LinearForwardModel('basis', A, resident=True), GaussianErrorModel(ys))
    cond = posterior_of(lik, K).conditional_factory(precision=tau)
    assert (cond.native_hmc_spec('coefficients') is None) == (why == 'K=17')
    s = HMCSampler(cond, dev_t(theta, device), dt, L, variable_name='coefficients', record_energies=True)
    if why == 'threshold':
        monkeypatch.setattr(linear_resident, 'RESIDENT_MAX_WORK', float(C * N * K - 1))
    if why == 'switched off':
        s.fused_transition = False
    sp = spies(monkeypatch)
    out = s.sample(p0=dev_t(p0, device), u=dev_t(u, device)).cpu().numpy()
    assert sp['hmc_sample_linear'].calls == 0 and sp['poly_leapfrog'].calls == 1
    assert sp['linear_gauss_logp'].calls == 2
    acc = s.last_move_accepted.cpu().numpy()
    eb, ea = s.last_e_before.cpu().numpy(), s.last_e_after.cpu().numpy()
    gp = cond.priors['precision_prior']
    case = RR.Case(A, ys, 5.0, True)
    for c in range(C):
        t = case.transition(theta[c], p0[c], tau, dt, L, post=(gp.shape - 1.0) * np.log(tau) - tau * gp.rate)
        if acc[c]:
            assert np.all(np.abs(out[c] - t['q']) <= t['bq']), c
        else:
            assert np.array_equal(out[c], theta[c]), c
        assert abs(eb[c] - t['e_before']) <= t['b_before'] and abs(ea[c] - t['e_after']) <= t['b_after'], c


def test_checkpoint_and_resume_reproduce_the_uninterrupted_run(device):
    mk = lambda: gibbs(device, True, 'hmc', DeviceRNG(4, device), timestep_adaption_limit=12)
    a, b, c = mk(), mk(), mk()
    ra = a.sample_n(20, thin=2)
    rb1 = b.sample_n(8, thin=2)
    ckpt = checkpoint.state_dict(gibbs=b)
    checkpoint.load_state_dict(ckpt, gibbs=c)
    rc2 = c.sample_n(12, thin=2)
    for k in ('coefficients', 'precision'):
        assert torch.equal(torch.cat([rb1[k], rc2[k]]), ra[k]), k
        assert torch.equal(c.state.variables[k], a.state.variables[k]), k
    sa, sc = a.subsamplers['coefficients'], c.subsamplers['coefficients']
    assert torch.equal(sa.timestep, sc.timestep) and torch.equal(sa.n_accepted, sc.n_accepted)
    assert sa.rng.offset == sc.rng.offset


# ---------------------------------------------------------------------------
# 5. Gibbs sweeps against a numpy restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('K,N,C', [(4, 20, 60), (9, 200, 40), (16, 129, 12)])
def test_three_gibbs_sweeps_against_numpy(device, K, N, C):
    n, L, beta = 3, 8, 0.2
    s = Sweeps(device, K, N, C, n, 'hmc', L=L)
    dt = s.base['timestep']
    rs = np.random.RandomState(12)
    p0, u = rs.standard_normal((n, C, K)), rs.uniform(size=(n, C))
    g = rs.gamma(s.gamma_shape, size=(n, C))
    o = s.run(dev_t(s.theta, device), dev_t(s.tau, device), n, p0=dev_t(p0, device), u=dev_t(u, device),
              g=dev_t(g, device))
    rc, rt = o['rc'].cpu().numpy(), o['rt'].cpu().numpy()
    acc = o['acc'].cpu().numpy().astype(bool)
    eb, ea = o['eb'].cpu().numpy(), o['ea'].cpu().numpy()
    case = RR.Case(s.A, s.ys, 5.0, True)
    undecided = 0
    for c in range(C):
        # the numpy sweep: HMC on the coefficients, then tau = g / (0.5 chi^2 + beta)
        q, tau = s.theta[c], s.tau[c]
        qs, taus, flags, es = [], [], [], []
        for i in range(n):
            t = case.transition(q, p0[i, c], tau, dt, L, post=(1.0 - 1.0) * np.log(tau) - tau * 0.2)
            a = bool(RR.accept_numpy(t['dE'], u[i, c]))
            q = t['q'] if a else q
            tau = g[i, c] / (0.5 * np.sum((q.dot(s.A) - s.ys) ** 2) + beta)
            qs.append(q), taus.append(tau), flags.append(a), es.append(t)
        b = PB.gibbs_bounds(case.pb, qs, flags, p0[:, c], taus, s.tau[c], s.theta[c], dt, L, beta)
        for i in range(n):
            B = es[i]['b_before'] + es[i]['b_after'] + b[i]['be_before'] + b[i]['be_after']
            if not RR.decided(es[i]['dE'], u[i, c], B):
                undecided += 1                 # a coin toss at rounding level: the chain's later
                break                          # sweeps have no numpy counterpart
            assert acc[i, c] == flags[i], (i, c)
            assert np.all(np.abs(rc[i, c] - qs[i]) <= b[i]['bq'] + 4 * PB.U * np.abs(qs[i])), (i, c)
            assert abs(rt[i, c] - taus[i]) <= b[i]['btau'] * taus[i], (i, c)
            assert abs(eb[i, c] - es[i]['e_before']) <= es[i]['b_before'] + b[i]['be_before'], (i, c)
            assert abs(ea[i, c] - es[i]['e_after']) <= es[i]['b_after'] + b[i]['be_after'], (i, c)
    assert undecided <= max(1, C // 20)


# ---------------------------------------------------------------------------
# 6. statistics
# ---------------------------------------------------------------------------
def test_resident_model_samples_its_analytic_gaussian(device, monkeypatch):
    """The rule and the numbers of test_gpu_linear.py::test_user_model_samples_its_analytic_gaussian,
    drawn through sample_n."""
    n_modes, tau, C = 3, 2.5, 4096
    K = 2 * n_modes + 1
    xs, ys, A = fourier_case(n_modes=n_modes, tau=tau)
    P = tau * A @ A.T + np.eye(K) / 5.0
    cov = np.linalg.inv(P)
    mean = cov @ (tau * A @ ys)
    rs = np.random.RandomState(5)
    lik = Likelihood('points', Fourier(xs, n_modes, resident=True), GaussianErrorModel(ys))
    cond = posterior_of(lik, K).conditional_factory(precision=tau)
    start = torch.from_numpy(mean + rs.standard_normal((C, K)) @ np.linalg.cholesky(cov).T).to(device)
    s = HMCSampler(cond, start, 0.03, 40, variable_name='coefficients', rng=DeviceRNG(3, device))
    sp = spies(monkeypatch)
    sweeps, burn = 120, 40
    s.sample_n(burn, record=False)
    x = s.sample_n(sweeps - burn, thin=5)
    assert sp['gibbs_linear_sample_n'].calls == 2 and sp['poly_leapfrog'].calls == 0
    acc = float(s.acceptance_rate.mean())
    assert 0.6 < acc <= 1.0
    x = x.cpu().numpy()
    assert x.shape == (16, C, K)
    se = np.sqrt(np.diag(cov) / C)
    assert (np.abs(x.mean((0, 1)) - mean) < 6 * se).all()
    emp = np.cov(x.reshape(-1, K).T)
    assert np.abs(emp - cov).max() < 0.15 * np.abs(cov).max()


def test_gibbs_posterior_means_agree_with_the_per_variable_loop(device):
    C, burn, keep, thin = 1024, 150, 300, 5
    means, ses = [], []
    for resident, seed in ((True, 21), (False, 22)):
        g = gibbs(device, resident, 'hmc', DeviceRNG(seed, device), C=C, L=15)
        if resident:
            g.sample_n(burn, record=False)
            rec = g.sample_n(keep, thin=thin)
            x = torch.cat([rec['coefficients'], rec['precision'][:, :, None]], dim=2)
        else:
            rows = []
            for i in range(burn + keep):
                st = g.sample()
                if i >= burn and (i - burn + 1) % thin == 0:
                    rows.append(torch.cat([st.variables['coefficients'], st.variables['precision'][:, None]], dim=1))
            x = torch.stack(rows)
        per_chain = x.mean(0).cpu().numpy()                  # [C x (K + 1)]
        means.append(per_chain.mean(0))
        ses.append(per_chain.std(0, ddof=1) / np.sqrt(C))
    z = np.abs(means[0] - means[1]) / np.sqrt(ses[0] ** 2 + ses[1] ** 2)
    print('largest |difference| / combined standard error: %.2f' % z.max())
    assert (z < 6).all(), z


# ---------------------------------------------------------------------------
# 7. guard zones
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('K,N,C', [(1, 1, 1), (4, 20, 5), (7, 37, 37), (9, 200, 33), (16, 129, 9),
                                   (3, 513, 3), (5, 920, 2), (16, 1024, 3), (13, 64, 300)])
def test_kernels_stay_inside_their_buffers(device, K, N, C):
    n = 3
    rs = np.random.RandomState(K + N)
    outs = []
    for make in (Guarded(device), None):
        t = make if make is not None else (lambda a, dtype=torch.float64: plain(a, device, dtype))
        res = []
        for move in ('hmc', 'rwmc'):
            s = Sweeps(device, K, N, C, n, move, t=t)
            p0 = rs.standard_normal((n, C, K)) * (1.0 if move == 'hmc' else 0.01)
            o = s.run(t(s.theta), t(s.tau), n, p0=t(p0), u=t(rs.uniform(size=(n, C))),
                      g=t(rs.gamma(s.gamma_shape, size=(n, C))), dt_chain=t(np.full(C, s.base.get('timestep', 0.1))),
                      n_adapt=2 if move == 'hmc' else 0)
            res += [o[k].clone().cpu() for k in sorted(o)]
            # generated draws, in place: theta_out aliasing theta0
            th, tau = t(s.theta), t(s.tau)
            _native.gibbs_linear_sample_n(th, tau, th, tau, s.Ad, s.yd, n, 1,
                                          streams=((1, 0, 130), (1, 1, 130), (1, 2, 130)), **s.base)
            res += [th.clone().cpu(), tau.clone().cpu()]
        A, ys, theta, tau = random_case(K, N, C)
        for q_out in (None, 'alias'):
            hm = Guarded(device) if make is not None else None
            r = hmc_launch(device, A, ys, theta, rs.standard_normal((C, K)), rs.uniform(size=C), tau,
                           RR.stable_dt(A, 4.0), 5, 5.0, t=hm or None, q_out=q_out)
            if hm is not None:
                hm.check()
            res += [torch.from_numpy(np.asarray(x)) for x in r]
        if make is not None:
            make.check()
        outs.append(res)
        rs = np.random.RandomState(K + N)
    for a, b in zip(*outs):
        assert torch.equal(a, b)
        assert not (a.is_floating_point() and bool(torch.isnan(a).any()))


# ---------------------------------------------------------------------------
# 8. a non-finite coefficient stays in its chain
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('K,N,C', [(7, 37, 40), (9, 200, 70), (3, 513, 5), (16, 1024, 4)])
@pytest.mark.parametrize('bad', [np.nan, np.inf])
def test_a_non_finite_coefficient_is_rejected_and_stays_in_its_chain(device, K, N, C, bad):
    n = 3
    s = Sweeps(device, K, N, C, n, 'hmc')
    rs = np.random.RandomState(1)
    draws = dict(p0=dev_t(rs.standard_normal((n, C, K)), device), u=dev_t(rs.uniform(size=(n, C)), device))
    dirty = s.theta.copy()
    c_bad = C // 2
    dirty[c_bad, K - 1] = bad
    tau0 = dev_t(s.tau, device)
    clean = s.run(dev_t(s.theta, device), tau0, n, keep_precision=True, **draws)
    got = s.run(dev_t(dirty, device), tau0, n, keep_precision=True, **draws)
    others = torch.tensor([c for c in range(C) if c != c_bad], device=device)
    for k in ('theta', 'nacc'):
        assert torch.equal(got[k][others], clean[k][others]), k
    for k in ('rc', 'acc', 'eb', 'ea'):
        assert torch.equal(got[k][:, others], clean[k][:, others]), k
    assert not bool(got['acc'][:, c_bad].any()) and int(got['nacc'][c_bad]) == 0
    kept = got['theta'][c_bad].cpu().numpy()
    assert np.array_equal(kept[:K - 1], dirty[c_bad, :K - 1])
    assert (np.isnan(kept[K - 1]) and np.isnan(bad)) or kept[K - 1] == bad
    # the single transition, too
    p1, u1 = rs.standard_normal((C, K)), rs.uniform(size=C)
    dt = RR.stable_dt(s.A, 4.0)
    a = hmc_launch(device, s.A, s.ys, s.theta, p1, u1, s.tau, dt, 5, 5.0)
    b = hmc_launch(device, s.A, s.ys, dirty, p1, u1, s.tau, dt, 5, 5.0)
    keep = np.arange(C) != c_bad
    for x, y in zip(a, b):
        assert np.array_equal(x[keep], y[keep])
    assert not b[1][c_bad] and np.array_equal(b[0][c_bad, :K - 1], dirty[c_bad, :K - 1])


# ---------------------------------------------------------------------------
# 9. the example script
# ---------------------------------------------------------------------------
def test_example_linear_basis_resident_recovers_the_signal(device, monkeypatch):
    path = os.path.join(os.path.dirname(GOLDEN_DIR), os.pardir, 'examples', 'linear_basis.py')
    spec = importlib.util.spec_from_file_location('linear_basis_resident', os.path.normpath(path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    sp = spies(monkeypatch)
    coeffs, prec = mod.main(['--chains', '256', '--iterations', '300', '--burn-in', '100', '--thin', '20',
                             '--modes', '3', '--data', '150', '--resident'])
    assert sp['gibbs_linear_sample_n'].calls == 2 and sp['poly_leapfrog'].calls == 0
    assert coeffs.shape == (10, 256, 7) and prec.shape[:2] == (10, 256)
    rs = np.random.RandomState(0)
    truth = rs.standard_normal(7) / (1.0 + np.arange(7) // 2)
    c = coeffs.reshape(-1, 7).cpu().numpy()
    assert np.all(np.abs(c.mean(0) - truth) < 5 * c.std(0) + 0.05)
    assert 2.0 < float(prec.mean()) < 8.0
