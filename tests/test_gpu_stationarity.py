"""Exact stationarity tests on the device: every transition route must leave its target
invariant.  What the bit-for-bit suites cannot see -- a wrong sign in the accept test, an
energy without one of its terms, a conditional draw with the wrong shape parameter -- a
restatement carries too; these tests do not restate anything.

Each route starts from EXACT draws of its target made on the host (``tests/stationarity.py``:
isotropic and diagonal Gaussians, the tempered ladder, the linear-Gaussian conditional whitened
by its Cholesky factor, the joint (coefficients, precision) posterior of the Gibbs loop through
a 40-digit quadrature of the precision's marginal), runs with the adaption off and the draws of
``DeviceRNG(seed)`` unless stated, and evaluates at the last time point.  Chains are independent,
so under invariance the C end states are again i.i.d. exact draws and every statistic has a known
null law: pooled chi^2 at its exact quantiles, the pooled mean, the Dvoretzky-Kiefer-Wolfowitz
bound, and the energy identity E exp(E_before - E_after) = 1 with a derived variance.  Each test
function has a total level of 1e-9 (Bonferroni over its parametrisations and statistics; the
energy identity 1e-6 of its own), fixed seeds, the step tuned to 0.6 ... 0.8 acceptance (asserted),
and asserts which tier ran.  No threshold comes from device output.

Shapes, steps and seeds are ``stationarity.ROUTES``; ``tests/test_stationarity.py`` shows on the
host sampler that at exactly these settings always-accept, a flipped sign of Delta E, a dropped
kinetic term, always-swap and a Gamma shape off by one are each rejected with |z| at least twice
the threshold.

The Gibbs target follows the reference's own Gamma draw, shape ``0.5 n + prior.shape - 1``
(``binf/example/samplers.py:27-32``; ``oracle/ref_numpy.py:296-299``, "one less than the textbook
value") at the conditional prior's rate = shape (quirk Q6, ``binf_amd/example/priors.py:36-43``):
the loop is exactly invariant for the posterior under a Gamma prior of shape ``prior.shape - 1``
and rate ``prior.shape``, and that is the target here (``prior.shape = 2``, so it is proper).

Out of scope:
* the pair-distance posterior, which has no exact sampler;
* the adaptive phase itself (step sizes, the windowed metric), which is not invariant by
  construction -- only the state AFTER a finished warm-up is tested;
* mildly wrong accept rules below the shown power: a test 10 % too lenient (``0.9 u < ...``)
  gives z = 1.7 ... 4.6 at one time point and is not decided by these tests.
"""
import numpy as np
import pytest
import torch

import stationarity as S
from binf_amd import _native
from binf_amd.example.likelihood import POLYVAL, ForwardModel, GaussianErrorModel
from binf_amd.example.priors import GammaPrior, GaussianPrior
from binf_amd.example.samplers import make_hmc_sampler, make_sampler
from binf_amd.model.linear import LinearForwardModel
from binf_amd.pdf import IsotropicGaussian, native_gauss
from binf_amd.pdf.likelihoods import Likelihood
from binf_amd.pdf.posteriors import Posterior
from binf_amd.samplers import BinfState
from binf_amd.samplers.hmc import HMCSampler
from binf_amd.samplers.replica import ReplicaExchangeSampler
from binf_amd.samplers.rng import DeviceRNG
from binf_amd.samplers.warmup import WindowedWarmup

pytestmark = pytest.mark.gpu


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device)


class Spy(object):
    """Counts the calls of ``_native.<name>`` (the hooks look it up per call)."""

    def __init__(self, monkeypatch, name):
        self.calls = 0
        self.fn = getattr(_native, name)
        monkeypatch.setattr(_native, name, self)

    def __call__(self, *a, **kw):
        self.calls += 1
        return self.fn(*a, **kw)


def spies(monkeypatch, *names):
    return {n: Spy(monkeypatch, n) for n in names}


def verdict(name, acceptance, x, tau=None, energies=None):
    """Print every statistic with its interval and the acceptance rate, then assert them."""
    x = x.cpu().numpy()
    tau = None if tau is None else tau.cpu().numpy()
    if energies is not None:
        energies = tuple(e.cpu().numpy() for e in energies)
    checks = S.evaluate(name, x, tau, energies)
    print('%s: acceptance %.4f, level per statistic %.3g' % (name, acceptance, S.alpha_of(name)))
    for c in checks:
        print('    ' + S.describe(c))
    assert np.isfinite(x).all()
    assert S.ACCEPT_WINDOW[0] < acceptance < S.ACCEPT_WINDOW[1], acceptance
    bad = [S.describe(c) for c in checks if not S.inside(c)]
    assert not bad, bad


def rate(sampler):
    return float(sampler.acceptance_rate.mean())


# ---------------------------------------------------------------------------
# the Gaussian kind: IsotropicGaussian(k = 2.5, x0 = 0.3), so that a dropped k or x0 shows
# ---------------------------------------------------------------------------
GAUSS_LAUNCHES = ('hmc_sample_n_gauss_rng', 'hmc_sample_n_gauss', 'hmc_gauss_rng_draws', 'hmc_sample_gauss',
                  'hmc_sample_gauss_big', 'hmc_sample_gauss_big_rng', 'hmc_sample_n_gauss_big', 'accept_select')


def gauss_sampler(device, name, **kw):
    r = S.ROUTES[name]
    fused = {'sample_n_rng_always': 'always', 'sample': False, 'per_step': False, 'graph': False}.get(r['how'], True)
    rng = DeviceRNG(r['seed'], device, fused=fused)
    s = HMCSampler(IsotropicGaussian(r['k'], r['x0']), dev(S.start_of(name), device), r['dt'], r['L'],
                   variable_name='x', rng=rng, mode=r['mode'], **kw)
    assert s.timestep_adaption_limit == 0
    return r, s


@pytest.mark.parametrize('name', S.parametrisations('gauss'))
def test_gaussian_whole_transition_kernels_keep_the_target(device, monkeypatch, name):
    """The persistent ``sample_n`` kernel with the draws made in the kernel (4096 x 64, 4096 x 33:
    one wave per chain; 1024 x 1024 with ``fused='always'``: by default that batch spreads a chain
    over 4 waves and gets the same draws written out first -- the split route, also here), with
    supplied numpy draws, in FMA mode, and the single-transition kernel behind ``sample()``."""
    r, s = gauss_sampler(device, name)
    C, D, n, how = r['C'], r['D'], r['n'], r['how']
    sp = spies(monkeypatch, *GAUSS_LAUNCHES)
    assert s._fused_spec('x', D, C) == ('gauss', r['k'], r['x0']) and _native.gauss_persist_covers(D)
    waves = _native.gauss_waves_per_chain(C, D)
    if how == 'sample_n_rng':
        assert waves == 1 and native_gauss.draws_in_kernel(s, C, D)
        x = s.sample_n(n, thin=n)[-1]
        want = {'hmc_sample_n_gauss_rng': 1}
    elif how == 'sample_n_rng_always':
        assert waves == 4 and native_gauss.draws_in_kernel(s, C, D) and s.rng.fused == 'always'
        x = s.sample_n(n, thin=n)[-1]
        want = {'hmc_sample_n_gauss_rng': 1}
    elif how == 'sample_n_split':
        assert waves == 4 and not native_gauss.draws_in_kernel(s, C, D)
        x = s.sample_n(n, thin=n)[-1]
        want = {'hmc_gauss_rng_draws': 1, 'hmc_sample_n_gauss': 1}
    elif how == 'sample_n_supplied':
        rs = np.random.RandomState(r['seed'] + 7000)
        p0, u = dev(rs.standard_normal((n, C, D)), device), dev(rs.uniform(size=(n, C)), device)
        x = s.sample_n(n, thin=n, p0=p0, u=u)[-1]
        want = {'hmc_sample_n_gauss': 1}
    else:
        assert how == 'sample' and not native_gauss.fused_rng(s, 'x', D)
        for _ in range(n):
            x = s.sample()
        want = {'hmc_sample_gauss': n}
    assert {k: v.calls for k, v in sp.items() if v.calls} == want
    assert s.counter == n and torch.equal(x, s.state)
    verdict(name, rate(s), x)


@pytest.mark.parametrize('name', S.parametrisations('gauss_steps'))
def test_gaussian_per_step_tier_keeps_the_target_and_the_energy_identity(device, monkeypatch, name):
    """``fused_transition = False``: energies, leapfrog launches and ``binf_accept_select_f64``
    one by one, eager and replayed from one HIP graph (``graph='always'``)."""
    r, s = gauss_sampler(device, name, record_energies=True, graph='always' if S.ROUTES[name]['how'] == 'graph' else False)
    s.fused_transition = False
    assert s._fused_spec('x', r['D'], r['C']) is None
    sp = spies(monkeypatch, *GAUSS_LAUNCHES)
    for _ in range(r['n']):
        x = s.sample()
    calls = {k: v.calls for k, v in sp.items() if v.calls}
    if r['how'] == 'graph':
        assert s._graph_captures == 1 and len(s._graphs) == 1
        assert calls == {'accept_select': 2}                     # the eager first call and the capture
    else:
        assert calls == {'accept_select': r['n']}
    verdict(name, rate(s), x, energies=(s.last_e_before, s.last_e_after))


@pytest.mark.parametrize('name', S.parametrisations('gauss_long'))
def test_gaussian_long_chain_kernels_keep_the_target(device, monkeypatch, name):
    """D = 8200 > 8192: the chunked kernels of ``csrc/hmc_gauss_big.hip`` behind ``sample()`` and
    ``sample_n`` (67 MB of state)."""
    r, s = gauss_sampler(device, name)
    assert not _native.gauss_persist_covers(r['D']) and _native.gauss_waves_per_chain(r['C'], r['D']) == 0
    sp = spies(monkeypatch, *GAUSS_LAUNCHES)
    if r['how'] == 'long_sample':
        for _ in range(r['n']):
            x = s.sample()
        want = {'hmc_sample_gauss_big_rng': r['n']}
    else:
        x = s.sample_n(r['n'], thin=r['n'])[-1]
        want = {'hmc_sample_n_gauss_big': 1}
    assert {k: v.calls for k, v in sp.items() if v.calls} == want
    verdict(name, rate(s), x)


# ---------------------------------------------------------------------------
# the diagonal-metric tier
# ---------------------------------------------------------------------------
class DiagGauss(object):
    """A user's torch PDF: log p(x) = -1/2 sum (x / sigma)^2."""

    def __init__(self, sigma):
        self.sigma = sigma

    def log_prob(self, x):
        z = x / self.sigma
        return -0.5 * (z * z).sum(dim=1)

    def gradient(self, x):
        return x / (self.sigma * self.sigma)


METRIC_LAUNCHES = ('leapfrog_kick_scaled', 'leapfrog_drift_scaled', 'leapfrog_kick_drift_scaled', 'leapfrog_kick_drift',
                   'accept_select')


@pytest.mark.parametrize('name', S.parametrisations('metric'))
def test_metric_tier_keeps_the_target_under_a_mismatched_metric(device, monkeypatch, name):
    """sigma = 1 ... 100; the metric is sigma times fixed factors in [0.5, 2], another set per
    row (``[3 x 8]``: chain c takes row c % 3; ``[8]``; FMA mode): invariance must hold for any
    positive scale.  Standardised by sigma, per group and pooled, plus the energy identity."""
    r = S.ROUTES[name]
    C, D, G, n, L = r['C'], r['D'], r['G'], r['n'], r['L']
    scale = S.metric_rows(S.SIGMA8, G)
    metric = dev(scale if G > 1 else scale[0], device)
    assert tuple(metric.shape) == ((G, D) if G > 1 else (D,)) and C % 3 == 0
    s = HMCSampler(DiagGauss(dev(S.SIGMA8, device)), dev(S.start_of(name), device), r['dt'], L, variable_name='x',
                   rng=DeviceRNG(r['seed'], device), mode=r['mode'], record_energies=True, metric=metric)
    assert s._fused_spec('x', D, C) is None and tuple(s.metric_scale.shape) == (G, D)
    sp = spies(monkeypatch, *METRIC_LAUNCHES)
    for _ in range(n):
        x = s.sample()
    assert {k: v.calls for k, v in sp.items() if v.calls} == {
        'leapfrog_kick_scaled': 2 * n, 'leapfrog_drift_scaled': n, 'leapfrog_kick_drift_scaled': n * (L - 1),
        'accept_select': n}
    assert np.array_equal(s.metric_scale.cpu().numpy(), scale)
    verdict(name, rate(s), x, energies=(s.last_e_before, s.last_e_after))


def test_the_state_after_a_finished_warmup_stays_invariant(device):
    """``WindowedWarmup(70, 10, 10, 10)`` run to its end on the same target (from twice
    over-dispersed starts, step 1.0, rates 1.06 / 0.9), then exact draws in ``sampler.state`` and 40
    more transitions: the target stays invariant and neither the step sizes nor the metric move
    any more, bit for bit."""
    name = 'after_warmup'
    r = S.ROUTES[name]
    C, D = r['C'], r['D']
    rs = np.random.RandomState(r['seed'] + 7000)
    s = HMCSampler(DiagGauss(dev(S.SIGMA8, device)), dev(2.0 * S.target_of(name).sample(rs, C, D), device),
                   r['dt'], r['L'], adaption_uprate=r['uprate'], adaption_downrate=r['downrate'], variable_name='x',
                   rng=DeviceRNG(r['seed'], device))
    w = WindowedWarmup(s, r['n_warmup'], init_buffer=10, term_buffer=10, base_window=10)
    assert w.windows == [(10, 20), (20, 60)]
    w.run()
    assert w.done and s.counter == r['n_warmup'] and s.timestep_adaption_limit == r['n_warmup'] + 1
    dt, scale = s.timestep.clone(), s.metric_scale.clone()
    assert dt.shape == (C,) and float(dt.min()) > 0.0 and not torch.equal(scale, torch.ones_like(scale))
    print('learnt scale / sigma: %s, step sizes %.3f ... %.3f'
          % ((scale.cpu().numpy()[0] / S.SIGMA8).round(3), float(dt.min()), float(dt.max())))
    s.state = dev(S.start_of(name), device)
    before = s.n_accepted.clone()
    for _ in range(r['n']):
        x = s.sample()
    assert s._fused_spec('x', D, C) is None
    assert torch.equal(s.timestep, dt) and torch.equal(s.metric_scale, scale)
    acceptance = float((s.n_accepted - before).to(torch.float64).mean()) / r['n']
    verdict(name, acceptance, x)


# ---------------------------------------------------------------------------
# polynomial and linear kinds: the coefficients' conditional at a fixed precision
# ---------------------------------------------------------------------------
LINEAR_LAUNCHES = ('hmc_sample_poly', 'gibbs_poly_sample_n', 'hmc_sample_linear', 'gibbs_linear_sample_n',
                   'poly_leapfrog', 'accept_select')


def posterior_of(name, gamma_prior):
    """The example's posterior on the route's data: polynomial, linear (dense design matrix) or
    linear with ``resident=True``; the likelihood is called 'points' as the Gibbs samplers expect."""
    r = S.ROUTES[name]
    xs, ys, A = S.design_of(name)
    how = r.get('model') or r['how']
    if xs is not None:
        fwm = ForwardModel(xs, POLYVAL)
    else:
        fwm = LinearForwardModel('basis', A, resident=not how.endswith('per_step'))
    lik = Likelihood('points', fwm, GaussianErrorModel(ys))
    return Posterior({lik.name: lik},
                     {'precision_prior': gamma_prior,
                      'coefficients_prior': GaussianPrior(np.zeros(r['K']), np.full(r['K'], r['prior_var']))})


@pytest.mark.parametrize('name', S.parametrisations('linear'))
def test_coefficient_conditional_keeps_its_gaussian_on_every_tier(device, monkeypatch, name):
    """K = 4, N = 20, C = 4096: the fused small-data transition (``sample()``) and the
    chain-resident sweep kernel with the precision draw off (``sample_n``) of the polynomial kind;
    N = 136 > 128 data points: its one-wave-per-chain kernel; a linear model with
    ``resident=True`` through both resident kernels; and both kinds on the per-step tier, whose
    force is the MFMA gradient inside ``binf_poly_leapfrog_f64``.  The force omits the prior, the
    energy has it (quirk Q4): the target is the full conditional all the same."""
    r = S.ROUTES[name]
    C, K, N, n, how = r['C'], r['K'], r['N'], r['n'], r['how']
    cond = posterior_of(name, GammaPrior(1.0, 0.2)).conditional_factory(precision=r['tau'])
    s = HMCSampler(cond, dev(S.start_of(name), device), r['dt'], r['L'], variable_name='coefficients',
                   rng=DeviceRNG(r['seed'], device))
    if how.endswith('per_step'):
        s.fused_transition = False
        assert s._fused_spec('coefficients', K, C) is None
        assert cond.native_leapfrog_spec('coefficients')[0] == ('poly' if how.startswith('poly') else 'linear')
    else:
        spec = s._fused_spec('coefficients', K, C)
        assert spec is not None and spec[0] == ('poly' if how.startswith('poly') else 'linear_resident')
        if spec[0] == 'poly':
            assert not native_lane_layout(s, spec, C) and (N > 128) == (name == 'poly_wave_sample')
    sp = spies(monkeypatch, *LINEAR_LAUNCHES)
    if how.endswith('sample_n'):
        x = s.sample_n(n, thin=n)[-1]
    else:
        for _ in range(n):
            x = s.sample()
    want = {'poly_sample': {'hmc_sample_poly': n}, 'poly_sample_n': {'gibbs_poly_sample_n': 1},
            'poly_per_step': {'poly_leapfrog': n, 'accept_select': n},
            'linear_sample': {'hmc_sample_linear': n}, 'linear_sample_n': {'gibbs_linear_sample_n': 1},
            'linear_per_step': {'poly_leapfrog': n, 'accept_select': n}}[how]
    assert {k: v.calls for k, v in sp.items() if v.calls} == want
    verdict(name, rate(s), x)


def native_lane_layout(sampler, spec, C):
    from binf_amd.example import native_poly
    return native_poly.lane_layout(sampler, spec, C)


# ---------------------------------------------------------------------------
# the joint (coefficients, precision) Gibbs loop
# ---------------------------------------------------------------------------
GIBBS_LAUNCHES = ('gibbs_poly_sample_n', 'gibbs_linear_sample_n', 'gamma_precision_update', 'hmc_sample_poly',
                  'rwmc_accept')


@pytest.mark.parametrize('name', S.parametrisations('gibbs'))
def test_gibbs_loop_keeps_the_joint_posterior(device, monkeypatch, name):
    """K = 3, N = 24, C = 4096, 30 sweeps from exact draws of (theta, tau): the multi-sweep launch
    of the polynomial and of the resident linear kind, each with the HMC and with the RWMC move,
    and the per-variable ``sample()`` loop -- the device Gamma draw, the chi^2 reductions, the
    precision update and the RWMC accept in one exact test.  F(tau) uniform (DKW, and the mean of
    its normal score), the whitened theta | tau chi^2 with C K degrees of freedom and normal by DKW,
    F(tau) uncorrelated with |z|^2."""
    r = S.ROUTES[name]
    C, n = r['C'], r['n']
    post = posterior_of(name, GammaPrior(r['prior_shape'], r['prior_rate']))
    theta, tau = S.start_of(name)
    start = BinfState(dict(coefficients=dev(theta, device), precision=dev(tau, device)))
    rng = DeviceRNG(r['seed'], device)
    if r['move'] == 'hmc':
        gips = make_hmc_sampler(post, r['dt'], r['L'], start, rng=rng)
    else:
        gips = make_sampler(post, r['stepsize'], start, rng=rng)
    ps = gips.subsamplers['precision']
    # the reference's draw: shape 0.5 n + prior.shape - 1 at the conditional prior's rate = shape
    assert ps._calculate_shape() == S.gibbs_shape(r) == 13.0 and ps._get_prior().rate == r['prior_shape']
    sp = spies(monkeypatch, *GIBBS_LAUNCHES)
    fused = 'gibbs_poly_sample_n' if r['model'] == 'poly' else 'gibbs_linear_sample_n'
    if r['how'] == 'sample_n':
        rec = gips.sample_n(n, thin=n)
        x, t = rec['coefficients'][-1], rec['precision'][-1]
        want = {fused: 1}
    else:
        gips.fused_sweep = False
        for _ in range(n):
            st = gips.sample()
        x, t = st.variables['coefficients'], st.variables['precision']
        want = {'gamma_precision_update': n, 'hmc_sample_poly': n}
    assert {k: v.calls for k, v in sp.items() if v.calls} == want
    assert bool((t > 0).all())
    verdict(name, rate(gips.subsamplers['coefficients']), x, tau=t)


# ---------------------------------------------------------------------------
# replica exchange
# ---------------------------------------------------------------------------
class Harmonic(object):
    """A torch PDF: log p_c(x) = -1/2 k_c sum x^2."""

    def __init__(self, k):
        self.k = k

    def log_prob(self, x):
        return -0.5 * self.k * (x * x).sum(dim=1)

    def gradient(self, x):
        return self.k[:, None] * x


def test_replica_exchange_keeps_every_slot_in_its_distribution(device):
    """R = 4 slots at k = 1, 1/2, 1/4, 1/8, 1024 ladders, D = 8, 40 rounds of one HMC transition
    and one swap round from exact draws: the pooled chi^2 of every slot at its exact quantiles."""
    name = 'ladder'
    r = S.ROUTES[name]
    R, n_ladders, D, n = r['R'], r['n_ladders'], r['D'], r['n']
    k = dev(S.ladder(n_ladders)[1], device)
    inner = HMCSampler(Harmonic(k), dev(S.start_of(name), device), r['dt'] / k.sqrt(), r['L'], variable_name='x',
                       rng=DeviceRNG(r['seed'], device))
    assert inner._fused_spec('x', D, R * n_ladders) is None
    re = ReplicaExchangeSampler(inner, R)
    for _ in range(n):
        x = re.sample()
    assert re.round == n and inner.counter == n
    att = re.n_swap_attempted.view(n_ladders, R).sum(0).cpu().numpy()
    acc = re.n_swap_accepted.view(n_ladders, R).sum(0).cpu().numpy()
    print('swap rates %s' % re.swap_acceptance_rate.cpu().numpy().round(3))
    assert np.array_equal(att, [n // 2 * n_ladders] * (R - 1) + [0]) and np.all(acc[:R - 1] > 0) and acc[R - 1] == 0
    assert np.all(acc[:R - 1] < att[:R - 1])
    verdict(name, rate(inner), x)
