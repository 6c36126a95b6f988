"""Device tests of the layers above the negative-binomial kernels: ``RWMCSampler(variable=...)``
(the default unchanged; a per-chain Metropolis move on ``log_dispersion`` held to a host quadrature
of its one-dimensional conditional), and the whole wiring -- a Gibbs run of NUTS on the coefficients
and Metropolis on lam against a long host-side reference run, its PSIS-LOO record and the comparison
with the Poisson fit of the same data."""
import math

import numpy as np
import pytest
import torch

import negbin_ref as NR
from binf_amd import diagnostics, loo
from binf_amd.example.samplers import RWMCSampler
from binf_amd.model.glm import NegBinomialLogErrorModel, PoissonLogErrorModel
from binf_amd.model.linear import LinearForwardModel
from binf_amd.pdf import IsotropicGaussian
from binf_amd.pdf.likelihoods import Likelihood
from binf_amd.pdf.posteriors import Posterior
from binf_amd.samplers import BinfState, NUTSSampler
from binf_amd.samplers.gibbs import GibbsSampler
from binf_amd.samplers.rng import DeviceRNG

pytestmark = pytest.mark.gpu


def up(x, device):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(device)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int64)


def _nb_counts(rs, mu, phi):
    return rs.negative_binomial(phi, phi / (phi + mu)).astype(np.float64)


def _posterior(A, ys, off, prior_theta, prior_lam):
    lik = Likelihood('outcomes', LinearForwardModel('covariates', A), NegBinomialLogErrorModel(ys, off))
    priors = {}
    if prior_theta:
        priors['prior'] = IsotropicGaussian(prior_theta[0], prior_theta[1], name='prior', variable_name='coefficients')
    if prior_lam:
        priors['lam_prior'] = IsotropicGaussian(prior_lam[0], prior_lam[1], name='lam_prior',
                                                variable_name='log_dispersion')
    return Posterior({'outcomes': lik}, priors)


# ---------------------------------------------------------------------------
# the default is the sampler it was
# ---------------------------------------------------------------------------
def test_rwmc_default_reproduces_an_unchanged_run(device):
    """``RWMCSampler(pdf, state, stepsize)`` on the host stream and the same with
    ``variable='coefficients'`` spelled out: the same states, bit for bit; the same on a DeviceRNG."""
    C, K = 9, 3
    rs = np.random.RandomState(1)
    pdf = IsotropicGaussian(k=2.0, x0=0.5, name='g', variable_name='coefficients')
    x0 = up(rs.standard_normal((C, K)), device)
    runs = []
    for kw in ({}, {'variable': 'coefficients'}):
        np.random.seed(77)
        s = RWMCSampler(pdf, x0.clone(), 0.4, **kw)
        runs.append([s.sample().clone() for _ in range(6)])
        assert list(s.last_draw_stats) == ['coefficients']
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(*runs))
    assert not torch.equal(runs[0][-1], x0)
    dev_runs = []
    for kw in ({}, {'variable': 'coefficients'}):
        s = RWMCSampler(pdf, x0.clone(), 0.4, rng=DeviceRNG(5, device), **kw)
        dev_runs.append([s.sample().clone() for _ in range(6)])
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(*dev_runs))


# ---------------------------------------------------------------------------
# stationarity of lam
# ---------------------------------------------------------------------------
N_OBS, CHAINS, N_WARM, N_KEEP, SEED = 24, 512, 150, 200, 20251
THETA, PRIOR_LAM = math.log(3.0), (1.0, 0.5)


def _lam_data():
    rs = np.random.RandomState(SEED)
    return _nb_counts(rs, np.full(N_OBS, 3.0), 2.0)


def _conditional_log_density(lam, ys, count_term=True):
    """log p(lam | theta, y) up to a constant on a grid ``lam`` [G], in numpy float64: the term at
    z = theta - lam, the count term by tail counts, the Gaussian prior."""
    phi = np.exp(lam)[:, None]
    z = THETA - lam[:, None]
    sp = np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))
    out = np.sum(ys[None, :] * z - (ys[None, :] + phi) * sp, axis=1)
    if count_term:
        tail = NR.tail_counts(ys).astype(np.float64)
        j = np.arange(tail.shape[0], dtype=np.float64)
        out = out + np.sum(tail[None, :] * np.log(phi + j[None, :]), axis=1)
    return out - 0.5 * PRIOR_LAM[0] * (lam - PRIOR_LAM[1]) ** 2


def _quadrature(ys):
    """Mean and variance of the conditional by the trapezoid rule on 40001 points over [-12, 13]
    (the prior alone puts 1e-30 beyond): the integrand is smooth and the step 6e-4, the rule's
    error is far below the Monte-Carlo errors it is compared with."""
    trapezoid = getattr(np, 'trapezoid', None) or np.trapz
    lam = np.linspace(-12.0, 13.0, 40001)
    lp = _conditional_log_density(lam, ys)
    w = np.exp(lp - lp.max())
    Z = trapezoid(w, lam)
    mean = trapezoid(w * lam, lam) / Z
    return float(mean), float(trapezoid(w * (lam - mean) ** 2, lam) / Z)


class _HostLamPDF(object):
    """The same conditional as a user's torch PDF, with or without the count term."""

    def __init__(self, ys, count_term):
        self.ys, self.count_term = ys, count_term
        tail = NR.tail_counts(ys.cpu().numpy())
        self.tail = torch.from_numpy(tail.astype(np.float64)).to(ys.device)
        self.j = torch.arange(tail.shape[0], dtype=torch.float64, device=ys.device)

    def log_prob(self, log_dispersion):
        lam = log_dispersion.reshape(-1, 1)
        phi, z = torch.exp(lam), THETA - lam
        out = (self.ys * z - (self.ys + phi) * torch.nn.functional.softplus(z)).sum(dim=1)
        if self.count_term:
            out = out + (self.tail * torch.log(phi + self.j)).sum(dim=1)
        return out - 0.5 * PRIOR_LAM[0] * (lam[:, 0] - PRIOR_LAM[1]) ** 2


def _lam_stationarity(device, pdf=None):
    ys = _lam_data()
    mean, var = _quadrature(ys)
    sd = math.sqrt(var)
    rs = np.random.RandomState(SEED + 1)
    lam0 = up(mean + sd * (1.0 + rs.standard_normal((CHAINS, 1))), device)     # started one sd off
    if pdf is None:
        post = _posterior(np.ones((1, N_OBS)), ys, None, None, PRIOR_LAM)
        pdf = post.conditional_factory(coefficients=torch.full((CHAINS, 1), THETA, dtype=torch.float64, device=device))
        assert set(pdf.variables) == {'log_dispersion'}
    s = RWMCSampler(pdf, lam0, 2.4 * sd, rng=DeviceRNG(SEED, device), variable='log_dispersion')
    for _ in range(N_WARM):
        s.sample()
    kept = torch.stack([s.sample().clone() for _ in range(N_KEEP)])
    centred = kept - kept.mean()
    d = diagnostics.summary(torch.cat((kept, centred * centred), dim=2).contiguous()).cpu()
    fig = dict(mean=float(d.mean[0]), want_mean=mean, mcse=float(d.mcse[0]), var=float(d.mean[1]), want_var=var,
               var_se=float(d.mcse[1]), rhat=float(d.rhat[0]), accept=float(s.acceptance_rate.mean()))
    ok = abs(fig['mean'] - mean) <= 5 * fig['mcse'] and abs(fig['var'] - var) <= 5 * fig['var_se'] and \
        all(math.isfinite(v) for v in fig.values())
    return ok, fig


def test_stationarity_of_lam(device):
    """Intercept-only, theta fixed, a Gaussian prior on lam; 512 chains, 150 + 200 moves of
    ``RWMCSampler(variable='log_dispersion')``: the mean within 5 MCSE and the pooled variance
    within 5 of its standard errors of the quadrature."""
    ok, fig = _lam_stationarity(device)
    print('lam', fig)
    assert ok, fig
    assert 0.1 < fig['accept'] < 0.9


def test_the_margin_sees_a_dropped_count_term(device):
    """The same check on a host-side torch PDF: passes as written, fails with the count term
    dropped.  No kernel is mutated."""
    y = up(_lam_data(), device)
    ok, fig = _lam_stationarity(device, _HostLamPDF(y, True))
    assert ok, fig
    bad, fig = _lam_stationarity(device, _HostLamPDF(y, False))
    print('dropped', fig)
    assert not bad, fig


# ---------------------------------------------------------------------------
# the whole wiring
# ---------------------------------------------------------------------------
W_N, W_K, W_PHI, W_C, W_SWEEPS, W_BURN = 256, 3, 2.0, 128, 200, 50
W_TRUTH = np.array([0.8, 0.5, -0.4])
W_PRIOR_THETA, W_PRIOR_LAM = (1.0 / 2.5 ** 2, 0.0), (0.25, 0.0)


def _wiring_data():
    rs = np.random.RandomState(11)
    A = np.vstack([np.ones(W_N), rs.standard_normal((W_K - 1, W_N))])
    exposure = rs.uniform(0.5, 4.0, size=W_N)
    ys = _nb_counts(rs, exposure * np.exp(W_TRUTH.dot(A)), W_PHI)
    return A, ys, np.log(exposure)


def _host_reference(A, ys, off, chains=48, steps=3000, burn=500):
    """A long random-walk Metropolis run on (theta, lam) jointly, in numpy on the host, with the
    textbook density (``scipy.special.gammaln``): ``(means [K + 1], mcse [K + 1])`` from the
    per-chain means (independent chains: the standard error of their mean)."""
    from scipy.special import gammaln
    rs = np.random.RandomState(12)

    def lp(x):
        theta, lam = x[:, :W_K], x[:, W_K]
        phi = np.exp(lam)[:, None]
        eta = theta.dot(A) + off[None, :]
        ll = gammaln(ys[None, :] + phi) - gammaln(phi) + phi * lam[:, None] + ys[None, :] * eta - \
            (ys[None, :] + phi) * np.logaddexp(lam[:, None], eta)
        return ll.sum(axis=1) - 0.5 * W_PRIOR_THETA[0] * np.sum((theta - W_PRIOR_THETA[1]) ** 2, axis=1) - \
            0.5 * W_PRIOR_LAM[0] * (lam - W_PRIOR_LAM[1]) ** 2
    x = np.hstack([np.tile(W_TRUTH, (chains, 1)), np.full((chains, 1), math.log(W_PHI))])
    x += 0.05 * rs.standard_normal(x.shape)
    cur = lp(x)
    scale = np.array([0.05, 0.04, 0.04, 0.12])
    total = np.zeros_like(x)
    for t in range(steps):
        prop = x + scale * rs.standard_normal(x.shape)
        new = lp(prop)
        acc = np.log(rs.uniform(size=chains)) < new - cur
        x[acc], cur[acc] = prop[acc], new[acc]
        if t >= burn:
            total += x
    per_chain = total / (steps - burn)
    return per_chain.mean(axis=0), per_chain.std(axis=0, ddof=1) / math.sqrt(chains)


def test_whole_wiring_gibbs_loo_and_compare(device):
    """Simulated data (N = 256, K = 3, phi = 2, an exposure offset): a 200-sweep Gibbs run of NUTS
    on the coefficients and Metropolis on lam (50 sweeps discarded) recovers the intercept and lam
    within 5 standard errors of the difference from a long host-side reference run's means (the
    two runs are independent: sqrt(mcse_device**2 + mcse_host**2)); ``loo`` on its record runs,
    and ``compare`` prefers the negative binomial over the Poisson fit of the same data."""
    A, ys, off = _wiring_data()
    want, want_se = _host_reference(A, ys, off)
    post = _posterior(A, ys, off, W_PRIOR_THETA, W_PRIOR_LAM)
    rng = DeviceRNG(21, device)
    rs = np.random.RandomState(13)
    theta0 = up(W_TRUTH + 0.05 * rs.standard_normal((W_C, W_K)), device)
    lam0 = up(math.log(W_PHI) + 0.1 * rs.standard_normal((W_C, 1)), device)
    state = BinfState({'coefficients': theta0, 'log_dispersion': lam0})
    subs = {'coefficients': NUTSSampler(post.conditional_factory(log_dispersion=lam0), theta0, 0.05,
                                        max_tree_depth=5, variable_name='coefficients', rng=rng),
            'log_dispersion': RWMCSampler(post.conditional_factory(coefficients=theta0), lam0, 0.3, rng=rng,
                                          variable='log_dispersion')}
    gibbs = GibbsSampler(post, state, subs)
    rec = gibbs.sample_n(W_SWEEPS)
    th, lm = rec['coefficients'][W_BURN:], rec['log_dispersion'][W_BURN:]
    assert th.shape == (W_SWEEPS - W_BURN, W_C, W_K) and lm.shape == (W_SWEEPS - W_BURN, W_C, 1)
    d = diagnostics.summary(torch.cat((th[:, :, :1], lm), dim=2).contiguous()).cpu()
    for k, name, ref in ((0, 'intercept', 0), (1, 'lam', W_K)):
        got, mcse = float(d.mean[k]), float(d.mcse[k])
        allow = 5 * math.sqrt(mcse ** 2 + want_se[ref] ** 2)
        print('%s: device %.4f +- %.4f, host %.4f +- %.4f' % (name, got, mcse, want[ref], want_se[ref]))
        assert abs(got - want[ref]) <= allow, (name, got, want[ref], allow)
    assert abs(float(d.mean[1]) - math.log(W_PHI)) < 0.5                 # and lam is near log 2 at all

    # PSIS-LOO on the record, from states and from the pair: the same record
    lik = post.likelihoods['outcomes']
    S = 40
    pair = (th[-S:, 0].contiguous(), lm[-S:, 0, 0].contiguous())
    states = [BinfState({'coefficients': th[-S + i, :1], 'log_dispersion': lm[-S + i, :1]}) for i in range(S)]
    assert torch.equal(bits(loo.pointwise_log_likelihood(lik, states)), bits(loo.pointwise_log_likelihood(lik, pair)))
    flat = (th.reshape(-1, W_K)[::8].contiguous(), lm.reshape(-1)[::8].contiguous())
    nb = loo.loo(loo.pointwise_log_likelihood(lik, flat))
    assert math.isfinite(nb.elpd) and bool(torch.isfinite(nb.khat).all())
    # its sums over the observations are the likelihood's log-prob
    r = loo.pointwise_log_likelihood(lik, pair)
    lp = lik.log_prob(coefficients=pair[0], log_dispersion=pair[1])
    assert torch.allclose(r.sum(dim=1), lp, rtol=1e-12, atol=0.0)

    # the Poisson fit of the same data
    plik = Likelihood('outcomes', LinearForwardModel('covariates', A), PoissonLogErrorModel(ys, off))
    ppost = Posterior({'outcomes': plik}, {'prior': IsotropicGaussian(W_PRIOR_THETA[0], W_PRIOR_THETA[1], name='prior',
                                                                     variable_name='coefficients')})
    ps = NUTSSampler(ppost, theta0.clone(), 0.03, max_tree_depth=5, variable_name='coefficients',
                     rng=DeviceRNG(22, device))
    ps.sample_n(W_BURN, record=False)
    pth = ps.sample_n(W_SWEEPS - W_BURN)
    po = loo.loo(loo.pointwise_log_likelihood(plik, pth.reshape(-1, W_K)[::8].contiguous()))
    diff, se = loo.compare(nb, po)
    print('elpd NB %.1f, Poisson %.1f, difference %.1f +- %.1f; khat > 0.7: NB %d, Poisson %d'
          % (nb.elpd, po.elpd, diff, se, nb.n_bad, po.n_bad))
    assert diff > 0.0 and se > 0.0


# ---------------------------------------------------------------------------
# the other drivers reach the same hooks
# ---------------------------------------------------------------------------
class _Spy(object):
    def __init__(self, monkeypatch, names):
        from binf_amd import _native
        self.calls = []
        for n in names:
            monkeypatch.setattr(_native, n, self._wrap(n, getattr(_native, n)))

    def _wrap(self, name, fn):
        def spy(*a, **k):
            self.calls.append(name)
            return fn(*a, **k)
        return spy


class _TemperedPDF(object):
    """log prior + beta_c log likelihood of a negative-binomial posterior with lam fixed: what
    ``TemperedSMC`` drives.  The likelihood's log-prob and gradient are the library's."""

    def __init__(self, post, beta):
        self.lik, self.prior, self.beta = post.likelihoods['outcomes'], post.priors['prior'], beta

    def log_likelihood(self, x):
        return self.lik.log_prob(coefficients=x)

    def log_prob(self, coefficients):
        return self.prior.log_prob(coefficients=coefficients) + self.beta * self.log_likelihood(coefficients)

    def gradient(self, coefficients):
        return self.prior.gradient(coefficients=coefficients) + \
            self.beta[:, None] * self.lik.gradient(coefficients=coefficients)


def test_chees_replica_smc_and_warmup_take_the_hooks(device, monkeypatch):
    """``ChEESSampler``, ``ReplicaExchangeSampler`` (a ladder of per-slot lam), ``TemperedSMC`` and
    ``warmup`` around samplers on a negative-binomial posterior with lam fixed: every one reaches the
    family's kernels (never the other families'), and the draws stay finite."""
    from binf_amd.samplers.chees import ChEESSampler
    from binf_amd.samplers.hmc import HMCSampler
    from binf_amd.samplers.replica import ReplicaExchangeSampler
    from binf_amd.samplers.smc import TemperedSMC
    from binf_amd.samplers.warmup import warmup
    K, N, C, R = 3, 40, 32, 4
    rs = np.random.RandomState(3)
    A = np.vstack([np.ones(N), rs.standard_normal((K - 1, N))])
    ys = _nb_counts(rs, np.exp(np.array([0.8, 0.5, -0.4]).dot(A)), 2.0)
    q0 = up(0.1 * rs.standard_normal((C, K)), device)
    lam = up(np.tile(np.log([2.0, 1.0, 0.5, 0.25]), C // R), device)          # slot r of every ladder

    def post():
        p = _posterior(A, ys, None, (0.16, 0.0), None)
        return p.conditional_factory(log_dispersion=lam)
    ours = ('linear_negbin_leapfrog', 'linear_negbin_grad', 'linear_negbin_logp', 'negbin_pointwise')
    spy = _Spy(monkeypatch, ours + ('linear_glm_leapfrog', 'linear_glm_grad', 'linear_glm_logp', 'glm_pointwise'))

    def taken(*names):
        """Only this family's kernels, its force among them (fused leapfrog or gradient), and
        every one of ``names``."""
        calls = set(spy.calls)
        del spy.calls[:]
        assert calls <= set(ours) and all(n in calls for n in names), calls
        assert 'linear_negbin_leapfrog' in calls or 'linear_negbin_grad' in calls, calls

    s = ChEESSampler(post(), q0.clone(), 0.05, max_leapfrog_steps=16, timestep_adaption_limit=6,
                     variable_name='coefficients', rng=DeviceRNG(1, device))
    out = s.sample_n(8)
    assert bool(torch.isfinite(out).all())
    taken('negbin_pointwise')

    inner = HMCSampler(post(), q0.clone(), 0.05, 4, variable_name='coefficients', rng=DeviceRNG(2, device))
    rex = ReplicaExchangeSampler(inner, R)
    out = rex.sample_n(6)
    assert bool(torch.isfinite(out).all()) and int(rex.n_swap_attempted.sum()) > 0
    taken('linear_negbin_leapfrog', 'negbin_pointwise')

    w = HMCSampler(post(), q0.clone(), 0.05, 4, variable_name='coefficients', rng=DeviceRNG(3, device))
    warmup(w, 40, init_buffer=5, term_buffer=5, base_window=10)
    assert bool(torch.isfinite(w.state).all())
    taken('negbin_pointwise')

    beta = torch.zeros(C, dtype=torch.float64, device=device)
    pdf = _TemperedPDF(_posterior(A, ys, None, (0.16, 0.0), None).conditional_factory(log_dispersion=lam), beta)
    mut = HMCSampler(pdf, q0.clone(), 0.05, 4, variable_name='coefficients', rng=DeviceRNG(4, device))
    smc = TemperedSMC(mut, beta, n_populations=2, n_mutations=2, log_likelihood=pdf.log_likelihood)
    res = smc.run()
    assert bool((smc.beta_population == 1.0).all()) and bool(torch.isfinite(res.log_evidence).all())
    taken('linear_negbin_grad', 'negbin_pointwise')
