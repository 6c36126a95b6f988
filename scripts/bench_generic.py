"""Per-step (generic) tier on a user-style PDF written with torch ops, at C2's
shape: what a plug-in posterior without a fused kernel costs (development aid)."""
import json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from binf_amd import _native
from binf_amd.samplers.hmc import HMCSampler
from binf_amd.samplers.rng import DeviceRNG
dev = torch.device('cuda:0')


class TorchGaussian(object):
    def __init__(self, k, x0):
        self.k, self.x0 = k, x0

    def log_prob(self, x):
        return (-0.5 * self.k) * _native.row_sum(x, _native.ROW_SUMSQ_SHIFT, shift=self.x0)

    def gradient(self, x):
        return self.k * (x - self.x0)


out = {}
for C, D, L, graph in ((4096, 1024, 20, False), (256, 768, 20, False), (256, 768, 20, True),
                       (2048, 64, 10, False), (2048, 64, 10, True), (64, 20000, 10, False)):
    q0 = torch.randn((C, D), dtype=torch.float64, device=dev)
    s = HMCSampler(TorchGaussian(1.0, 0.0), q0, 0.05, L, variable_name='x', rng=DeviceRNG(0, dev), graph=graph)
    for _ in range(3): s.sample()
    torch.cuda.synchronize(); t = time.perf_counter()
    K = 10
    for _ in range(K): s.sample()
    torch.cuda.synchronize(); dt = (time.perf_counter() - t) / K
    bytes_step = 32.0 * D * C          # unfused kick + drift traffic per leapfrog step
    out['%dx%d L=%d%s' % (C, D, L, ' graph' if graph else '')] = {'ms_per_sample': dt * 1e3, 'us_per_leapfrog_step': dt / L * 1e6,
                                     'chain_steps_per_s': C * L / dt,
                                     'kick_drift_GBps_if_alone': bytes_step * L / dt / 1e9}

# The Likelihood plug-in surface with a user's forward model (no fused kernel of its own):
# forward pass and error-model gradient are the user's / the example's classes, the chain rule
# is binf_jacobian_contract_f64, the Posterior's sums binf_sum_terms_f64 (likelihoods.py:141-155)
from binf_amd.example.likelihood import POLYVAL, ForwardModel, GaussianErrorModel
from binf_amd.example.priors import GammaPrior, GaussianPrior
from binf_amd.pdf.likelihoods import Likelihood
from binf_amd.pdf.posteriors import Posterior


class PlainPolynomial(ForwardModel):
    def _evaluate(self, coefficients):           # an override: no fused kernel may be assumed
        return ForwardModel._evaluate(self, coefficients)


for C, K, N, L, graph in ((4096, 8, 512, 20, False), (4096, 8, 512, 20, True), (8192, 33, 16384, 20, False)):
    rs = np.random.RandomState(0)
    xs = np.linspace(-1, 1, N)
    ys = POLYVAL(xs, rs.standard_normal(K)) + rs.standard_normal(N) / np.sqrt(2.5)
    lik = Likelihood('points', PlainPolynomial(xs, POLYVAL), GaussianErrorModel(ys))
    post = Posterior({lik.name: lik}, {'precision_prior': GammaPrior(1.0, 0.2),
                                       'coefficients_prior': GaussianPrior(np.zeros(K), np.ones(K) * 5)})
    cond = post.conditional_factory(precision=torch.full((C,), 2.5, dtype=torch.float64, device=dev))
    assert cond.native_hmc_spec('coefficients') is None
    q0 = torch.from_numpy(rs.standard_normal((C, K)) * 0.1).to(dev)
    s = HMCSampler(cond, q0, 1e-4, L, variable_name='coefficients', rng=DeviceRNG(0, dev, fused=False), graph=graph)
    for _ in range(3): s.sample()
    torch.cuda.synchronize(); t = time.perf_counter()
    R = 10 if N < 10000 else 4
    for _ in range(R): s.sample()
    torch.cuda.synchronize(); dt = (time.perf_counter() - t) / R
    out['plug-in model %d chains, K=%d, N=%d, L=%d%s' % (C, K, N, L, ' graph' if graph else '')] = {
        'ms_per_sample': dt * 1e3, 'us_per_leapfrog_step': dt / L * 1e6, 'chain_steps_per_s': C * L / dt}

# The linear kind (binf_amd/model/linear.py): the same three shapes with a user's model that
# is a LinearForwardModel subclass -- its design matrix is all it supplies -- next to the
# registered polynomial kind at the same shapes, and the two log-prob passes alone
from binf_amd.model.linear import LinearForwardModel


class PowerBasis(LinearForwardModel):
    def __init__(self, xs, K):
        super(PowerBasis, self).__init__('power_basis', np.vstack([xs ** i for i in range(K)]))


def _time(fn, reps):
    for _ in range(3): fn()
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(reps): fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


for C, K, N, L, graph in ((4096, 8, 512, 20, False), (4096, 8, 512, 20, True), (8192, 33, 16384, 20, False)):
    rs = np.random.RandomState(0)
    xs = np.linspace(-1, 1, N)
    ys = POLYVAL(xs, rs.standard_normal(K)) + rs.standard_normal(N) / np.sqrt(2.5)
    for label, fwm in (('linear kind', PowerBasis(xs, K)), ('polynomial kind', ForwardModel(xs, POLYVAL))):
        lik = Likelihood('points', fwm, GaussianErrorModel(ys))
        assert lik._native_pair() is not None
        post = Posterior({lik.name: lik}, {'precision_prior': GammaPrior(1.0, 0.2),
                                           'coefficients_prior': GaussianPrior(np.zeros(K), np.ones(K) * 5)})
        cond = post.conditional_factory(precision=torch.full((C,), 2.5, dtype=torch.float64, device=dev))
        q0 = torch.from_numpy(rs.standard_normal((C, K)) * 0.1).to(dev)
        s = HMCSampler(cond, q0, 1e-4, L, variable_name='coefficients', rng=DeviceRNG(0, dev, fused=False), graph=graph)
        s.fused_transition = False              # the per-step tier for both (the polynomial kind's
                                                # whole-transition kernel is another feature)
        dt = _time(s.sample, 10 if N < 10000 else 4)
        out['%s %d chains, K=%d, N=%d, L=%d%s' % (label, C, K, N, L, ' graph' if graph else '')] = {
            'ms_per_sample': dt * 1e3, 'us_per_leapfrog_step': dt / L * 1e6, 'chain_steps_per_s': C * L / dt}
    if N > 10000:
        th = torch.from_numpy(rs.standard_normal((C, K)) * 0.1).to(dev)
        A = PowerBasis(xs, K).design_matrix(K, dev)
        xd, yd = torch.from_numpy(xs).to(dev), torch.from_numpy(ys).to(dev)
        t_lin = _time(lambda: _native.linear_gauss_logp(th, A, yd, 2.5), 20)
        t_pol = _time(lambda: _native.poly_gauss_logp(th, xd, yd, 2.5), 20)
        t_fwd = _time(lambda: _native.linear_forward(th, A), 20)
        floor = 2.0 * K * N * C / 70.8e12       # sustained FP64-MFMA rate
        out['log-prob pass %d chains, K=%d, N=%d' % (C, K, N)] = {
            'linear_gauss_logp_ms': t_lin * 1e3, 'poly_gauss_logp_horner_ms': t_pol * 1e3,
            'linear_forward_ms': t_fwd * 1e3, 'mfma_floor_ms': floor * 1e3,
            'linear_TFLOPs': 2.0 * K * N * C / t_lin / 1e12}

# The chain-resident kernels (LinearForwardModel(..., resident=True), kind 'linear_resident'):
# whole transitions and whole Gibbs sweeps through sample_n, one launch for n, next to the
# same model's per-step path and the polynomial kind's resident kernel on the same power basis
# (scripts/probe_linear_resident.py measures the crossover that sets RESIDENT_MAX_WORK)
import probe_linear_resident as _probe

for C, K, N, L in ((4096, 8, 512, 20), (1024, 9, 200, 30), (4096, 9, 200, 30)):
    out['resident linear %d chains, K=%d, N=%d, L=%d' % (C, K, N, L)] = _probe.measure(C, K, N, L, dev, 3, 0.2)
print(json.dumps(out))
