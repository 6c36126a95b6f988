"""The windowed warm-up end to end on the device, deterministic (``DeviceRNG(seed)``): the
8-dimensional Gaussian with sigma from 1 to 100 as a user's torch PDF, 16 chains started at
3 sigma z, nsteps = 5, timestep = 0.5, rates 1.02 / 0.9 (acceptance target 0.84),
``WindowedWarmup(n_warmup=300, init_buffer=20, term_buffer=40, base_window=20)``, 200 kept
draws -- and the same run without the metric.

The thresholds are those ``tests/test_metric.py`` holds the numpy restatement to over ten
seeds (there: scale / sigma 0.89 ... 1.08, max split-R^ <= 1.08 with the metric, >= 3.38
without)."""
import numpy as np
import pytest
import torch

import metric_ref as MR
from binf_amd import diagnostics
from binf_amd.samplers.hmc import HMCSampler
from binf_amd.samplers.rng import DeviceRNG
from binf_amd.samplers.warmup import WindowedWarmup

pytestmark = pytest.mark.gpu


class DiagGauss(object):
    """log p(x) = -1/2 sum (x / sigma)^2, a torch PDF."""

    def __init__(self, sigma):
        self.sigma = sigma

    def log_prob(self, x):
        z = x / self.sigma
        return -0.5 * (z * z).sum(dim=1)

    def gradient(self, x):
        return x / (self.sigma * self.sigma)


def run(device, with_metric, seed=2025, C=16, n_warmup=300, n_keep=200):
    sigma = torch.from_numpy(MR.SIGMA8).to(device)
    rng = DeviceRNG(seed, device)
    x0 = 3.0 * sigma * rng.normal((C, sigma.numel()), device)
    s = HMCSampler(DiagGauss(sigma), x0, 0.5, 5, adaption_uprate=1.02, adaption_downrate=0.9,
                   variable_name='x', rng=rng)
    if with_metric:
        w = WindowedWarmup(s, n_warmup, init_buffer=20, term_buffer=40, base_window=20)
        assert w.windows == [(20, 40), (40, 80), (80, 260)]
        w.run()
    else:
        s.timestep_adaption_limit = n_warmup + 1
        for _ in range(n_warmup):
            s.sample()
    assert s.counter == n_warmup
    kept = s.sample_n(n_keep)
    return s, kept, diagnostics.summary(kept)


def test_the_learnt_metric_makes_the_anisotropic_gaussian_mix(device):
    sigma = MR.SIGMA8
    s1, kept1, sum1 = run(device, True)
    s0, kept0, sum0 = run(device, False)
    ratio = s1.metric_scale.cpu().numpy()[0] / sigma
    rhat1, rhat0 = sum1.rhat.cpu().numpy(), sum0.rhat.cpu().numpy()
    ess1, ess0 = sum1.ess.cpu().numpy(), sum0.ess.cpu().numpy()
    print('scale / sigma:', np.round(ratio, 3))
    print('split-R^ with the metric:', np.round(rhat1, 4), ' without:', np.round(rhat0, 3))
    print('ESS of the widest dimension: %.0f with, %.1f without (x %.1f); acceptance %.2f / %.2f'
          % (ess1[-1], ess0[-1], ess1[-1] / ess0[-1], float(s1.acceptance_rate.mean()),
             float(s0.acceptance_rate.mean())))
    assert s0.metric_scale is None and tuple(s1.metric_scale.shape) == (1, 8)
    assert np.all(ratio >= 0.7) and np.all(ratio <= 1.4)
    assert rhat1.max() < 1.2
    assert rhat0.max() > 2.0
