#!/usr/bin/env python3
"""A diagonal HMC metric learnt during warm-up, and what it buys.

Default: an 8-dimensional Gaussian with standard deviations from 1 to 100, written as a
user's torch PDF.  16 chains start at 3 sigma z and run 300 adapting transitions with
nsteps = 5, then 200 kept ones -- once with the identity mass (the narrowest dimension
limits the step, the widest crawls) and once with ``warmup()`` learning a per-dimension
scale in the same 300 transitions.  ``summary()`` of both records is printed.

``--linear``: a Fourier regression whose basis columns carry amplitudes 1 ... 100 (the
coefficients' posterior widths then span 1 ... 1/100), the HMC subsampler of the Gibbs scheme
warmed up with ``advance=gibbs.sample``.

``--dense``: the same Gaussian ROTATED by a fixed random orthogonal matrix -- marginal widths
nearly alike, the condition number where it was.  Three rows: the identity mass, the diagonal
metric (which finds nothing to learn) and ``warmup(..., dense=True)`` learning the Cholesky
factor of the covariance; per row the largest split-R^ and the eigenvalues of the learnt
M^-1 whitened by the true covariance (all 1 when the metric is the truth).

    python examples/adapted_metric.py [--linear | --dense] [--chains 16] [--seed 0]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from binf_amd import diagnostics
from binf_amd.samplers.hmc import HMCSampler
from binf_amd.samplers.rng import DeviceRNG
from binf_amd.samplers.warmup import warmup


class DiagGauss(object):
    """log p(x) = -1/2 sum (x / sigma)^2."""

    def __init__(self, sigma):
        self.sigma = sigma

    def log_prob(self, x):
        z = x / self.sigma
        return -0.5 * (z * z).sum(dim=1)

    def gradient(self, x):
        return x / (self.sigma * self.sigma)


def gaussian(args, dev):
    sigma = torch.tensor(100.0 ** (np.arange(8) / 7.0), dtype=torch.float64, device=dev)
    names = ['sigma=%.3g' % s for s in sigma.cpu().numpy()]
    for with_metric in (False, True):
        rng = DeviceRNG(args.seed, dev)
        x0 = 3.0 * sigma * rng.normal((args.chains, 8), dev)
        s = HMCSampler(DiagGauss(sigma), x0, 0.5, 5, adaption_uprate=1.02, adaption_downrate=0.9,
                       variable_name='x', rng=rng)
        if with_metric:
            warmup(s, args.warmup, init_buffer=20, term_buffer=40, base_window=20)
        else:
            s.timestep_adaption_limit = args.warmup + 1
            for _ in range(args.warmup):
                s.sample()
        kept = s.sample_n(args.keep)
        print('\n== %s: acceptance %.2f, mean step %.3g'
              % ('metric learnt in the warm-up' if with_metric else 'identity mass',
                 float(s.acceptance_rate.mean()), float(s.timestep.mean())))
        if with_metric:
            print('   scale / sigma:', np.round((s.metric_scale[0] / sigma).cpu().numpy(), 3))
        print(diagnostics.summary(kept).table(names))


class RotatedGauss(object):
    """log p(x) = -1/2 x^T P x."""

    def __init__(self, precision):
        self.P = precision

    def log_prob(self, x):
        return -0.5 * (x * (x @ self.P)).sum(dim=1)

    def gradient(self, x):
        return x @ self.P


def dense(args, dev):
    sigma = 100.0 ** (np.arange(8) / 7.0)
    Q, _ = np.linalg.qr(np.random.RandomState(1000).standard_normal((8, 8)))
    true_chol = np.linalg.cholesky((Q * sigma ** 2) @ Q.T)
    P = torch.from_numpy((Q / sigma ** 2) @ Q.T).to(dev)
    Lt = torch.from_numpy(true_chol).to(dev)
    print('%-9s %13s  %s' % ('metric', 'max split-R^', 'eigenvalues of the learnt M^-1, whitened by the true covariance'))
    for kind in ('none', 'diagonal', 'dense'):
        rng = DeviceRNG(args.seed, dev)
        x0 = 3.0 * rng.normal((args.chains, 8), dev) @ Lt.T
        s = HMCSampler(RotatedGauss(P), x0, 0.5, 5, adaption_uprate=1.02, adaption_downrate=0.9,
                       variable_name='x', rng=rng)
        if kind == 'none':
            s.timestep_adaption_limit = args.warmup + 1
            for _ in range(args.warmup):
                s.sample()
            learnt = None
        else:
            warmup(s, args.warmup, init_buffer=20, term_buffer=40, base_window=20, dense=kind == 'dense')
            learnt = s.metric_chol[0].cpu().numpy() if kind == 'dense' else np.diag(s.metric_scale[0].cpu().numpy())
        rhat = float(diagnostics.summary(s.sample_n(args.keep)).rhat.max())
        if learnt is None:
            print('%-9s %13.3f  -' % (kind, rhat))
        else:
            M = np.linalg.solve(true_chol, learnt)
            ev = np.linalg.eigvalsh(M @ M.T)
            print('%-9s %13.3f  %.3g ... %.3g' % (kind, rhat, ev.min(), ev.max()))


def linear(args, dev):
    from binf_amd.example.priors import GammaPrior, GaussianPrior
    from binf_amd.example.likelihood import GaussianErrorModel
    from binf_amd.example.samplers import make_hmc_sampler
    from binf_amd.model.linear import LinearForwardModel
    from binf_amd.pdf.likelihoods import Likelihood
    from binf_amd.pdf.posteriors import Posterior
    from binf_amd.samplers import BinfState
    K, N = 8, 200
    rs = np.random.RandomState(args.seed)
    t = np.linspace(0.0, 1.0, N)
    amp = 100.0 ** (np.arange(K) / (K - 1.0))
    design = np.stack([amp[k] * (np.cos if k % 2 == 0 else np.sin)(np.pi * (k + 1) * t) for k in range(K)])
    truth = rs.standard_normal(K) / amp
    ys = truth @ design + rs.standard_normal(N) / np.sqrt(4.0)
    for with_metric in (False, True):
        # the likelihood must be called 'points' and the variable 'coefficients' for the
        # example's GammaSampler (binf_amd/example/samplers.py)
        L = Likelihood('points', LinearForwardModel('fourier', design), GaussianErrorModel(ys))
        post = Posterior({L.name: L}, {'precision_prior': GammaPrior(1.0, 0.2),
                                       'coefficients_prior': GaussianPrior(np.zeros(K), np.full(K, 5.0))})
        start = BinfState(dict(coefficients=torch.zeros((args.chains, K), dtype=torch.float64, device=dev),
                               precision=torch.ones(args.chains, dtype=torch.float64, device=dev)))
        gips = make_hmc_sampler(post, 1e-3, 10, start, rng=DeviceRNG(args.seed, dev),
                                adaption_uprate=1.02, adaption_downrate=0.9)
        hmc = gips.subsamplers['coefficients']
        if with_metric:
            warmup(hmc, args.warmup, advance=gips.sample)
        else:
            hmc.timestep_adaption_limit = args.warmup + 1
            gips.sample_n(args.warmup, record=False)
        kept = gips.sample_n(args.keep)['coefficients']
        print('\n== %s: acceptance %.2f' % ('metric learnt in the warm-up' if with_metric else 'identity mass',
                                            float(hmc.acceptance_rate.mean())))
        if with_metric:
            print('   scale x amplitude:', np.round((hmc.metric_scale[0].cpu().numpy() * amp), 3))
        print(diagnostics.summary(kept).table(['amp=%.3g' % a for a in amp]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--linear', action='store_true')
    ap.add_argument('--dense', action='store_true')
    ap.add_argument('--chains', type=int, default=16)
    ap.add_argument('--warmup', type=int, default=300)
    ap.add_argument('--keep', type=int, default=200)
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    (linear if args.linear else dense if args.dense else gaussian)(args, dev)


if __name__ == '__main__':
    main()
