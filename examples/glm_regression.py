#!/usr/bin/env python3
"""Logistic (or Poisson) regression on synthetic covariates: NUTS, rank diagnostics, PSIS-LOO.

Binary outcomes drawn from a logistic model with an intercept and five standardised
covariates, of which the last two have no effect; a Gaussian prior on the coefficients.  The
likelihood is ``LinearForwardModel`` + ``BinomialLogitErrorModel``: its log-prob and gradient
run in the fused kernels of ``csrc/glm.hip``.  ``warmup(NUTSSampler, ..., dense=True)`` learns
the metric and the steps, the kept draws are summarised with ``rank_summary``, and the full
design is compared with the nested one that drops the two idle covariates by
``loo.compare``.  ``--poisson``: counts with an exposure offset (``PoissonLogErrorModel``).

    python examples/glm_regression.py [--poisson] [--n 400] [--chains 16] [--warmup 200] [--keep 200] [--seed 0]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from binf_amd import diagnostics, loo
from binf_amd.model.glm import BinomialLogitErrorModel, PoissonLogErrorModel
from binf_amd.model.linear import LinearForwardModel
from binf_amd.pdf import IsotropicGaussian
from binf_amd.pdf.likelihoods import Likelihood
from binf_amd.pdf.posteriors import Posterior
from binf_amd.samplers import NUTSSampler
from binf_amd.samplers.rng import DeviceRNG
from binf_amd.samplers.warmup import warmup

TRUTH = np.array([-0.5, 1.2, -0.8, 0.6, 0.0, 0.0])


def fit(design, error_model, args, dev, seed):
    """``(kept draws [T x C x K], likelihood)`` of one design."""
    lik = Likelihood('outcomes', LinearForwardModel('covariates', design), error_model)
    post = Posterior({'outcomes': lik},
                     {'prior': IsotropicGaussian(k=1.0 / 2.5 ** 2, x0=0.0, name='prior',
                                                 variable_name='coefficients')})
    rng = DeviceRNG(seed, dev)
    x0 = 0.1 * rng.normal((args.chains, design.shape[0]), dev)
    s = NUTSSampler(post, x0, 0.1, max_tree_depth=6, target_accept=0.8, variable_name='coefficients', rng=rng)
    warmup(s, args.warmup, dense=True)
    return s.sample_n(args.keep), lik


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--poisson', action='store_true')
    ap.add_argument('--n', type=int, default=400)
    ap.add_argument('--chains', type=int, default=16)
    ap.add_argument('--warmup', type=int, default=200)
    ap.add_argument('--keep', type=int, default=200)
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    rs = np.random.RandomState(args.seed)
    K = len(TRUTH)
    design = np.vstack([np.ones(args.n), rs.standard_normal((K - 1, args.n))])
    eta = TRUTH.dot(design)
    if args.poisson:
        exposure = rs.uniform(0.5, 4.0, size=args.n)
        ys = rs.poisson(exposure * np.exp(eta)).astype(np.float64)
        make = lambda: PoissonLogErrorModel(ys, offset=np.log(exposure))
    else:
        ys = (rs.uniform(size=args.n) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
        make = lambda: BinomialLogitErrorModel(ys)
    names = ['intercept'] + ['x%d' % i for i in range(1, K)]

    full, lik_full = fit(design, make(), args, dev, args.seed)
    print('%s regression, %d observations, %d chains: all %d covariates (truth %s)'
          % ('Poisson' if args.poisson else 'logistic', args.n, args.chains, K - 1, TRUTH.tolist()))
    print(diagnostics.rank_summary(full).table(names))

    nested, lik_nested = fit(design[:K - 2], make(), args, dev, args.seed + 1)
    print('\nwithout the last two covariates')
    print(diagnostics.rank_summary(nested).table(names[:K - 2]))

    a = loo.loo(loo.pointwise_log_likelihood(lik_full, full.reshape(-1, K)))
    b = loo.loo(loo.pointwise_log_likelihood(lik_nested, nested.reshape(-1, K - 2)))
    print('\nPSIS-LOO   full: elpd %.2f +- %.2f, p_loo %.2f, khat > 0.7: %d' % (a.elpd, a.se, a.p_loo, a.n_bad))
    print('PSIS-LOO nested: elpd %.2f +- %.2f, p_loo %.2f, khat > 0.7: %d' % (b.elpd, b.se, b.p_loo, b.n_bad))
    diff, se = loo.compare(a, b)
    print('elpd(full) - elpd(nested) = %.2f +- %.2f' % (diff, se))


if __name__ == '__main__':
    main()
