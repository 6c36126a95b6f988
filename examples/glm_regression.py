#!/usr/bin/env python3
"""Logistic (or Poisson) regression on synthetic covariates: NUTS, rank diagnostics, PSIS-LOO.

Binary outcomes drawn from a logistic model with an intercept and five standardised
covariates, of which the last two have no effect; a Gaussian prior on the coefficients.  The
likelihood is ``LinearForwardModel`` + ``BinomialLogitErrorModel``: its log-prob and gradient
run in the fused kernels of ``csrc/glm.hip``.  ``warmup(NUTSSampler, ..., dense=True)`` learns
the metric and the steps, the kept draws are summarised with ``rank_summary``, and the full
design is compared with the nested one that drops the two idle covariates by
``loo.compare``.  ``--poisson``: counts with an exposure offset (``PoissonLogErrorModel``).
``--negbin``: overdispersed counts (phi = 2) with ``NegBinomialLogErrorModel`` -- a Gibbs loop of
NUTS on the coefficients and Metropolis on the log dispersion, the posterior of phi, and
``loo.compare`` against the Poisson fit of the same data.

    python examples/glm_regression.py [--poisson | --negbin] [--n 400] [--chains 16] [--warmup 200] [--keep 200] [--seed 0]
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


def negbin(args, dev):
    """Overdispersed counts (phi = 2, an exposure offset): a Gibbs loop of NUTS on the coefficients
    and Metropolis on lam = log(phi), the posterior of phi, and PSIS-LOO against the Poisson fit of
    the same data."""
    import math
    from binf_amd.example.samplers import RWMCSampler
    from binf_amd.model.glm import NegBinomialLogErrorModel
    from binf_amd.samplers import BinfState
    from binf_amd.samplers.gibbs import GibbsSampler
    rs = np.random.RandomState(args.seed)
    K, phi = 4, 2.0
    truth = TRUTH[:K]
    design = np.vstack([np.ones(args.n), rs.standard_normal((K - 1, args.n))])
    exposure = rs.uniform(0.5, 4.0, size=args.n)
    mu = exposure * np.exp(truth.dot(design))
    ys = rs.negative_binomial(phi, phi / (phi + mu)).astype(np.float64)
    names = ['intercept'] + ['x%d' % i for i in range(1, K)]
    prior = lambda: IsotropicGaussian(k=1.0 / 2.5 ** 2, x0=0.0, name='prior', variable_name='coefficients')

    lik = Likelihood('outcomes', LinearForwardModel('covariates', design),
                     NegBinomialLogErrorModel(ys, offset=np.log(exposure)))
    post = Posterior({'outcomes': lik},
                     {'prior': prior(),
                      'lam_prior': IsotropicGaussian(k=0.25, x0=0.0, name='lam_prior', variable_name='log_dispersion')})
    rng = DeviceRNG(args.seed, dev)
    theta0 = 0.1 * rng.normal((args.chains, K), dev)
    lam0 = 0.1 * rng.normal((args.chains, 1), dev)
    subs = {'coefficients': NUTSSampler(post.conditional_factory(log_dispersion=lam0), theta0, 0.05,
                                        max_tree_depth=6, target_accept=0.8, variable_name='coefficients', rng=rng),
            'log_dispersion': RWMCSampler(post.conditional_factory(coefficients=theta0), lam0, 0.3, rng=rng,
                                          variable='log_dispersion')}
    gibbs = GibbsSampler(post, BinfState({'coefficients': theta0, 'log_dispersion': lam0}), subs)
    gibbs.sample_n(args.warmup, record=False)
    rec = gibbs.sample_n(args.keep)
    theta, lam = rec['coefficients'], rec['log_dispersion']
    print('negative-binomial regression, %d observations, %d chains (truth %s, phi = %g)'
          % (args.n, args.chains, truth.tolist(), phi))
    print(diagnostics.rank_summary(torch.cat((theta, lam), dim=2).contiguous()).table(names + ['log phi']))
    ph = torch.exp(lam).reshape(-1)
    q = torch.quantile(ph, torch.tensor([0.05, 0.5, 0.95], dtype=ph.dtype, device=ph.device)).tolist()
    print('posterior of phi: mean %.3f, 5 %% %.3f, median %.3f, 95 %% %.3f (truth %g, log phi = %.3f)'
          % (float(ph.mean()), q[0], q[1], q[2], phi, math.log(phi)))

    pois, plik = fit(design, PoissonLogErrorModel(ys, offset=np.log(exposure)), args, dev, args.seed + 1)
    a = loo.loo(loo.pointwise_log_likelihood(lik, (theta.reshape(-1, K).contiguous(), lam.reshape(-1).contiguous())))
    b = loo.loo(loo.pointwise_log_likelihood(plik, pois.reshape(-1, K)))
    print('\nPSIS-LOO negative binomial: elpd %.2f +- %.2f, p_loo %.2f, khat > 0.7: %d, largest khat %.2f'
          % (a.elpd, a.se, a.p_loo, a.n_bad, float(a.khat.max())))
    print('PSIS-LOO            Poisson: elpd %.2f +- %.2f, p_loo %.2f, khat > 0.7: %d, largest khat %.2f'
          % (b.elpd, b.se, b.p_loo, b.n_bad, float(b.khat.max())))
    diff, se = loo.compare(a, b)
    print('elpd(negative binomial) - elpd(Poisson) = %.2f +- %.2f' % (diff, se))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--poisson', action='store_true')
    ap.add_argument('--negbin', action='store_true')
    ap.add_argument('--n', type=int, default=400)
    ap.add_argument('--chains', type=int, default=16)
    ap.add_argument('--warmup', type=int, default=200)
    ap.add_argument('--keep', type=int, default=200)
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    if args.negbin:
        return negbin(args, dev)
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
