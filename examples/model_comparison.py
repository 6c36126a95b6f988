#!/usr/bin/env python3
"""
Which polynomial degree PREDICTS best?  Data from a cubic plus noise, polynomial fits of
degree 1 .. 6 through the Gibbs-within-HMC wiring of examples/polynomial_fit.py, and for each
the leave-one-out predictive accuracy (PSIS-LOO) with its Pareto-k^ diagnostic and WAIC --
the companion of the evidence that examples/free_energy.py and examples/smc_evidence.py
estimate.  The pointwise log-likelihood record [draws x observations], its sort per
observation, the generalised-Pareto fits and the log-sum-exps all run on the device
(binf_amd/loo.py, csrc/loo.hip).

With --outlier one observation is moved far off the curve: its k^ is printed, which is what
the diagnostic is for -- the estimate for THAT point rests on a few draws and is flagged
instead of silently trusted.

  python examples/model_comparison.py
  python examples/model_comparison.py --outlier --chains 2048
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from binf_amd import loo
from binf_amd.example.likelihood import make_likelihood
from binf_amd.example.priors import GammaPrior, GaussianPrior
from binf_amd.example.samplers import make_hmc_sampler
from binf_amd.pdf.posteriors import Posterior
from binf_amd.samplers import BinfState
from binf_amd.samplers.rng import DeviceRNG


def fit(xs, ys, degree, args, dev):
    """(likelihood, coefficients [kept x chains x degree + 1], precision [kept x chains])."""
    K, C = degree + 1, args.chains
    polynomial = np.polynomial.polynomial.polyval
    lik = make_likelihood(xs, ys, polynomial)
    pp, cp = GammaPrior(1.0, 0.2), GaussianPrior(means=np.zeros(K), variances=np.ones(K) * 5)
    posterior = Posterior({lik.name: lik}, {pp.name: pp, cp.name: cp})
    start = BinfState(dict(coefficients=torch.ones((C, K), dtype=torch.float64, device=dev),
                           precision=torch.ones(C, dtype=torch.float64, device=dev)))
    gips = make_hmc_sampler(posterior, args.timestep, args.nsteps, start, rng=DeviceRNG(args.seed + degree, dev))
    gips.sample_n(args.burn_in, record=False)
    rec = gips.sample_n(args.kept * args.thin, thin=args.thin)
    return lik, rec['coefficients'], rec['precision']


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--chains', type=int, default=1024)
    ap.add_argument('--points', type=int, default=60)
    ap.add_argument('--burn-in', type=int, default=1000)
    ap.add_argument('--kept', type=int, default=20, help='kept sweeps per chain')
    ap.add_argument('--thin', type=int, default=10)
    ap.add_argument('--timestep', type=float, default=0.01)
    ap.add_argument('--nsteps', type=int, default=40)
    ap.add_argument('--max-degree', type=int, default=6)
    ap.add_argument('--outlier', action='store_true', help='move one observation 8 noise sd off the curve')
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args(argv)
    dev = torch.device('cuda', torch.cuda.current_device())

    rs = np.random.RandomState(args.seed)
    real_coeffs, real_precision = np.array([2.0, -4.0, 1.0, 1.5]), 2.5
    xs = np.linspace(-2, 2, args.points)
    ys = np.polynomial.polynomial.polyval(xs, real_coeffs) + rs.standard_normal(args.points) / np.sqrt(real_precision)
    where = args.points // 3
    if args.outlier:
        ys[where] += 8.0 / np.sqrt(real_precision)

    results = {}
    print('%-6s %12s %8s %8s %12s %8s %6s' % ('degree', 'elpd_loo', 'se', 'p_loo', 'elpd_waic', 'max k^', 'n_bad'))
    for degree in range(1, args.max_degree + 1):
        lik, c, tau = fit(xs, ys, degree, args, dev)
        ll = loo.pointwise_log_likelihood(lik, (c, tau.reshape(-1)))          # [kept * chains x points]
        r, w = loo.loo(ll.view(c.shape[0], c.shape[1], -1)), loo.waic(ll)
        results[degree] = r
        print('%-6d %12.3f %8.3f %8.2f %12.3f %8.3f %6d'
              % (degree, r.elpd, r.se, r.p_loo, w.elpd, float(r.khat.max()), r.n_bad))
    best = max(results, key=lambda d: results[d].elpd)
    print('\nbest degree by elpd_loo: %d (the data come from degree 3)' % best)
    print('%-6s %12s %10s' % ('degree', 'elpd_diff', 'se_diff'))
    for degree in sorted(results):
        diff, se = loo.compare(results[degree], results[best])
        print('%-6d %12.3f %10.3f' % (degree, diff, se))
    if args.outlier:
        r = results[3]
        print('\nthe outlier is observation %d (x = %.2f): under degree 3 its k^ is %.3f, elpd_i %.3f, n_eff %.0f '
              'of %d draws; the median k^ of the others is %.3f'
              % (where, xs[where], float(r.khat[where]), float(r.elpd_i[where]), float(r.n_eff[where]),
                 c.shape[0] * c.shape[1], float(torch.cat((r.khat[:where], r.khat[where + 1:])).median())))
    return results


if __name__ == '__main__':
    main()
