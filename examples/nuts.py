#!/usr/bin/env python3
"""The no-U-turn sampler on a badly conditioned, rotated Gaussian.

The 8-dimensional Gaussian of ``adapted_metric.py --dense`` (standard deviations 1 ... 100,
rotated by a fixed random orthogonal matrix), written as a user's torch PDF.  16 chains start
3 sigma out; ``warmup(NUTSSampler, 300, dense=True)`` learns the Cholesky factor of the
covariance while dual averaging tunes every chain's step towards a mean acceptance statistic
of 0.8; 200 transitions are kept.  Printed: R^ / ESS of the kept draws, the histogram of tree
depths, divergences, the adapted steps.

    python examples/nuts.py [--chains 16] [--warmup 300] [--keep 200] [--max-depth 8] [--seed 0]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from binf_amd import diagnostics
from binf_amd.samplers import NUTSSampler
from binf_amd.samplers.rng import DeviceRNG
from binf_amd.samplers.warmup import warmup


class RotatedGauss(object):
    """log p(x) = -1/2 x^T P x."""

    def __init__(self, precision):
        self.P = precision

    def log_prob(self, x):
        return -0.5 * (x * (x @ self.P)).sum(dim=1)

    def gradient(self, x):
        return x @ self.P


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--chains', type=int, default=16)
    ap.add_argument('--warmup', type=int, default=300)
    ap.add_argument('--keep', type=int, default=200)
    ap.add_argument('--max-depth', type=int, default=8)
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    sigma = 100.0 ** (np.arange(8) / 7.0)
    Q, _ = np.linalg.qr(np.random.RandomState(1000).standard_normal((8, 8)))
    true_chol = np.linalg.cholesky((Q * sigma ** 2) @ Q.T)
    P = torch.from_numpy((Q / sigma ** 2) @ Q.T).to(dev)
    rng = DeviceRNG(args.seed, dev)
    x0 = 3.0 * rng.normal((args.chains, 8), dev) @ torch.from_numpy(true_chol).to(dev).T
    s = NUTSSampler(RotatedGauss(P), x0, 0.5, max_tree_depth=args.max_depth, target_accept=0.8,
                    variable_name='x', rng=rng)
    warmup(s, args.warmup, dense=True)
    div_warm = int(s.n_divergent.sum())
    depths, leaps = [], []
    kept = torch.empty((args.keep,) + tuple(x0.shape), dtype=torch.float64, device=dev)
    for i in range(args.keep):
        kept[i] = s.sample()
        depths.append(s.last_tree_depth)
        leaps.append(s.last_n_leapfrog)
    M = np.linalg.solve(true_chol, s.metric_chol[0].cpu().numpy())
    ev = np.linalg.eigvalsh(M @ M.T)
    print(diagnostics.summary(kept).table(['x%d' % i for i in range(8)]))
    hist = torch.bincount(torch.stack(depths).reshape(-1), minlength=args.max_depth + 1).cpu().tolist()
    print('\ntree depth   ' + ' '.join('%6d' % d for d in range(len(hist))))
    print('transitions  ' + ' '.join('%6d' % h for h in hist))
    print('leapfrog steps per transition: mean %.1f' % float(torch.stack(leaps).double().mean()))
    print('divergences: %d in the warm-up, %d after' % (div_warm, int(s.n_divergent.sum()) - div_warm))
    print('adapted steps: %.3f ... %.3f (mean accept_stat of the last transition %.2f)'
          % (float(s.timestep.min()), float(s.timestep.max()), float(s.last_accept_stat.mean())))
    print('learnt M^-1 whitened by the true covariance: eigenvalues %.3g ... %.3g' % (ev.min(), ev.max()))


if __name__ == '__main__':
    main()
