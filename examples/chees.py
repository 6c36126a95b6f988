#!/usr/bin/env python3
"""ChEES-HMC: one trajectory length for all chains, learnt during warm-up.

The 16-dimensional Gaussian with standard deviations 1 ... 10, plain and rotated by a fixed
random orthogonal matrix, written as a user's torch PDF.  On the plain target the sampler adapts
with the identity mass (``timestep_adaption_limit``): the step size eps and the trajectory length
T are learnt from the whole batch.  On the rotated one ``warmup(ChEESSampler, n, dense=True)``
learns the Cholesky factor of the covariance too.  Afterwards the sampler is fixed-length HMC
with a jittered step count.  Printed per target: the learnt T, eps and mean leapfrog steps per
transition, and the leapfrog steps per unit of minimum bulk ESS beside ``NUTSSampler``'s on the
same target, warm-up and number of kept draws -- the steps a chain takes, and the steps
launched (every chain of a NUTS batch waits for the longest tree).

    python examples/chees.py [--chains 64] [--warmup 500] [--keep 200] [--seed 0]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from binf_amd import diagnostics
from binf_amd.samplers import ChEESSampler, NUTSSampler
from binf_amd.samplers.rng import DeviceRNG
from binf_amd.samplers.warmup import warmup


class Gauss(object):
    """log p(x) = -1/2 x^T P x."""

    def __init__(self, precision):
        self.P = precision

    def log_prob(self, x):
        return -0.5 * (x * (x @ self.P)).sum(dim=1)

    def gradient(self, x):
        return x @ self.P


def run(make, x0, n_warmup, n_keep, dense):
    """Warm up, keep ``n_keep`` transitions; returns the sampler, the mean leapfrog steps a chain
    took per kept transition, the mean number of steps LAUNCHED per kept transition (a NUTS
    transition runs until its longest tree is done) and the minimum bulk ESS of the kept draws."""
    s = make(x0.clone())
    if dense:
        # a long last fast phase: after the last change of metric the trajectory length has to
        # find its place again, at no more than the learning rate per transition
        warmup(s, n_warmup, dense=True, term_buffer=(2 * n_warmup) // 5)
    else:
        s.timestep_adaption_limit = n_warmup + 1
        for _ in range(n_warmup):
            s.sample()
    kept = torch.empty((n_keep,) + tuple(x0.shape), dtype=torch.float64, device=x0.device)
    steps = launched = 0.0
    for i in range(n_keep):
        kept[i] = s.sample()
        n = s.last_n_leapfrog
        steps += float(n.double().mean()) if isinstance(n, torch.Tensor) else float(n)
        launched += float(n.max()) if isinstance(n, torch.Tensor) else float(n)
    ess = float(diagnostics.rank_summary(kept).ess_bulk.min())
    return s, steps / n_keep, launched / n_keep, ess


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--chains', type=int, default=64)
    ap.add_argument('--warmup', type=int, default=500)
    ap.add_argument('--keep', type=int, default=200)
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    D = 16
    sigma = np.linspace(1.0, 10.0, D)
    Q, _ = np.linalg.qr(np.random.RandomState(1000).standard_normal((D, D)))
    for name, R, dense in (('plain', np.eye(D), False), ('rotated, dense=True', Q, True)):
        P = torch.from_numpy((R / sigma ** 2) @ R.T).to(dev)
        chol = torch.from_numpy(np.linalg.cholesky((R * sigma ** 2) @ R.T)).to(dev)
        x0 = DeviceRNG(args.seed + 1, dev).normal((args.chains, D), dev) @ chol.T
        pdf = Gauss(P)
        c, c_steps, c_launched, c_ess = run(
            lambda x: ChEESSampler(pdf, x, 0.1, variable_name='x', rng=DeviceRNG(args.seed, dev)),
            x0, args.warmup, args.keep, dense)
        n, n_steps, n_launched, n_ess = run(
            lambda x: NUTSSampler(pdf, x, 0.1, max_tree_depth=8, variable_name='x', rng=DeviceRNG(args.seed, dev)),
            x0, args.warmup, args.keep, dense)
        total = args.keep * args.chains
        print('%s: sigma = 1 ... 10, %d chains, %d warm-up + %d kept transitions' % (name, args.chains, args.warmup, args.keep))
        print('  ChEES  T %.3f  eps %.3f  mean L %.2f (without jitter: %d)   min bulk ESS %.0f   '
              'leapfrog steps per ESS: taken %.2f = launched %.2f'
              % (c.trajectory_length, c.timestep, c_steps, c.mean_leapfrog_steps, c_ess,
                 c_steps * total / c_ess, c_launched * total / c_ess))
        print('  NUTS   eps %.3f ... %.3f  mean L %.2f, longest tree %.2f   min bulk ESS %.0f   '
              'leapfrog steps per ESS: taken %.2f, launched %.2f'
              % (float(n.timestep.min()), float(n.timestep.max()), n_steps, n_launched, n_ess,
                 n_steps * total / n_ess, n_launched * total / n_ess))


if __name__ == '__main__':
    main()
