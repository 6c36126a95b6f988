#!/usr/bin/env python3
"""
Replica exchange: C = n_ladders x R chains, slot r of every ladder samples a tempered
copy of the target, neighbouring slots exchange their states on the device
(``binf_amd/samplers/replica.py``, ``csrc/replica.hip``).  Slot 0 is the target.

Default run: the double well of ``examples/custom_pdf.py`` with a per-chain ``beta``,
log p_c(x) = -beta_c a sum_d (x_d^2 - 1)^2 with a barrier no cold chain crosses.  Every chain
starts in the right-hand well; with the swaps the cold slot ends up half left, half right,
without them it stays where it started.

  python examples/replica_exchange.py --ladders 512 --rounds 150

``--restraints``: the pairwise-distance-restraint posterior of
``examples/distance_restraints.py`` (BASELINE config C5) on a precision ladder -- the
likelihood takes a per-chain precision, so the tempered ladder L(x)^beta_r pi(x) is
``precision = beta_r * tau`` per chain and no kernel changes.  Prints the swap rates per slot
pair and the walkers' round trips (bottom slot -> top slot -> bottom slot).

  python examples/replica_exchange.py --restraints --ladders 64 --replicas 8 --beads 64
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.append(os.path.dirname(os.path.abspath(__file__)))            # custom_pdf.py, when imported
from binf_amd.samplers.hmc import HMCSampler
from binf_amd.samplers.replica import ReplicaExchangeSampler, geometric_betas, ladder_precision
from binf_amd.samplers.rng import DeviceRNG
from custom_pdf import DoubleWell


class TemperedDoubleWell(DoubleWell):
    """log p_c(x) = -beta_c a sum_d (x_d^2 - 1)^2: ``beta`` is a ``[C]`` tensor, one inverse
    temperature per chain."""

    def __init__(self, a, beta):
        super(TemperedDoubleWell, self).__init__(a)
        self.beta = beta

    def log_prob(self, x):
        return self.beta * super(TemperedDoubleWell, self).log_prob(x)

    def gradient(self, x):
        return self.beta[:, None] * super(TemperedDoubleWell, self).gradient(x)


def round_trips(walker_history, n_replicas):
    """Completed bottom -> top -> bottom trips per walker from the ``[n_rounds, C]`` record of
    ``ReplicaExchangeSampler.walker`` (host arithmetic, after the run)."""
    w = walker_history.cpu().numpy()
    n, C = w.shape
    slot_of = np.empty_like(w)
    slot_of[np.arange(n)[:, None], w] = np.arange(C)[None, :] % n_replicas     # slot of walker id at round t
    trips = np.zeros(C, dtype=np.int64)
    heading_up = np.ones(C, dtype=bool)          # a walker counts from its first visit to the bottom
    started = slot_of[0] == 0
    for t in range(n):
        s = slot_of[t]
        started |= s == 0
        top = started & heading_up & (s == n_replicas - 1)
        heading_up[top] = False
        back = started & ~heading_up & (s == 0)
        trips[back] += 1
        heading_up[back] = True
    return trips


def run_double_well(args, dev):
    betas = [1.0, 0.5, 0.25, 0.12, 0.06, 0.03] if args.replicas is None else \
        geometric_betas(args.replicas, args.beta_min)
    R = len(betas)
    C = args.ladders * R
    beta = torch.tensor(betas, dtype=torch.float64, device=dev).repeat(args.ladders)
    rng = DeviceRNG(args.seed, dev)
    start = torch.ones((C, args.dims), dtype=torch.float64, device=dev)
    inner = HMCSampler(TemperedDoubleWell(args.a, beta), start, args.timestep, args.nsteps,
                       variable_name='x', rng=rng)
    re = ReplicaExchangeSampler(inner, R, swap_interval=args.swap_interval)
    for _ in range(args.rounds):
        x = re.sample()
    plain = HMCSampler(TemperedDoubleWell(args.a, beta), start, args.timestep, args.nsteps,
                       variable_name='x', rng=DeviceRNG(args.seed, dev))
    for _ in range(args.rounds * args.swap_interval):
        y = plain.sample()
    print('betas                              :', ' '.join('%.3g' % b for b in betas))
    print('swap acceptance per slot pair      :', ' '.join('%.3f' % r for r in re.swap_acceptance_rate.tolist()))
    print('cold slot, fraction in the left well: %.3f with swaps, %.3f without (target 0.5)'
          % (float((re.slot(x, 0) < 0).double().mean()), float((re.slot(y, 0) < 0).double().mean())))
    return re


def run_restraints(args, dev):
    from binf_amd.example.distance import make_distance_likelihood
    from binf_amd.pdf import IsotropicGaussian
    from binf_amd.pdf.posteriors import Posterior
    n = args.beads
    R = 8 if args.replicas is None else args.replicas
    C = args.ladders * R
    rs = np.random.RandomState(args.seed)
    truth = np.cumsum(rs.standard_normal((n, 3)), axis=0) * 0.5
    I, J = np.triu_indices(n, 1)
    d_true = np.sqrt(((truth[I] - truth[J]) ** 2).sum(1))
    ys = np.abs(d_true + rs.standard_normal(d_true.shape) / np.sqrt(args.precision))
    lik = make_distance_likelihood(ys, n)
    prior = IsotropicGaussian(0.01, 0.0, name='coordinates_prior', variable_name='coordinates')
    betas = geometric_betas(R, args.beta_min)
    tau = ladder_precision(betas, args.precision, args.ladders, dev)
    cond = Posterior({lik.name: lik}, {prior.name: prior}).conditional_factory(precision=tau)
    rng = DeviceRNG(args.seed + 1, dev)
    start = torch.from_numpy(truth.reshape(1, -1)).to(dev) + 0.3 * rng.normal((C, 3 * n), dev)
    # a hotter slot takes a longer step: the force scales with beta
    dt = args.restraint_timestep / torch.tensor(betas, dtype=torch.float64, device=dev).sqrt().repeat(args.ladders)
    inner = HMCSampler(cond, start, dt, args.nsteps, variable_name='coordinates', rng=rng,
                       timestep_adaption_limit=args.rounds * args.swap_interval // 2)
    re = ReplicaExchangeSampler(inner, R, swap_interval=args.swap_interval, track_walkers=True)
    history = torch.empty((args.rounds, C), dtype=torch.int64, device=dev)
    for i in range(args.rounds):
        x = re.sample()
        history[i].copy_(re.walker)
    trips = round_trips(history, R)
    cold = re.slot(x, 0).reshape(-1, n, 3)
    Id, Jd = torch.from_numpy(I).to(dev), torch.from_numpy(J).to(dev)
    d = (cold[:, Id] - cold[:, Jd]).pow(2).sum(-1).sqrt()
    rmsd = (d - torch.from_numpy(d_true).to(dev)).pow(2).mean().sqrt()
    print('precision ladder                   :', ' '.join('%.3g' % (b * args.precision) for b in betas))
    print('swap acceptance per slot pair      :', ' '.join('%.3f' % r for r in re.swap_acceptance_rate.tolist()))
    print('HMC acceptance per slot            :', ' '.join(
        '%.3f' % float(re.slot(inner.acceptance_rate, r).mean()) for r in range(R)))
    print('walker round trips                 : %d in all, %.2f per walker, %d walkers with none'
          % (trips.sum(), trips.mean(), int((trips == 0).sum())))
    print('cold slot, distance RMSD to truth  : %.3f (noise sd %.3f)' % (float(rmsd), 1.0 / np.sqrt(args.precision)))
    return re


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--ladders', type=int, default=512)
    ap.add_argument('--replicas', type=int, default=None, help='slots per ladder (default: 6 / 8 with --restraints)')
    ap.add_argument('--beta-min', type=float, default=None,
                    help='beta of the top slot of a geometric ladder (default 0.03; 0.75 with --restraints: the\n'
                         'energy of P restraints fluctuates by ~sqrt(P / 2), neighbours must overlap)')
    ap.add_argument('--rounds', type=int, default=150)
    ap.add_argument('--swap-interval', type=int, default=2, help='transitions per swap round')
    ap.add_argument('--nsteps', type=int, default=8)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--dims', type=int, default=1)
    ap.add_argument('--a', type=float, default=16.0)
    ap.add_argument('--timestep', type=float, default=0.07)
    ap.add_argument('--restraints', action='store_true', help='the distance-restraint posterior on a precision ladder')
    ap.add_argument('--beads', type=int, default=64)
    ap.add_argument('--precision', type=float, default=4.0)
    ap.add_argument('--restraint-timestep', type=float, default=0.002)
    args = ap.parse_args(argv)
    if args.beta_min is None:
        args.beta_min = 0.75 if args.restraints else 0.03
    dev = torch.device('cuda', torch.cuda.current_device())
    return run_restraints(args, dev) if args.restraints else run_double_well(args, dev)


if __name__ == '__main__':
    main()
