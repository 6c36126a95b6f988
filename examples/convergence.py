#!/usr/bin/env python3
"""
Has the run converged, and what is the record worth?  Split-R^, effective sample size and
Monte-Carlo standard error per dimension, computed on the device from the kept draws
(``binf_amd/diagnostics.py``, ``csrc/diagnostics.hip``).

Default run: the Gaussian chains of ``examples/gaussian_chains.py`` (BASELINE config C2) from
an over-dispersed start.  The table after a handful of transitions shows R^ well above 1 --
the chains still remember where they started -- and the table after a long run shows R^ at 1
and an effective sample size of a fixed fraction of the draws.

  python examples/convergence.py --chains 4096 --dims 8 --short 8 --long 400

``--ladder``: the double well of ``examples/replica_exchange.py``, half of the ladders
started in either well, diagnosed on the cold slot only (``draws[:, 0::R, :]``, a strided
view: nothing is copied).  Without the swaps no cold chain ever changes wells and R^ stays far
above 1; with them the cold slot mixes and R^ comes down to 1.

  python examples/convergence.py --ladder --ladders 256 --rounds 300

``--rank``: after each table, the rank-based one (``diagnostics.rank_summary``, a sort of the
record per dimension on the device, ``csrc/ranks.hip``): the larger of the rank-normalised and
the folded split-R^, which also sees chains that agree in mean and differ in scale -- cold
chains in wells of different width --, bulk and tail ESS, and the 5 %, 50 % and 95 % quantiles.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.append(os.path.dirname(os.path.abspath(__file__)))            # replica_exchange.py
from binf_amd import diagnostics
from binf_amd.dist import SampleStore
from binf_amd.pdf import IsotropicGaussian
from binf_amd.samplers.hmc import HMCSampler
from binf_amd.samplers.rng import DeviceRNG


def run_gaussian(args, dev):
    C, D = args.chains, args.dims
    rng = DeviceRNG(args.seed, dev)
    start = args.spread * (2.0 * rng.uniform(C * D, dev).reshape(C, D) - 1.0)
    sampler = HMCSampler(IsotropicGaussian(1.0, 0.0), start, args.timestep, args.nsteps,
                         variable_name='x', rng=rng)
    store = SampleStore(args.short + args.long, C, D, device=dev)
    store.extend(sampler.sample_n(args.short))
    short = store.summary()
    print('after %d transitions of %d chains (start spread +-%g):' % (args.short, C, args.spread))
    print(short.table())
    if args.rank:
        print(store.rank_summary().table())
    store.extend(sampler.sample_n(args.long))
    kept = store.local()[args.short + args.long // 2:]                 # the second half of the long run
    long = diagnostics.summary(kept)
    print('draws %d .. %d:' % (args.short + args.long // 2, args.short + args.long))
    print(long.table())
    if args.rank:
        print(diagnostics.rank_summary(kept).table())
    print('acceptance rate: %.3f' % float(sampler.acceptance_rate.mean()))
    return short, long


def run_ladder(args, dev):
    from binf_amd.samplers.replica import ReplicaExchangeSampler
    from replica_exchange import TemperedDoubleWell
    betas = [1.0, 0.5, 0.25, 0.12, 0.06, 0.03]
    R = len(betas)
    C = args.ladders * R
    beta = torch.tensor(betas, dtype=torch.float64, device=dev).repeat(args.ladders)
    # ladders alternately in the right-hand and the left-hand well
    side = torch.where(torch.arange(C, device=dev) // R % 2 == 0, 1.0, -1.0).to(torch.float64)
    start = side[:, None].repeat(1, args.ladder_dims).contiguous()
    out = []
    for swaps in (False, True):
        inner = HMCSampler(TemperedDoubleWell(args.a, beta), start.clone(), args.ladder_timestep, 8,
                           variable_name='x', rng=DeviceRNG(args.seed, dev))
        sampler = ReplicaExchangeSampler(inner, R, swap_interval=2) if swaps else inner
        store = SampleStore(args.rounds, C, args.ladder_dims, device=dev)
        for _ in range(args.rounds):
            if swaps:
                x = sampler.sample()
            else:
                sampler.sample()
                x = sampler.sample()
            store.record(x)
        cold = store.local()[:, 0::R, :]                                # slot 0 of every ladder
        s = diagnostics.summary(cold)
        print('cold slot of %d ladders, %d rounds, %s:' % (args.ladders, args.rounds,
                                                          'with swaps' if swaps else 'WITHOUT swaps'))
        print(s.table())
        if args.rank:
            print(diagnostics.rank_summary(cold).table())
        out.append(s)
    return tuple(out)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--chains', type=int, default=4096)
    ap.add_argument('--dims', type=int, default=8)
    ap.add_argument('--short', type=int, default=8, help='transitions before the first table')
    ap.add_argument('--long', type=int, default=400, help='further transitions before the second')
    ap.add_argument('--nsteps', type=int, default=20)
    ap.add_argument('--timestep', type=float, default=0.05)
    ap.add_argument('--spread', type=float, default=10.0, help='the start is uniform in +-spread')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--ladder', action='store_true', help='the cold slot of the tempered double well')
    ap.add_argument('--rank', action='store_true', help='the rank-based table after each table')
    ap.add_argument('--ladders', type=int, default=256)
    ap.add_argument('--rounds', type=int, default=300)
    ap.add_argument('--ladder-dims', type=int, default=1)
    ap.add_argument('--ladder-timestep', type=float, default=0.07)
    ap.add_argument('--a', type=float, default=16.0)
    args = ap.parse_args(argv)
    dev = torch.device('cuda', torch.cuda.current_device())
    return run_ladder(args, dev) if args.ladder else run_gaussian(args, dev)


if __name__ == '__main__':
    main()
