#!/usr/bin/env python3
"""
Fourier-basis regression: a periodic signal sampled at irregular points, fitted with
a truncated Fourier series -- a model that is linear in its parameters but that the
example's polynomial class cannot express.  The user's side is a subclass of
LinearForwardModel that builds its design matrix; log-prob, gradient and the leapfrog
integration then run in the fused HIP kernels of the registered kind 'linear'.

Gibbs-within-HMC as in examples/polynomial_fit.py: HMC on the coefficients, the
conjugate Gamma draw on the noise precision; many chains at once, sharded over the
ranks when torch.distributed is initialised.

--resident builds the model with resident=True: at this size (a handful of coefficients,
a few hundred data points) the per-step path is launch-bound, and the burn-in and the
kept sweeps then run through GibbsSampler.sample_n -- every block of sweeps ONE launch
of the chain-resident kernel, the state of a chain on chip in between.

  python examples/linear_basis.py --chains 4096 --iterations 600
  python examples/linear_basis.py --chains 4096 --iterations 600 --resident
  python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 \\
      --master-addr 127.0.0.1 examples/linear_basis.py --chains 32768
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from binf_amd.dist import SampleStore, shard_chains, world
from binf_amd.example.likelihood import GaussianErrorModel
from binf_amd.example.priors import GammaPrior, GaussianPrior
from binf_amd.example.samplers import make_hmc_sampler
from binf_amd.model.linear import LinearForwardModel
from binf_amd.pdf.likelihoods import Likelihood
from binf_amd.pdf.posteriors import Posterior
from binf_amd.samplers import BinfState
from binf_amd.samplers.rng import DeviceRNG


class FourierSeries(LinearForwardModel):
    """mock(x) = c0 + sum_m a_m cos(m x) + b_m sin(m x), m = 1 .. n_modes."""

    def __init__(self, xs, n_modes, resident=False):
        self.xs, self.n_modes = np.asarray(xs, dtype=np.float64), int(n_modes)
        rows = [np.ones_like(self.xs)]
        for m in range(1, self.n_modes + 1):
            rows += [np.cos(m * self.xs), np.sin(m * self.xs)]
        super(FourierSeries, self).__init__('fourier_series', np.vstack(rows), resident=resident)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--chains', type=int, default=1024, help='total over all ranks')
    ap.add_argument('--iterations', type=int, default=600)
    ap.add_argument('--burn-in', type=int, default=200)
    ap.add_argument('--thin', type=int, default=10)
    ap.add_argument('--modes', type=int, default=4)
    ap.add_argument('--data', type=int, default=200)
    ap.add_argument('--timestep', type=float, default=0.01)
    ap.add_argument('--nsteps', type=int, default=30)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--resident', action='store_true',
                    help='opt the model into the chain-resident kernels and sweep with sample_n')
    args = ap.parse_args(argv)

    if 'RANK' in os.environ and int(os.environ.get('WORLD_SIZE', '1')) > 1:
        import torch.distributed as dist
        torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', '0')))
        dist.init_process_group('nccl')
    rank, ws = world()
    dev = torch.device('cuda', torch.cuda.current_device())
    start_chain, C = shard_chains(args.chains, rank, ws)

    # the data: every rank makes the same
    rs = np.random.RandomState(args.seed)
    K = 2 * args.modes + 1
    real_coeffs = rs.standard_normal(K) / (1.0 + np.arange(K) // 2)
    real_precision = 4.0
    xs = np.sort(rs.uniform(0.0, 2 * np.pi, size=args.data))
    model = FourierSeries(xs, args.modes, resident=args.resident)
    ys = real_coeffs.dot(model.design) + rs.standard_normal(args.data) / np.sqrt(real_precision)

    # the likelihood must be called 'points' and the variable 'coefficients' for the
    # example's GammaSampler (binf_amd/example/samplers.py)
    likelihood = Likelihood('points', model, GaussianErrorModel(ys))
    assert likelihood._native_pair() is not None          # the fused kind took the pair
    posterior = Posterior({likelihood.name: likelihood},
                          {'precision_prior': GammaPrior(1.0, 0.2),
                           'coefficients_prior': GaussianPrior(np.zeros(K), np.full(K, 5.0))})
    start = BinfState(dict(
        coefficients=torch.zeros((C, K), dtype=torch.float64, device=dev),
        precision=torch.ones(C, dtype=torch.float64, device=dev)))
    # one seed for the whole run; the streams are keyed by the GLOBAL chain index
    rng = DeviceRNG(args.seed, dev, chain_offset=start_chain)
    gips = make_hmc_sampler(posterior, args.timestep, args.nsteps, start, rng=rng)

    n_keep = max(1, (args.iterations - args.burn_in + args.thin - 1) // args.thin)
    store_c = SampleStore(n_keep, C, K, thin=args.thin, burn_in=args.burn_in, device=dev)
    store_p = SampleStore(n_keep, C, 1, thin=args.thin, burn_in=args.burn_in, device=dev)
    if args.resident:
        # the burn-in in one launch, nothing recorded; then the kept sweeps, the state after
        # every thin-th one recorded by the kernel itself
        if args.burn_in > 0:
            gips.sample_n(args.burn_in, record=False)
        rec = gips.sample_n(args.iterations - args.burn_in, thin=args.thin) \
            if args.iterations > args.burn_in else None
        if rec is not None and rec['coefficients'].shape[0] > 0:
            store_c.extend(rec['coefficients'])
            store_p.extend(rec['precision'])
        if rank == 0:
            acc = gips.subsamplers['coefficients'].acceptance_rate
            print('coefficient sampler acceptance {:.3f}'.format(float(acc.mean())))
    else:
        for i in range(args.iterations):
            state = gips.sample()
            store_c.record(state.variables['coefficients'])
            store_p.record(state.variables['precision'])
            if rank == 0 and i % 200 == 0 and i > 0:
                acc = gips.last_draw_stats['coefficients'].accepted.double()
                print('sweep {}: coefficient sampler acceptance {:.3f}'.format(i, float(acc.mean())))

    coeffs = store_c.gather(args.chains)           # [n_kept, chains, K] on every rank
    prec = store_p.gather(args.chains)
    if rank == 0 and coeffs.shape[0] > 0:
        c = coeffs.reshape(-1, K)
        print('kept {} draws x {} chains'.format(coeffs.shape[0], coeffs.shape[1]))
        print('true coefficients     :', real_coeffs.round(3), ' precision', real_precision)
        print('posterior mean (coeff):', c.mean(0).cpu().numpy().round(3))
        print('posterior std  (coeff):', c.std(0).cpu().numpy().round(3))
        print('posterior mean (prec) : {:.3f}'.format(float(prec.mean())))
    return coeffs, prec


if __name__ == '__main__':
    main()
