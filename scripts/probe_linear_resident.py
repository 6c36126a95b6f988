"""Where the chain-resident kernels of a linear forward model (resident=True,
csrc/linear_chain_kernel.hpp) beat the per-step path, and how far they are from the
polynomial kind's resident kernel -- the measurement behind
binf_amd/model/linear_resident.py:RESIDENT_MAX_WORK (development aid).

For every (chains, K, N, L) it times, alternating the paths round by round:
  per-step   the same model without the flag: HMCSampler.sample() / GibbsSampler.sample()
             (binf_linear_gauss_logp_f64, binf_poly_leapfrog_f64, the Gamma draw)
  resident   HMCSampler.sample_n(n) / GibbsSampler.sample_n(n): one launch for n
  poly       the polynomial kind's resident kernel on the power basis of the same
             (K, N) -- the yardstick
and prints one JSON object: microseconds per transition and per Gibbs sweep, each the
median over the rounds, with the spread (min, max).  fused_transition='always' keeps the
resident path on beyond the threshold, so that the crossover itself is measured.

  python scripts/probe_linear_resident.py [--quick] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from binf_amd.example.likelihood import POLYVAL, ForwardModel, GaussianErrorModel
from binf_amd.example.priors import GammaPrior, GaussianPrior
from binf_amd.example.samplers import make_hmc_sampler
from binf_amd.model.linear import LinearForwardModel
from binf_amd.pdf.likelihoods import Likelihood
from binf_amd.pdf.posteriors import Posterior
from binf_amd.samplers import BinfState
from binf_amd.samplers.hmc import HMCSampler
from binf_amd.samplers.rng import DeviceRNG


class PowerBasis(LinearForwardModel):
    def __init__(self, xs, K, resident=False):
        super(PowerBasis, self).__init__('power_basis', np.vstack([xs ** i for i in range(K)]),
                                         resident=resident)


def posterior(fwm, ys, K):
    lik = Likelihood('points', fwm, GaussianErrorModel(ys))
    return Posterior({lik.name: lik}, {'precision_prior': GammaPrior(1.0, 0.2),
                                       'coefficients_prior': GaussianPrior(np.zeros(K), np.ones(K) * 5)})


def build(path, what, C, K, N, L, dev):
    rs = np.random.RandomState(0)
    xs = np.linspace(-1, 1, N)
    ys = POLYVAL(xs, rs.standard_normal(K)) + rs.standard_normal(N) / np.sqrt(2.5)
    fwm = ForwardModel(xs, POLYVAL) if path == 'poly' else PowerBasis(xs, K, resident=(path == 'resident'))
    post = posterior(fwm, ys, K)
    q0 = torch.from_numpy(rs.standard_normal((C, K)) * 0.1).to(dev)
    dt = 0.2 / np.sqrt(2.5 * N * K)
    if what == 'transition':
        cond = post.conditional_factory(precision=torch.full((C,), 2.5, dtype=torch.float64, device=dev))
        s = HMCSampler(cond, q0, dt, L, variable_name='coefficients', rng=DeviceRNG(0, dev))
        hmc = s
    else:
        start = BinfState(dict(coefficients=q0, precision=torch.full((C,), 2.5, dtype=torch.float64, device=dev)))
        s = make_hmc_sampler(post, dt, L, start, rng=DeviceRNG(0, dev))
        hmc = s.subsamplers['coefficients']
    if path != 'per-step':
        hmc.fused_transition = 'always' if path == 'resident' else 'group'
    return s


def one_round(s, path, n):
    """Seconds per transition / sweep of one timed window."""
    torch.cuda.synchronize()
    t = time.perf_counter()
    if path == 'per-step':
        for _ in range(n):
            s.sample()
    else:
        s.sample_n(n, record=False)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n


def measure(C, K, N, L, dev, rounds, budget_s):
    out = {}
    for what in ('transition', 'sweep'):
        samplers = {p: build(p, what, C, K, N, L, dev) for p in ('per-step', 'resident', 'poly')}
        # sweeps per window: enough work to time, sized by a first look at each path
        n = {}
        for p, s in samplers.items():
            one_round(s, p, 3)                                  # warm-up: code objects, caches
            t1 = one_round(s, p, 5)
            # (a launch of n sweeps writes n x C flags and energies: keep that small)
            n[p] = int(max(5, min(2000, 3e7 / C, budget_s / max(t1, 1e-7))))
        times = {p: [] for p in samplers}
        for _ in range(rounds):                                 # alternate the paths
            for p, s in samplers.items():
                times[p].append(one_round(s, p, n[p]))
        for p, ts in times.items():
            out['%s %s' % (what, p)] = {'us_median': float(np.median(ts)) * 1e6, 'us_min': min(ts) * 1e6,
                                        'us_max': max(ts) * 1e6, 'per_window': n[p]}
        out['%s per-step / resident' % what] = float(np.median(times['per-step']) / np.median(times['resident']))
        out['%s resident / poly' % what] = float(np.median(times['resident']) / np.median(times['poly']))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--quick', action='store_true', help='the three headline shapes only')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.25, help='seconds of work per timed window')
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    dev = torch.device('cuda:0')
    shapes = [(4096, 8, 512, 20), (1024, 9, 200, 30), (4096, 9, 200, 30)]
    if not args.quick:
        # the crossover: chains x N x K from 1e6 to 1e9 at small, medium and the largest shape
        shapes += [(C, K, N, 20) for K, N in ((4, 20), (9, 200), (16, 1024))
                   for C in (256, 4096, 65536, 262144) if C * N * K <= 1.1e9]
        shapes += [(16384, 8, 512, 20), (65536, 8, 512, 20), (16384, 16, 1024, 20)]
    table = {}
    for C, K, N, L in shapes:
        key = '%d chains, K=%d, N=%d, L=%d' % (C, K, N, L)
        table[key] = measure(C, K, N, L, dev, args.rounds, args.window)
        table[key]['chains x N x K'] = float(C) * N * K
        print(key, json.dumps(table[key]), flush=True)
    line = json.dumps(table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
