#!/usr/bin/env python3
"""
Free-energy differences from a tempered ladder: ``ReplicaExchangeSampler(...,
record_work=n)`` keeps the log-prob differences every swap round evaluates anyway, and
``free_energy()`` turns them into ``log Z_r - log Z_{r+1}`` of neighbouring slots by
Bennett's acceptance ratio (``binf_amd/free_energy.py``, ``csrc/free_energy.hip``).

Two targets with a known answer:

  harmonic     log p_r(x) = -1/2 k_r |x|^2, k = 1, 1/2, 1/4, 1/8, D = 8:
               log Z_r - log Z_{r+1} = (D / 2) ln(k_{r+1} / k_r)
  double well  the ladder of ``examples/replica_exchange.py`` in one dimension,
               log p_r(x) = -beta_r a (x^2 - 1)^2, against a quadrature of Z_beta

For both: BAR next to the two exponential averages (the draws of one slot of the pair
alone) and the overlap.  Where neighbours overlap well the three agree; where they do not
(the cold end of the double well) the one-sided averages drift apart, each dominated by a
few draws in the other slot's tail, and BAR, which weighs both sides, is the one to trust.

  python examples/free_energy.py --ladders 128 --rounds 400
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from binf_amd.samplers.hmc import HMCSampler
from binf_amd.samplers.replica import ReplicaExchangeSampler
from binf_amd.samplers.rng import DeviceRNG


def _sibling(name):
    """The example next to this one, by its path (whatever else is called ``name``)."""
    import importlib.util
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location('examples_' + name, os.path.join(here, name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TemperedDoubleWell = _sibling('replica_exchange').TemperedDoubleWell

HARMONIC_K = (1.0, 0.5, 0.25, 0.125)
HARMONIC_D = 8
DW_BETAS = (1.0, 0.5, 0.25, 0.12, 0.06, 0.03)
DW_A = 16.0


class Harmonic(object):
    """A torch PDF: log p_c(x) = -1/2 k_c sum x^2 (unnormalised: Z_c = (2 pi / k_c)^(D/2))."""

    def __init__(self, k):
        self.k = k

    def log_prob(self, x):
        return -0.5 * self.k * (x * x).sum(dim=1)

    def gradient(self, x):
        return self.k[:, None] * x


def double_well_log_z(beta, a=DW_A):
    """log of Z_beta = integral exp(-beta a (x^2 - 1)^2) dx, trapezoid rule on a grid far finer
    and wider than the integrand."""
    x = np.linspace(-6.0, 6.0, 1200001)
    f = np.exp(-beta * a * (x * x - 1.0) ** 2)
    return float(np.log(np.sum(0.5 * (f[1:] + f[:-1])) * (x[1] - x[0])))


def report(name, fe, exact, quiet):
    if quiet:
        return
    h = fe.cpu()
    print('%s' % name)
    print('%-6s %11s %11s %9s %11s %11s %8s' % ('pair', 'exact', 'BAR', 'stderr', 'forward', 'reverse', 'overlap'))
    for r, e in enumerate(exact):
        print('%-6s %11.5f %11.5f %9.2g %11.5f %11.5f %8.4f'
              % ('%d-%d' % (r, r + 1), e, float(h.delta[r]), float(h.stderr[r]), float(h.delta_forward[r]),
                 float(h.delta_reverse[r]), float(h.overlap[r])))
    print('%-6s %11.5f %11.5f %9.2g\n' % ('total', float(np.sum(exact)), float(h.total), float(h.total_stderr)))


def run(pdf, start, timestep, nsteps, R, rounds, burn_in, groups, seed, dev):
    rng = DeviceRNG(seed, dev)
    inner = HMCSampler(pdf, start, timestep, nsteps, variable_name='x', rng=rng)
    re = ReplicaExchangeSampler(inner, R, swap_interval=2, record_work=rounds)
    for _ in range(burn_in):
        re.sample()
    re.reset_work()                        # the record starts after burn-in
    for _ in range(rounds):
        re.sample()
    return re.free_energy(groups=groups)


def main(rounds=400, n_ladders=128, groups=16, seed=0, quiet=False):
    dev = torch.device('cuda', torch.cuda.current_device())
    out = {}
    R = len(HARMONIC_K)
    k = torch.tensor(HARMONIC_K, dtype=torch.float64, device=dev).repeat(n_ladders)
    start = DeviceRNG(seed + 1, dev).normal((R * n_ladders, HARMONIC_D), dev) / k.sqrt()[:, None]
    fe = run(Harmonic(k), start, 0.3 / k.sqrt(), 8, R, rounds, 0, groups, seed, dev)
    kk = np.asarray(HARMONIC_K)
    exact = 0.5 * HARMONIC_D * np.log(kk[1:] / kk[:-1])
    report('harmonic ladder, k = %s, D = %d' % (HARMONIC_K, HARMONIC_D), fe, exact, quiet)
    out['harmonic'] = (fe, exact)

    R = len(DW_BETAS)
    beta = torch.tensor(DW_BETAS, dtype=torch.float64, device=dev).repeat(n_ladders)
    start = torch.ones((R * n_ladders, 1), dtype=torch.float64, device=dev)
    fe = run(TemperedDoubleWell(DW_A, beta), start, 0.07, 8, R, rounds, rounds // 4, groups, seed, dev)
    logz = np.array([double_well_log_z(b) for b in DW_BETAS])
    exact = logz[:-1] - logz[1:]
    report('double well, a = %g, beta = %s' % (DW_A, DW_BETAS), fe, exact, quiet)
    out['double_well'] = (fe, exact)
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--ladders', type=int, default=128)
    ap.add_argument('--rounds', type=int, default=400)
    ap.add_argument('--groups', type=int, default=16)
    ap.add_argument('--seed', type=int, default=0)
    a = ap.parse_args()
    main(a.rounds, a.ladders, a.groups, a.seed)
