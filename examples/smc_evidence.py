#!/usr/bin/env python3
"""
Log-evidence by tempered sequential Monte Carlo: ``TemperedSMC`` moves G populations of P
chains from draws of a normalised ``p_0`` to the target along ``log p_beta = log p_0 + beta
l``, choosing every next beta from the particles (``binf_amd/samplers/smc.py``,
``csrc/smc.hip``).  The product of the stage-wise mean weights is ``Z = integral p_0 exp(l)``
itself; the spread over populations is its standard error.

Two targets with a known answer:

  gaussian     prior N(0, 3^2 I_4), likelihood N(y = 2 1 | x, 0.5^2 I_4): the evidence is
               N(y | 0, (3^2 + 0.5^2) I_4), log Z = -8.98987
  double well  p_0 = N(0, 1.5^2) in one dimension, l(x) = -a (x^2 - 1)^2 - log p_0(x), so that
               Z = integral exp(-a (x^2 - 1)^2) dx: the quadrature of ``examples/free_energy.py``.
               Both wells are found because the prior covers both: no chain has to cross

  python examples/smc_evidence.py --populations 16 --particles 256
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from binf_amd.samplers.hmc import HMCSampler
from binf_amd.samplers.rng import DeviceRNG
from binf_amd.samplers.smc import TemperedSMC


def _sibling(name):
    """The example next to this one, by its path (whatever else is called ``name``)."""
    import importlib.util
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location('examples_' + name, os.path.join(here, name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


PRIOR_SD, NOISE_SD, Y, DIMS = 3.0, 0.5, 2.0, 4
DW_A, DW_PRIOR_SD = 16.0, 1.5


def gauss_logpdf(x, sd):
    return -0.5 * (x * x).sum(dim=1) / sd ** 2 - 0.5 * x.shape[1] * math.log(2.0 * math.pi * sd ** 2)


class TemperedGaussian(object):
    """log p_beta(x) = log N(x | 0, PRIOR_SD^2 I) + beta_c log N(Y 1 | x, NOISE_SD^2 I); ``beta``
    is the ``[C]`` device tensor the SMC writes."""

    def __init__(self, beta):
        self.beta = beta

    def log_likelihood(self, x):
        return gauss_logpdf(x - Y, NOISE_SD)

    def log_prob(self, x):
        return gauss_logpdf(x, PRIOR_SD) + self.beta * self.log_likelihood(x)

    def gradient(self, x):
        return x / PRIOR_SD ** 2 + self.beta[:, None] * (x - Y) / NOISE_SD ** 2

    def stiffness(self):
        return 1.0 / PRIOR_SD ** 2 + self.beta / NOISE_SD ** 2


class TemperedWell(object):
    """log p_beta(x) = (1 - beta_c) log N(x | 0, DW_PRIOR_SD^2) - beta_c a (x^2 - 1)^2.  No
    ``log_likelihood``: the SMC takes log_prob at beta = 1 minus log_prob at beta = 0."""

    def __init__(self, beta, a=DW_A):
        self.beta, self.a = beta, a

    def log_prob(self, x):
        w = x * x - 1.0
        return (1.0 - self.beta) * gauss_logpdf(x, DW_PRIOR_SD) - self.beta * self.a * (w * w).sum(dim=1)

    def gradient(self, x):
        b = self.beta[:, None]
        return (1.0 - b) * x / DW_PRIOR_SD ** 2 + b * (4.0 * self.a) * x * (x * x - 1.0)

    def stiffness(self):
        return (1.0 - self.beta) / DW_PRIOR_SD ** 2 + self.beta * 8.0 * self.a       # the wells' curvature


def run(make_pdf, dims, prior_sd, G, P, seed, dev, explicit):
    rng = DeviceRNG(seed, dev)
    beta = torch.zeros(G * P, dtype=torch.float64, device=dev)
    pdf = make_pdf(beta)
    start = rng.normal((G * P, dims), dev) * prior_sd            # draws of the normalised p_0
    inner = HMCSampler(pdf, start, 0.1, 8, variable_name='x', rng=rng)

    def set_timestep(smc):
        # a colder stage is stiffer: the step follows beta, on the device
        smc.sampler.timestep = 0.5 / torch.sqrt(pdf.stiffness())
    smc = TemperedSMC(inner, beta, n_populations=G, ess_fraction=0.5, n_mutations=2,
                      log_likelihood=pdf.log_likelihood if explicit else None,
                      before_mutation=set_timestep)
    return smc, smc.run()


def main(populations=16, particles=256, seed=0, quiet=False):
    dev = torch.device('cuda', torch.cuda.current_device())
    out = {}
    var = PRIOR_SD ** 2 + NOISE_SD ** 2
    exact = DIMS * (-0.5 * Y * Y / var - 0.5 * math.log(2.0 * math.pi * var))
    smc, r = run(TemperedGaussian, DIMS, PRIOR_SD, populations, particles, seed, dev, True)
    out['gaussian'] = (r, exact)
    if not quiet:
        print('conjugate Gaussian, analytic log Z = %.5f' % exact)
        print(r)
        print('ladder of population 0: %s\n' % ' '.join('%.4g' % b for b in r.betas[:, 0].tolist()))
    exact = _sibling('free_energy').double_well_log_z(1.0, DW_A)
    smc, r = run(TemperedWell, 1, DW_PRIOR_SD, populations, particles, seed + 1, dev, False)
    out['double_well'] = (r, exact)
    if not quiet:
        print('double well, a = %g, quadrature log Z = %.5f' % (DW_A, exact))
        print(r)
        print('fraction in the left well: %.3f (target 0.5)' % float((smc.state < 0).double().mean()))
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--populations', type=int, default=16)
    ap.add_argument('--particles', type=int, default=256)
    ap.add_argument('--seed', type=int, default=0)
    a = ap.parse_args()
    main(a.populations, a.particles, a.seed)
