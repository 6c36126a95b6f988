#!/usr/bin/env python3
"""Fused GLM kernels against the as-written path, on one GPU (DESIGN section 4.7's table).

For each shape (C, K, N) and both families: log-prob, gradient and a 20-step leapfrog, fused
(``binf_linear_glm_logp_f64`` / ``_grad_f64`` / ``_leapfrog_f64``) against as written
(``binf_linear_forward_f64``, ``binf_glm_pointwise_f64``, then ``binf_row_sum_f64`` or
``binf_jacobian_contract_f64``; the leapfrog through ``HMCSampler._leapfrog`` on a forward model
that overrides ``_evaluate``).  Device events around each call, 3 warm-up calls, ``--reps``
timed calls alternating the two paths, the median and the quartiles of each.  The Gaussian
gradient kernel (``binf_poly_gauss_grad_f64``) is timed at the same shape: the MFMA rate of
both is ``4 C K N`` flops over the median.  One JSON line per measurement.  ``--families``
chooses among ``binomial_logit poisson_log negbin_log``; the negative binomial's two paths are
timed as its hooks run them (``binf_linear_negbin_*``; the count term's launch included on both
sides, a per-chain ``log_dispersion`` fixed in the model).  ``--count`` times the count kernel alone.

    python scripts/glm_measure.py [--reps 21] [--families negbin_log] [--shapes 4096,8,1024 4096,33,16384 8192,64,16384]
    python scripts/glm_measure.py --count
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from binf_amd import _native
from binf_amd.model.glm import BinomialLogitErrorModel, NegBinomialLogErrorModel, PoissonLogErrorModel
from binf_amd.model.linear import LinearForwardModel
from binf_amd.pdf import IsotropicGaussian
from binf_amd.pdf.likelihoods import Likelihood
from binf_amd.pdf.posteriors import Posterior
from binf_amd.samplers.hmc import HMCSampler


class AsWritten(LinearForwardModel):
    """The same model, evaluated as written (an overridden ``_evaluate`` opts out of fusion)."""

    def _evaluate(self, **variables):
        return LinearForwardModel._evaluate(self, **variables)


def timed(fns, reps):
    """Median and quartiles [ms] of each callable, alternating them call by call."""
    for f in fns:
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times[i].append(a.elapsed_time(b))
    return [tuple(float(np.percentile(t, q)) for q in (50, 25, 75)) for t in times]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=21)
    ap.add_argument('--shapes', nargs='*', default=['4096,8,1024', '4096,33,16384', '8192,64,16384'])
    ap.add_argument('--families', nargs='*', default=['binomial_logit', 'poisson_log', 'negbin_log'])
    ap.add_argument('--count', action='store_true',
                    help='time binf_negbin_count_term_f64 (the chain sum) at ymax 64, 4096, 65536 x 4096 chains')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)
    if args.count:
        C = 4096
        lam = up(np.log(2.0) + 0.1 * np.random.RandomState(0).standard_normal(C))
        for ymax in (64, 4096, 65536):
            tail = up(np.arange(ymax, 0, -1, dtype=np.float64))
            r = timed([lambda: _native.negbin_count_term(lam, tail, -1.5)], args.reps)[0]
            print(json.dumps(dict(what='count_term', C=C, ymax=ymax, ms=r[0], q=r[1:])), flush=True)
        return
    for shape in args.shapes:
        C, K, N = (int(v) for v in shape.split(','))
        rs = np.random.RandomState(C + K + N)
        A = rs.standard_normal((K, N)) / np.sqrt(K)
        theta = rs.standard_normal((C, K))
        p0 = rs.standard_normal((C, K))
        trials = rs.randint(1, 21, size=N).astype(np.float64)
        offset = 0.1 * rs.standard_normal(N)
        for name in args.families:
            lam = None
            if name == 'binomial_logit':
                ys = np.floor(rs.uniform(size=N) * (trials + 1)).clip(0, trials)
                em = lambda: BinomialLogitErrorModel(ys, trials, offset)
            elif name == 'poisson_log':
                ys = rs.poisson(2.0, size=N).astype(np.float64)
                em = lambda: PoissonLogErrorModel(ys, offset)
            else:
                # counts with phi = 2; a per-chain lam around log 2, fixed in the model (as inside
                # a Gibbs conditional): the leapfrog hook is matched
                ys = rs.negative_binomial(2.0, 0.5, size=N).astype(np.float64)
                lam = up(np.log(2.0) + 0.1 * rs.standard_normal(C))

                def em():
                    m = NegBinomialLogErrorModel(ys, offset)
                    m.fix_variables(log_dispersion=lam)
                    return m
            e = em()
            dA, x = up(A), up(theta)
            dy, dm, do, dl = e.ys_device(dev), e.trials_device(dev), e.offset_device(dev), e.lconst_device(dev)
            fam = e.family

            if lam is None:
                logp_fused = lambda: _native.linear_glm_logp(x, dA, dy, dm, do, fam, e.log_norm)
                grad_fused = lambda: _native.linear_glm_grad(x, dA, dy, dm, do, fam)

                def logp_written():
                    ll, _ = _native.glm_pointwise(_native.linear_forward(x, dA), dy, dm, do, fam, dl)
                    return _native.row_sum(ll)

                def grad_written():
                    _, g = _native.glm_pointwise(_native.linear_forward(x, dA), dy, dm, do, fam, want_ll=False,
                                                 want_grad=True)
                    return _native.jacobian_contract(dA, g)
            else:
                # both paths as the hooks run them: the count term (chain sum / prefix) included
                logp_fused = lambda: _native.linear_negbin_logp(x, dA, dy, do, lam, e.log_norm_chain(lam))
                grad_fused = lambda: _native.linear_negbin_grad(x, dA, dy, do, lam)
                logp_written = lambda: _native.row_sum(e.pointwise_log_prob(_native.linear_forward(x, dA), lam))
                grad_written = lambda: _native.jacobian_contract(
                    dA, e._nb_pointwise(_native.linear_forward(x, dA), lam, False, True)[1])

            posts = []
            for cls in (LinearForwardModel, AsWritten):
                lik = Likelihood('outcomes', cls('covariates', A), em())
                posts.append(Posterior({'outcomes': lik}, {'prior': IsotropicGaussian(
                    1.0, 0.0, name='prior', variable_name='coefficients')}))
            samplers = [HMCSampler(p, x.clone(), 1e-4, 20, variable_name='coefficients') for p in posts]
            q, p = x.clone(), up(p0)

            def leap(s):
                def run():
                    q.copy_(x)
                    s._leapfrog(q, p, 1e-4, 20)
                return run

            gauss = lambda: _native.poly_gauss_grad(x, dA, dy, 1.0)
            res = {
                'logp': timed([logp_fused, logp_written], args.reps),
                'grad': timed([grad_fused, grad_written, gauss], args.reps),
                'leapfrog20': timed([leap(samplers[0]), leap(samplers[1])], args.reps),
            }
            flops = 4.0 * C * K * N
            for what, r in res.items():
                line = dict(family=name, C=C, K=K, N=N, what=what, fused_ms=r[0][0], fused_q=r[0][1:],
                            written_ms=r[1][0], written_q=r[1][1:], speedup=r[1][0] / r[0][0])
                if what == 'grad':
                    line.update(gauss_ms=r[2][0], gauss_q=r[2][1:], glm_tflops=flops / r[0][0] * 1e-9,
                                gauss_tflops=flops / r[2][0] * 1e-9)
                print(json.dumps(line), flush=True)
            del samplers, posts
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
