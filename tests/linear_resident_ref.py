"""numpy restatement and derived bounds for the chain-resident kernels of a linear
forward model (tests/test_gpu_linear_resident.py).

The restatement is the reference path written out for one chain: ``mock = theta . A``
(binf/model/forwardmodels.py:23-28), the Gaussian error model's log-prob
(binf/pdf/likelihoods.py:141-146), the posterior's components added in their order
(binf/pdf/posteriors.py:147-151), the leapfrog of binf/samplers/hmc.py:116-123.

Bounds (no flat tolerance):
  trajectory   tests/poly_bounds.PolyBound.transition on the design matrix (every force
               evaluation within 1e-10 of its sum-of-magnitudes scale, propagated through
               the exact linear leapfrog map);
  energies     evaluation error only: tests/linear_bounds.logp_float's bound for the
               likelihood term (a K-term dot product per datum, squared residuals summed
               over N) plus 16 U times the magnitudes of the remaining terms (a handful of
               roundings each, generously); E_after additionally carries the propagated
               ``be_after``.

These bounds are what can be said against the REFERENCE, whose BLAS order is not reproducible.
Against the kernels' own arithmetic contract the stronger statement holds: tests/chain_contract.py
restates it on the host and tests/test_gpu_chain_contract.py compares bit for bit."""
import numpy as np

import linear_bounds as LB
import poly_bounds as PB

U = PB.U


def stable_dt(A, tau_max, safety=0.45):
    """A leapfrog step inside the stability limit 2 / sqrt(lambda_max(tau A A^T))."""
    lam = np.linalg.eigvalsh(A.dot(A.T)).max() * float(tau_max)
    return safety * 2.0 / np.sqrt(max(lam, 1e-300))


class Case(object):
    """One posterior: design matrix, data, optional Gaussian prior N(0, var) on theta
    (energy only), its place relative to the likelihood, and per-chain constants added
    first / last."""

    def __init__(self, A, ys, var=None, prior_first=True):
        self.A, self.ys = np.asarray(A, dtype=np.float64), np.asarray(ys, dtype=np.float64)
        self.K, self.N = self.A.shape
        self.var, self.prior_first = var, prior_first
        pb = object.__new__(PB.PolyBound)
        pb.J, pb.aJ, pb.y = self.A, np.abs(self.A), self.ys
        pb.K, pb.N = self.K, self.N
        pb.mu = None if var is None else np.zeros(self.K)
        pb.var = None if var is None else np.full(self.K, float(var))
        pb.JJt = self.A.dot(self.A.T)
        self.pb = pb

    def terms(self, theta, tau, pre=None, post=None):
        """The log-prob terms in summation order."""
        chi2 = np.sum((theta.dot(self.A) - self.ys) ** 2)
        lik = -0.5 * chi2 * tau + self.N * 0.5 * np.log(tau)
        out = [] if pre is None else [pre]
        pri = None if self.var is None else -0.5 * np.sum((theta - 0.0) ** 2 / self.var)
        if pri is not None and self.prior_first:
            out.append(pri)
        out.append(lik)
        if pri is not None and not self.prior_first:
            out.append(pri)
        if post is not None:
            out.append(post)
        return out, lik

    def energy(self, theta, p, tau, pre=None, post=None):
        """``(E, evaluation bound)`` of hmc.py:148 / :150 at ``(theta, p)``."""
        terms, lik = self.terms(theta, tau, pre, post)
        lp = terms[0]
        for t in terms[1:]:
            lp = lp + t
        kin = 0.5 * np.sum(p ** 2)
        _, lb = LB.logp_float(theta[None, :], self.A, self.ys, tau)
        rest = sum(abs(t) for t in terms) - abs(lik) + kin
        return -lp + kin, float(lb[0]) + 16 * U * rest

    def transition(self, theta, p0, tau, dt, L, pre=None, post=None):
        """The numpy transition of one chain and its bounds: dict(q, p, bq, e_before,
        e_after, b_before, b_after, dE)."""
        b = self.pb.transition(theta, p0, tau, dt, L)
        e0, v0 = self.energy(theta, p0, tau, pre, post)
        e1, v1 = self.energy(b['q'], b['p'], tau, pre, post)
        return dict(q=b['q'], p=b['p'], bq=b['bq'] + 4 * U * np.abs(b['q']), e_before=e0, e_after=e1,
                    b_before=v0, b_after=v1 + b['be_after'], dE=e1 - e0)


def accept_numpy(dE, u):
    """hmc.py:151 with csb's clipped exp."""
    return u < np.exp(np.clip(-dE, -308.0, 709.0))


def decided(dE, u, B):
    """Is the accept test further from a tie than the energies' error?"""
    with np.errstate(divide='ignore'):
        return np.abs(-dE - np.log(u)) > B
