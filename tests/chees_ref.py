"""Host restatement (numpy) of the ChEES criterion kernels of ``csrc/chees.hip`` and of the
``ChEESSampler`` loop, written from the contract in ``include/binf_hip.h`` -- not from the
kernels.  Nothing here calls into the library.

Every multiply and add is one numpy operation on float64.  Row sums are ``np.sum`` of a
contiguous row (numpy's pairwise order); sums over chains take the contract's orders: chunks of
``CHUNK`` chains from chain 0, a chunk's column sums chain by chain from 0.0 (means), a chunk's
64 terms joined by the balanced tree over neighbours (sums), chunks added in ascending order from
0.0.  ``expc(x) = np.exp(np.clip(x, -308, 709))`` is numpy's exponential, which may differ from
the device's by an ulp.

The sampler loop's scalar logic is NOT restated: it is ``binf_amd.samplers.chees.TrajectoryAdaption``
itself, plain Python floats that run the same on every host.  The leapfrog is ``metric_ref`` /
``dense_metric_ref``'s (the identity: the reference's own lines, ``oracle/ref_numpy.py``).
"""
import numpy as np

f64 = np.float64
CHUNK = 64


def expc(x):
    with np.errstate(all='ignore'):
        return np.exp(np.clip(x, -308.0, 709.0))


def rowsum(x):
    with np.errstate(all='ignore'):
        return np.sum(np.ascontiguousarray(x), axis=1)


def accept_prob(e_before, e_after):
    """min(1, expc(e_before - e_after)); +0.0 where e_after is not finite or the difference is NaN."""
    with np.errstate(all='ignore'):
        x = e_before - e_after
        ok = np.isfinite(e_after) & ~np.isnan(x)
        return np.where(ok, np.minimum(f64(1.0), expc(np.where(ok, x, 0.0))), f64(0.0))


def _chunked(x):
    """x [C, ...] as [chunks, CHUNK, ...], the last chunk filled with +0.0 (adding +0.0 to a sum
    that started at +0.0 changes no bit)."""
    C = x.shape[0]
    nch = (C + CHUNK - 1) // CHUNK
    pad = np.zeros((nch * CHUNK,) + x.shape[1:], dtype=f64)
    pad[:C] = x
    return pad.reshape((nch, CHUNK) + x.shape[1:])


def column_mean(x):
    """Chunk partials chain by chain from 0.0, partials in ascending order from 0.0, one division."""
    C = x.shape[0]
    ch = _chunked(x)
    with np.errstate(all='ignore'):
        part = np.zeros((ch.shape[0],) + x.shape[1:], dtype=f64)
        for i in range(CHUNK):
            part = part + ch[:, i]
        tot = np.zeros(x.shape[1:], dtype=f64)
        for k in range(ch.shape[0]):
            tot = tot + part[k]
        return tot / f64(C)


def effective(q, q_prop, alpha):
    return np.where((alpha > 0.0)[:, None], q_prop, q)


def means(q, q_prop, alpha):
    return column_mean(q), column_mean(effective(q, q_prop, alpha))


def terms(q, q_prop, v, alpha, mean_q, mean_prop):
    moved = alpha > 0.0
    with np.errstate(all='ignore'):
        xp = effective(q, q_prop, alpha) - mean_prop
        xq = q - mean_q
        a, b = rowsum(xp * xp), rowsum(xq * xq)
        s = rowsum(xp * np.where(moved[:, None], v, 0.0))
        return np.where(moved, (a - b) * s, f64(0.0))


def tree_sum(t):
    """[chunks, 64] -> [chunks]: neighbours joined level by level."""
    with np.errstate(all='ignore'):
        while t.shape[1] > 1:
            t = t[:, 0::2] + t[:, 1::2]
    return t[:, 0]


def chain_sum(t):
    part = tree_sum(_chunked(t))
    tot = f64(0.0)
    with np.errstate(all='ignore'):
        for k in range(part.shape[0]):
            tot = tot + part[k]
    return tot


def sums(alpha, g):
    fin = np.isfinite(g)
    with np.errstate(all='ignore'):
        return np.array([chain_sum(np.where(fin, alpha * g, 0.0)), chain_sum(np.where(fin, alpha, 0.0)),
                         chain_sum(f64(1.0) / alpha), chain_sum(np.where(fin, 0.0, 1.0))], dtype=f64)


def criterion(q, q_prop, v, alpha):
    """(mean_q, mean_prop, g, out): the three launches after accept_prob."""
    mq, mp = means(q, q_prop, alpha)
    g = terms(q, q_prop, v, alpha, mq, mp)
    return mq, mp, g, sums(alpha, g)


# ---------------------------------------------------------------------------
# the sampler loop
# ---------------------------------------------------------------------------
class Integrator(object):
    """'identity', 'diag' (``param`` = scales ``[G x D]``) or 'dense' (lower factors ``[G x D x D]``),
    exact mode, a scalar step."""

    def __init__(self, kind='identity', param=None):
        self.kind, self.param = kind, param

    def leapfrog(self, q, p, grad, eps, nsteps):
        if self.kind == 'diag':
            import metric_ref as MR
            return MR.leapfrog(q, p, grad, self.param, eps, None, nsteps)
        if self.kind == 'dense':
            import dense_metric_ref as DM
            return DM.leapfrog(q, p, grad, self.param, eps, None, nsteps)
        eps = f64(eps)
        with np.errstate(all='ignore'):
            p = p - f64(0.5) * eps * grad(q)
            for _ in range(max(1, int(nsteps)) - 1):
                q = q + p * eps
                p = p - eps * grad(q)
            q = q + p * eps
            p = p - f64(0.5) * eps * grad(q)
        return q, p

    def velocity(self, p):
        """What the drift adds to a zeroed row at step 1.0; the momentum itself without a metric."""
        if self.kind == 'diag':
            import metric_ref as MR
            return MR.drift(np.zeros_like(p), p, self.param, 1.0)
        if self.kind == 'dense':
            import dense_metric_ref as DM
            return DM.drift(np.zeros_like(p), p, self.param, 1.0)
        return p


class ChEES(object):
    """``ChEESSampler`` restated: ``sample(p0, u)`` is one transition of every chain.  ``adaption``
    is a ``TrajectoryAdaption``.  Records of the last transition: ``alpha``, ``out``, ``g``, ``steps``,
    ``tau_over_eps`` (before the ceiling), ``accept_margin`` (min |u - alpha| over chains),
    ``cancellation`` (sum |alpha g| / |sum alpha g|)."""

    def __init__(self, logp, grad, q, adaption, integ=None, adaption_limit=0, jitter=True):
        self.logp, self.grad = logp, grad
        self.q = np.array(q, dtype=f64)
        self.ad = adaption
        self.integ = integ if integ is not None else Integrator()
        self.adaption_limit, self.jitter, self.counter = int(adaption_limit), bool(jitter), 0
        self.n_leapfrog_total = 0
        self.alpha = self.out = self.g = None
        self.min_accept_margin, self.max_cancellation, self.min_ceil_margin = np.inf, 0.0, np.inf

    def energy(self, q, p):
        with np.errstate(all='ignore'):
            return f64(0.5) * rowsum(p * p) - self.logp(q)

    def sample(self, p0, u):
        from binf_amd.samplers.chees import halton
        ad = self.ad
        adapting = self.counter + 1 < self.adaption_limit
        if not adapting and not ad.frozen:
            ad.freeze()
        if adapting or self.jitter:
            L = ad.begin()
            r = halton(ad.index) * ad.T / ad.eps
            if 0.5 <= r < ad.max_leapfrog_steps:        # (below 1/2 the count is 1 whatever an ulp does)
                self.min_ceil_margin = min(self.min_ceil_margin, abs(r - round(r)))
        else:
            L = ad.mean_steps()
        self.steps, eps = L, ad.eps
        q0 = self.q
        eb = self.energy(q0, p0)
        q1, p1 = self.integ.leapfrog(q0, p0, self.grad, eps, L)
        ea = self.energy(q1, p1)
        with np.errstate(all='ignore'):
            a = expc(-(ea - eb))
            acc = u < a
        self.min_accept_margin = min(self.min_accept_margin, float(np.nanmin(np.abs(u - a))))
        if adapting:
            self.alpha = accept_prob(eb, ea)
            self.mean_q, self.mean_prop, self.g, self.out = criterion(q0, q1, self.integ.velocity(p1), self.alpha)
            with np.errstate(all='ignore'):
                fin = np.isfinite(self.g)
                num = float(np.sum(np.abs(self.alpha * self.g)[fin]))
            if self.out[0] != 0.0:
                self.max_cancellation = max(self.max_cancellation, num / abs(float(self.out[0])))
            ad.update([float(x) for x in self.out], q0.shape[0], freeze=self.counter + 2 >= self.adaption_limit)
        self.q = np.where(acc[:, None], q1, q0)
        self.accepted = acc
        self.counter += 1
        self.n_leapfrog_total += L
        return self.q


def run_gaussian(sigma, C, n, seed, timestep, target_accept=0.651, max_leapfrog_steps=1000, **kw):
    """``n`` adapting transitions (the last one freezes) of C chains on N(0, diag sigma^2) from
    exact draws of the target; returns the frozen ``TrajectoryAdaption``."""
    from binf_amd.samplers.chees import TrajectoryAdaption
    sigma = np.asarray(sigma, dtype=f64)
    prec = f64(1.0) / (sigma * sigma)
    rs = np.random.RandomState(seed)
    q = sigma * rs.standard_normal((C, sigma.size))
    ad = TrajectoryAdaption(timestep, max_leapfrog_steps, target_accept, **kw)
    s = ChEES(lambda x: f64(-0.5) * rowsum(x * x * prec), lambda x: x * prec, q, ad, adaption_limit=n + 1)
    for _ in range(n):
        s.sample(rs.standard_normal(q.shape), rs.uniform(size=C))
    assert ad.frozen
    return ad
