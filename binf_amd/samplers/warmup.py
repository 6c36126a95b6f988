"""
Windowed warm-up adaption of a diagonal HMC metric, on the device.

Not in the reference, whose sampler integrates with the identity mass
(``binf/samplers/hmc.py:92-125``): where the posterior's dimensions have different scales
the narrowest one limits the step size and the widest moves a few percent of its width per
transition.  ``HMCSampler(metric=scale)`` integrates with M = diag(1 / scale^2);
:class:`WindowedWarmup` learns ``scale`` while the chains warm up:

* the schedule is Stan's (:func:`window_schedule`): a fast phase (``init_buffer``), slow
  windows that double from ``base_window``, a fast phase (``term_buffer``);
* inside a slow window every transition's new state goes through
  ``binf_metric_accumulate_f64`` -- three running moments per chain and dimension, no record
  of warm-up draws is ever kept;
* at a window's last transition ``binf_metric_pool_f64`` pools the chains of each group into
  a variance (between-chain spread included, Stan's shrinkage towards 1e-3 if
  ``regularise``) and writes its square root INTO the sampler's scale buffer: the address
  stays, a captured graph goes on replaying;
* step sizes adapt over the whole warm-up by the sampler's own in-kernel multiplicative rule
  (``timestep_adaption_limit`` is raised to cover it).  A chain's step settles where
  ``up^a * down^(1-a) = 1``, i.e. at the acceptance rate
  ``a = ln(1/down) / (ln up + ln(1/down))``: 0.51 at the default 1.05 / 0.95, 0.84 at
  1.02 / 0.9.

No host read-back anywhere; everything is stream-ordered.  Sharded runs: at a window's end
the moments are all-gathered (``dist.gather_chains``) and every rank pools ALL chains in
global order, so every rank holds the scale of the one-GPU run bit for bit -- one
collective per window (about five per run), none in the transitions.  With more than one
group shard by whole groups (``dist.shard_ladders``).

``dense=True`` learns a DENSE metric on the same schedule, for posteriors whose dimensions are
correlated (a diagonal metric then learns marginal widths that are all alike):
``HMCSampler(dense_metric=chol)`` integrates with M^-1 = L L^T, inside a window every
transition's new state goes through ``binf_metric_comoments_f64`` (pooled co-moments per group,
``[G x D x D]``: nothing per chain), and at a window's end ``binf_metric_factor_f64`` pools the
covariance (Stan's shrinkage if ``regularise``) and writes its Cholesky factor INTO the
sampler's ``metric_chol``; a group whose covariance has no factor keeps the one it had and is
flagged in ``status`` (a device tensor, never read back here).  One GPU only: per-group sums
cannot reproduce the one-GPU bits after an all-reduce (a FIXED dense metric is chain-local and
works on shards as it is).
"""
import torch

from binf_amd import _native, dist


def window_schedule(n_warmup, init_buffer=75, term_buffer=50, base_window=25):
    """Stan's slow windows as ``[(start, stop), ...]`` (transition indices, stop exclusive).
    If ``n_warmup < init + term + base``: ``init = floor(0.15 n)``, ``term = floor(0.1 n)``,
    ``base = n - init - term``.  Each window is twice its predecessor; the one after which
    another doubled window would overrun ``n - term`` is stretched to ``n - term``.
    n = 1000: [75, 100), [100, 150), [150, 250), [250, 450), [450, 950)."""
    n, init, term, base = int(n_warmup), int(init_buffer), int(term_buffer), int(base_window)
    if n < 0 or init < 0 or term < 0 or base < 1:
        raise ValueError('window_schedule: n_warmup, init_buffer, term_buffer >= 0 and base_window >= 1 required')
    if n < init + term + base:
        init, term = int(0.15 * n), int(0.1 * n)
        base = n - init - term
    if base < 1:
        return []
    last = n - term - 1                       # the last slow transition
    out, start, size, nxt = [], init, base, init + base - 1
    while True:
        out.append((start, nxt + 1))
        if nxt == last:
            return out
        start, size = nxt + 1, 2 * size
        nxt = nxt + size
        if nxt != last and nxt + 2 * size >= n - term:
            nxt = last


def _hmc_of(sampler):
    """The sampler that carries the metric: ``sampler`` itself, or the inner sampler of a
    ``ReplicaExchangeSampler``; and the default number of groups (1, or R)."""
    inner = getattr(sampler, 'sampler', None)
    if inner is not None and hasattr(sampler, 'n_replicas'):
        return inner, int(sampler.n_replicas)
    return sampler, 1


class WindowedWarmup(object):
    """Drives ``n_warmup`` transitions of ``sampler`` and adapts its diagonal metric.

      sampler      an ``HMCSampler`` (it gets ``set_metric``) or a ``ReplicaExchangeSampler``
                   around one (the inner sampler gets the metric, one row per ladder slot)
      groups       G, rows of the scale: chain ``c`` belongs to group ``c % G``; default 1, or
                   R for a ``ReplicaExchangeSampler``
      regularise   Stan's shrinkage of the pooled variance
      advance      what one transition is; default ``sampler.sample``.  A Gibbs loop passes
                   ``gibbs.sample`` and its HMC subsampler as ``sampler``
      group        the process group of a sharded run (``None``: the default group)
      dense        learn a dense metric (the sampler gets ``set_dense_metric``; the start is the
                   factor it carries, or the identity); ``status`` (int32 ``[G]``, on the device)
                   says which groups kept their previous factor at the last window's end

    ``step()`` is one transition, ``run()`` the rest of the warm-up; ``state_dict()`` /
    ``load_state_dict()`` let a checkpoint continue bit for bit.  A metric the sampler
    already carries is the starting point (it must have ``groups`` rows); otherwise ones."""

    def __init__(self, sampler, n_warmup, init_buffer=75, term_buffer=50, base_window=25,
                 groups=None, regularise=True, advance=None, group=None, dense=False):
        hmc, default_groups = _hmc_of(sampler)
        if not hasattr(hmc, 'set_metric'):
            raise TypeError('WindowedWarmup needs a sampler with set_metric (an HMCSampler), got %r'
                            % type(hmc).__name__)
        self.dense = bool(dense)
        if self.dense and not hasattr(hmc, 'set_dense_metric'):
            raise TypeError('WindowedWarmup(dense=True) needs a sampler with set_dense_metric, got %r'
                            % type(hmc).__name__)
        if self.dense and dist.world()[1] > 1:
            raise NotImplementedError('WindowedWarmup(dense=True): the dense warm-up runs on one GPU (per-group '
                                      'co-moments cannot be all-reduced to the one-GPU bits); a FIXED '
                                      'dense_metric works on shards as it is')
        self.sampler, self.hmc = sampler, hmc
        self.n_warmup = int(n_warmup)
        self.windows = window_schedule(n_warmup, init_buffer, term_buffer, base_window)
        self.regularise = bool(regularise)
        self.advance = advance if advance is not None else sampler.sample
        self.group = group
        state = hmc.state
        if not isinstance(state, torch.Tensor) or not state.is_cuda or state.dtype != torch.float64:
            raise ValueError('WindowedWarmup: the sampler state must be an fp64 ROCm tensor')
        q = state if state.dim() == 2 else state.reshape(1, -1)
        C, D = q.shape
        carried = hmc.metric_chol if self.dense else hmc.metric_scale
        G = int(groups) if groups is not None else \
            (carried.shape[0] if carried is not None else default_groups)
        if G < 1 or C % G != 0:
            raise ValueError('WindowedWarmup: %d groups do not divide the %d chains' % (G, C))
        if self.dense:
            if hmc.metric_chol is None:
                hmc.set_dense_metric(torch.eye(D, dtype=torch.float64, device=q.device).repeat(G, 1, 1))
            elif hmc.metric_chol.shape[0] != G:
                raise ValueError('WindowedWarmup: the sampler\'s dense metric has %d factors, groups = %d'
                                 % (hmc.metric_chol.shape[0], G))
        elif hmc.metric_scale is None:
            hmc.set_metric(torch.ones((G, D), dtype=torch.float64, device=q.device))
        elif hmc.metric_scale.shape[0] != G:
            raise ValueError('WindowedWarmup: the sampler\'s metric has %d rows, groups = %d'
                             % (hmc.metric_scale.shape[0], G))
        self.groups = G
        if hmc.timestep_adaption_limit < hmc.counter + self.n_warmup + 1:
            hmc.timestep_adaption_limit = hmc.counter + self.n_warmup + 1
        self.t = 0                                # transitions made
        self.n_window = 0                         # draws accumulated in the open window
        z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=q.device)
        if self.dense:
            # pooled per group: [G x D], [G x D], [G x D x D] -- nothing per chain
            self.n_chains = C
            self._k0, self._s1, self._s2, self._work = z(G, D), z(G, D), z(G, D, D), z(G, D, D)
            # 0: the last window's factor was taken; 1: the group kept its previous one
            self.status = torch.zeros(G, dtype=torch.int32, device=q.device)
        else:
            self._k0, self._s1, self._s2 = z(C, D), z(C, D), z(C, D)

    @property
    def done(self):
        return self.t >= self.n_warmup

    def _window(self, t):
        for w in self.windows:
            if w[0] <= t < w[1]:
                return w
        return None

    def step(self):
        """One warm-up transition; returns what ``advance()`` returned."""
        if self.done:
            raise RuntimeError('WindowedWarmup: all %d warm-up transitions are made' % self.n_warmup)
        out = self.advance()
        w = self._window(self.t)
        if w is not None:
            x = self.hmc.state
            x = (x if x.dim() == 2 else x.reshape(1, -1)).contiguous()
            accumulate = _native.metric_comoments if self.dense else _native.metric_accumulate
            accumulate(x, self._k0, self._s1, self._s2, first=self.t == w[0])
            self.n_window = 1 if self.t == w[0] else self.n_window + 1
            if self.t == w[1] - 1:
                self._pool()
                self.n_window = 0
        self.t += 1
        return out

    def run(self):
        """The remaining warm-up transitions; returns the sampler."""
        while not self.done:
            self.step()
        return self.sampler

    def _pool(self):
        restart = getattr(self.hmc, 'restart_step_adaption', None)
        if restart is not None:
            restart()                     # a sampler with dual-averaged steps: a new metric, a new average
        if self.dense:
            _native.metric_factor(self._s1, self._s2, self.n_window, self.n_chains, self.hmc.metric_chol,
                                  self._work, self.status, self.regularise)
            return
        k0, s1, s2 = self._k0, self._s1, self._s2
        _, ws = dist.world()
        if ws > 1:
            # every rank pools all chains in global order: the one-GPU scale, bit for bit
            every = dist.gather_chains(torch.stack((k0, s1, s2), dim=1), group=self.group)
            k0, s1, s2 = (every[:, j].contiguous() for j in range(3))
        _native.metric_pool(k0, s1, s2, self.n_window, self.hmc.metric_scale, self.regularise)

    # -- checkpoint / resume (binf_amd/checkpoint.py) ----------------------------------
    def state_dict(self):
        d = {'t': int(self.t), 'n_window': int(self.n_window), 'n_warmup': int(self.n_warmup),
             'windows': [list(w) for w in self.windows], 'k0': self._k0, 's1': self._s1, 's2': self._s2}
        if self.dense:
            d['dense'], d['status'] = True, self.status
        return d

    def load_state_dict(self, d):
        if int(d['n_warmup']) != self.n_warmup or [list(w) for w in self.windows] != [list(w) for w in d['windows']]:
            raise ValueError('WindowedWarmup: the checkpoint belongs to another schedule')
        if bool(d.get('dense', False)) != self.dense:
            raise ValueError('WindowedWarmup: the checkpoint belongs to a %s warm-up'
                             % ('dense' if d.get('dense') else 'diagonal'))
        if self.dense:
            self.status.copy_(d['status'].to(device=self.status.device, dtype=self.status.dtype))
        self.t, self.n_window = int(d['t']), int(d['n_window'])
        for mine, name in ((self._k0, 'k0'), (self._s1, 's1'), (self._s2, 's2')):
            mine.copy_(d[name].to(device=mine.device, dtype=mine.dtype))


def warmup(sampler, n_warmup, **kw):
    """``WindowedWarmup(sampler, n_warmup, **kw).run()``; returns the driver (its sampler now
    carries the adapted metric and step sizes)."""
    w = WindowedWarmup(sampler, n_warmup, **kw)
    w.run()
    return w
