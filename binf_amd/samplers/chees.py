"""
ChEES-HMC (Hoffman, Radul & Sountsov 2021): fixed-length HMC whose trajectory length is learnt
during warm-up from ALL chains at once, so that every chain takes the same number of leapfrog
steps per transition and everything built for a fixed ``nsteps`` -- the whole-transition
kernels, the kernels that draw for themselves, ``sample_n`` in one launch, sharding -- applies
once the warm-up is over.

While adapting, a transition is the per-step tier's (scalar step, ``nsteps = L_t``) followed by
the four criterion launches of ``csrc/chees.hip`` and ONE 32-byte read-back; the scalar logic
that turns those four sums into the next step size, trajectory length and step count is
:class:`TrajectoryAdaption`, plain Python floats.  After the freeze the sampler is an
:class:`HMCSampler` whose ``nsteps`` is set from the host before every call.

There is no CPU path for the sampler: without the HIP library it raises.
"""
import math

import torch

from binf_amd import _native, dist
from binf_amd.samplers.hmc import HMCSampler, _MODES, _as2d, _device_state


def halton(t):
    """The base-2 van der Corput value of ``t`` = 1, 2, ...: 1/2, 1/4, 3/4, 1/8, ... (exact)."""
    t, h, f = int(t), 0.0, 0.5
    while t > 0:
        if t & 1:
            h += f
        t >>= 1
        f *= 0.5
    return h


class TrajectoryAdaption(object):
    """The scalars of ChEES-HMC, on the host: the shared step size ``eps``, the trajectory length
    ``T``, the jitter index.  ``begin()`` opens transition t = 1, 2, ... and returns its step
    count; ``update(sums, n_chains, freeze)`` closes an ADAPTING transition with the four sums of
    ``binf_chees_sums_f64``.

      jitter       h_t = halton(t); tau_t = h_t T; L_t = min(max_leapfrog_steps, max(1, ceil(tau_t / eps)))
      length       if sums[1] > 0 and sums[0] is finite: g = (L_t eps) sums[0] / sums[1] (L_t eps is
                   the time integrated), Adam ascent on log T with beta1 = 0:
                   m2 = beta2 m2 + (1 - beta2) g^2; log T += lr g / (sqrt(m2 / (1 - beta2^n)) + 1e-8),
                   n the updates made; otherwise T keeps its value
      step size    unless ``target_accept`` is None: dual averaging (Hoffman & Gelman 2014) of
                   log eps towards ``target_accept``; the statistic is the harmonic mean of the
                   acceptance probabilities, n_chains / sums[2] (0 if any is 0); mu = log(10 eps)
                   at every (re)start
      clip         T into [eps, max_leapfrog_steps eps]
      average      a = decay a + (1 - decay) log T, read as a / (1 - decay^k)
      freeze       T = exp(the average), eps = exp(the dual average): host floats from then on
    """

    def __init__(self, timestep, max_leapfrog_steps=1000, target_accept=0.651, learning_rate=0.025,
                 beta2=0.95, averaging_decay=0.9, gamma=0.05, t0=10.0, kappa=0.75):
        eps = float(timestep)
        if not (eps > 0.0 and math.isfinite(eps)):
            raise ValueError('timestep must be a positive number, not %r' % (timestep,))
        if int(max_leapfrog_steps) < 1:
            raise ValueError('max_leapfrog_steps must be >= 1')
        if target_accept is not None and not 0.0 < float(target_accept) < 1.0:
            raise ValueError('target_accept must lie in (0, 1), or be None (a fixed step size)')
        if not 0.0 <= float(beta2) < 1.0 or not 0.0 <= float(averaging_decay) < 1.0:
            raise ValueError('beta2 and averaging_decay must lie in [0, 1)')
        self.max_leapfrog_steps = int(max_leapfrog_steps)
        self.target_accept = None if target_accept is None else float(target_accept)
        self.learning_rate, self.beta2 = float(learning_rate), float(beta2)
        self.averaging_decay = float(averaging_decay)
        self.gamma, self.t0, self.kappa = float(gamma), float(t0), float(kappa)
        self.eps = eps
        self.log_T = math.log(eps)                  # T0 = eps0
        self.index = 0                              # the Halton index of the last transition begun
        self.last_steps = 0
        self.m2, self.n_updates = 0.0, 0            # Adam's second moment, updates made
        self.avg, self.n_avg = 0.0, 0               # running average of log T
        self.frozen = False
        self.n_skipped = 0                          # transitions whose sums moved T nowhere
        self.restart_step_adaption()

    # (keys of state_dict: every attribute the arithmetic reads)
    _FLOATS = ('eps', 'log_T', 'm2', 'avg', 'mu', 'hbar', 'logeps', 'logeps_bar')
    _INTS = ('index', 'last_steps', 'n_updates', 'n_avg', 'da_t', 'n_skipped')

    @property
    def T(self):
        return math.exp(self.log_T)

    def restart_step_adaption(self):
        """Start the dual averaging over around ten times the current step; T, its Adam moment
        and its average carry on."""
        self.mu = math.log(10.0 * self.eps)
        self.hbar, self.logeps, self.logeps_bar, self.da_t = 0.0, math.log(self.eps), 0.0, 0

    def steps_for(self, h):
        """L for a jitter value h: min(max, max(1, ceil(h T / eps)))."""
        tau = h * self.T
        return min(self.max_leapfrog_steps, max(1, int(math.ceil(tau / self.eps))))

    def mean_steps(self):
        """The constant step count of a run without jitter: max(1, ceil(T / (2 eps)))."""
        return self.steps_for(0.5)

    def begin(self):
        """Open the next transition: advance the jitter index, return L_t."""
        self.index += 1
        self.last_steps = self.steps_for(halton(self.index))
        return self.last_steps

    def _clip(self):
        lo = math.log(self.eps)
        hi = math.log(self.max_leapfrog_steps * self.eps)
        self.log_T = min(max(self.log_T, lo), hi)

    def update(self, sums, n_chains, freeze=False):
        """Close an adapting transition begun with ``begin()``: ``sums`` = ``out[0..3]`` of
        ``binf_chees_sums_f64`` as floats, ``n_chains`` = C.  ``freeze``: this was the last one."""
        if self.frozen:
            raise RuntimeError('TrajectoryAdaption: frozen')
        s_ag, s_a, s_inv = float(sums[0]), float(sums[1]), float(sums[2])
        g = (self.last_steps * self.eps) * s_ag / s_a if (s_a > 0.0 and math.isfinite(s_ag)) else float('nan')
        m2 = self.beta2 * self.m2 + (1.0 - self.beta2) * (g * g)
        if math.isfinite(g) and math.isfinite(m2):
            self.n_updates += 1
            self.m2 = m2
            scale = math.sqrt(m2 / (1.0 - self.beta2 ** self.n_updates)) + 1e-8
            self.log_T = self.log_T + self.learning_rate * g / scale
        else:                                       # no accepted mass, or an overflow: T stays
            self.n_skipped += 1
        if self.target_accept is not None:
            stat = float(n_chains) / s_inv if s_inv > 0.0 else 0.0     # harmonic mean; 0 at +inf
            if not math.isfinite(stat):
                stat = 0.0
            self.da_t += 1
            t = float(self.da_t)
            w1, k1, eta = 1.0 / (t + self.t0), math.sqrt(t) / self.gamma, t ** -self.kappa
            self.hbar = (1.0 - w1) * self.hbar + w1 * (self.target_accept - stat)
            self.logeps = self.mu - k1 * self.hbar
            self.logeps_bar = eta * self.logeps + (1.0 - eta) * self.logeps_bar
            self.eps = math.exp(self.logeps)
        self._clip()
        self.avg = self.averaging_decay * self.avg + (1.0 - self.averaging_decay) * self.log_T
        self.n_avg += 1
        if freeze:
            self.freeze()

    def freeze(self):
        """T = exp(the averaged log T), eps = exp(the dual average); nothing moves afterwards."""
        if self.frozen:
            return
        if self.target_accept is not None and self.da_t > 0:
            self.eps = math.exp(self.logeps_bar)
        if self.n_avg > 0:
            self.log_T = self.avg / (1.0 - self.averaging_decay ** self.n_avg)
        self._clip()
        self.frozen = True

    def state_dict(self):
        d = {k: float(getattr(self, k)) for k in self._FLOATS}
        d.update({k: int(getattr(self, k)) for k in self._INTS})
        d['frozen'] = bool(self.frozen)
        return d

    def load_state_dict(self, d):
        for k in self._FLOATS:
            setattr(self, k, float(d[k]))
        for k in self._INTS:
            setattr(self, k, int(d[k]))
        self.frozen = bool(d['frozen'])


class ChEESSampler(HMCSampler):
    """``ChEESSampler(pdf, state, timestep, max_leapfrog_steps=1000, target_accept=0.651,
    timestep_adaption_limit=0, jitter=True, ...)``: HMC with one step size and one trajectory
    length for all chains, both learnt while ``counter + 1 < timestep_adaption_limit`` (the last
    such transition freezes them; ``WindowedWarmup`` raises the limit to cover its warm-up and
    restarts the step averaging whenever it changes the metric).

    An adapting transition runs on the per-step tier with the scalar step ``timestep`` and
    ``nsteps = L_t``, then ``binf_chees_accept_prob_f64``, ``_means_``, ``_terms_`` and ``_sums_``
    on the trajectory's ends (the velocity is the end momentum, through the sampler's own drift
    launch where there is a metric: one criterion kernel serves all three) and one 32-byte
    read-back -- the only host synchronisation.  All chains form ONE group: adapting on a shard of
    a distributed run is refused, and so is an adapting sampler inside a
    ``ReplicaExchangeSampler``.

    A frozen sampler sets ``nsteps`` (``jitter=True``: the Halton sequence goes on, ``L_t =
    ceil(h_t T / eps)``; ``jitter=False``: the constant ``ceil(T / (2 eps))``) and calls
    ``HMCSampler.sample`` unchanged.  Graph replay of a learnt configuration:
    ``HMCSampler(pdf, state, s.timestep, s.mean_leapfrog_steps, graph=True)``.

    Attributes: ``trajectory_length`` (T), ``timestep`` (eps, a float), ``adapting``,
    ``last_n_leapfrog``, ``last_accept_prob`` (``[C]``, of the last ADAPTING transition),
    ``n_leapfrog_total``, ``mean_leapfrog_steps`` (``ceil(T / (2 eps))``, an int), ``adaption``
    (the :class:`TrajectoryAdaption`).

    Not supported (refused): ``graph`` other than False, ``nsteps``, rows beyond 8192 elements
    while adapting."""

    pools_chains_to_adapt = True          # (ReplicaExchangeSampler refuses it while adapting)

    def __init__(self, pdf, state, timestep, max_leapfrog_steps=1000, target_accept=0.651,
                 timestep_adaption_limit=0, jitter=True, variable_name=None, rng=None, mode='exact',
                 metric=None, dense_metric=None, learning_rate=0.025, beta2=0.95, averaging_decay=0.9,
                 gamma=0.05, t0=10.0, kappa=0.75, **refused):
        if refused.get('graph', False) is not False:
            raise ValueError('ChEESSampler: graph replay is not supported (graph must be False); replay a learnt '
                             'configuration with HMCSampler(pdf, state, s.timestep, s.mean_leapfrog_steps, graph=True)')
        refused.pop('graph', None)
        if 'nsteps' in refused:
            raise ValueError('ChEESSampler takes no nsteps: the trajectory length is learnt '
                             '(max_leapfrog_steps bounds it)')
        if refused:
            raise TypeError('ChEESSampler: unexpected arguments %s' % sorted(refused))
        if isinstance(timestep, torch.Tensor) and timestep.dim() > 0:
            raise ValueError('ChEESSampler: one step size for all chains (timestep must be a number)')
        self.adaption = TrajectoryAdaption(timestep, max_leapfrog_steps, target_accept, learning_rate, beta2,
                                           averaging_decay, gamma, t0, kappa)
        super(ChEESSampler, self).__init__(pdf, state, float(timestep), 1,
                                           timestep_adaption_limit=timestep_adaption_limit,
                                           variable_name=variable_name, rng=rng, mode=mode, metric=metric,
                                           dense_metric=dense_metric)
        self.jitter = bool(jitter)
        self.last_n_leapfrog = 0
        self.n_leapfrog_total = 0
        self.last_accept_prob = None
        self._ws, self._ws_key = None, None
        self._criterion = False           # the transition in flight is an adapting one
        self._inside = False              # ... a frozen one, inside HMCSampler.sample

    @property
    def variable_name(self):
        return 'ChEES' if self._variable_name is None else self._variable_name

    @property
    def adapting(self):
        return (self.counter + 1) < self.timestep_adaption_limit

    @property
    def trajectory_length(self):
        return self.adaption.T

    @trajectory_length.setter
    def trajectory_length(self, value):
        """Set T by hand (a value learnt elsewhere); clipped into [eps, max_leapfrog_steps eps]
        at the next transition's end or at the freeze."""
        if not (float(value) > 0.0 and math.isfinite(float(value))):
            raise ValueError('trajectory_length must be a positive number, not %r' % (value,))
        self.adaption.log_T = math.log(float(value))

    @property
    def max_leapfrog_steps(self):
        return self.adaption.max_leapfrog_steps

    @property
    def target_accept(self):
        return self.adaption.target_accept

    @property
    def mean_leapfrog_steps(self):
        """``max(1, ceil(T / (2 eps)))``, an int: the mean of the jittered step counts, and the
        constant count of ``jitter=False`` (the ``nsteps`` of an ``HMCSampler`` that replays the
        learnt configuration).  The steps actually taken: ``n_leapfrog_total / counter``."""
        return self.adaption.mean_steps()

    def restart_step_adaption(self):
        """Start the step size's dual averaging over (``WindowedWarmup``: after a change of
        metric); the trajectory length carries on."""
        self.adaption.restart_step_adaption()

    # -- what the base class asks ------------------------------------------------------------
    def _adapts_steps_in_kernel(self):
        return False                      # the step size is dual-averaged on the host, never per chain

    def _fused_spec(self, name, D, C=None):
        if self._criterion:
            return None                   # the criterion needs the proposal and its momentum
        return super(ChEESSampler, self)._fused_spec(name, D, C)

    def _workspace(self, C, D, dev):
        key = (C, D, dev, self.metric_scale is not None or self.metric_chol is not None)
        if self._ws_key != key:
            z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
            self._ws = {'alpha': z(C), 'g': z(C), 'mean_q': z(D), 'mean_prop': z(D), 'out': z(4),
                        'slab': _native.chees_workspace(C, D, dev), 'v': z(C, D) if key[3] else None}
            self._ws_key = key
        return self._ws

    def _before_accept(self, q0, q, p, e_before, e_after):
        if not self._criterion:
            return
        C, D = q0.shape
        ws = self._workspace(C, D, q0.device)
        alpha = ws['alpha']
        _native.chees_accept_prob(e_before, e_after, alpha)
        v = p                              # dq/dt at the trajectory's end: r' itself without a metric,
        if ws['v'] is not None:            # else what the sampler's drift adds at step 1.0
            v = ws['v'].zero_()
            self._integrator(_MODES[self.mode])[1](v, p, 1.0, None)
        _native.chees_means(q0, q, alpha, ws['slab'], ws['mean_q'], ws['mean_prop'])
        _native.chees_terms(q0, q, v, alpha, ws['mean_q'], ws['mean_prop'], ws['g'])
        _native.chees_sums(alpha, ws['g'], ws['slab'], ws['out'])

    # -- one transition ------------------------------------------------------------------------
    def sample(self, p0=None, u=None):
        """One transition per chain.  ``p0`` (``[C x D]``) and ``u`` (``[C]``) override the random
        draws (parity tests, pre-generated pools)."""
        if self.graph is not False:
            raise ValueError('ChEESSampler: graph must be False')
        if self._dt_chain is not None:
            raise ValueError('ChEESSampler: one step size for all chains (timestep must be a number)')
        ad = self.adaption
        if not self.adapting:
            if not ad.frozen:
                ad.eps = float(self._timestep)            # (a step the caller set before any adaption)
                ad.freeze()
            self.nsteps = ad.begin() if self.jitter else ad.mean_steps()
            self._timestep = ad.eps
            self._inside = True
            try:
                out = super(ChEESSampler, self).sample(p0=p0, u=u)
            finally:
                self._inside = False
            self.last_n_leapfrog = self.nsteps
            self.n_leapfrog_total += self.nsteps
            return out
        if ad.frozen:
            raise RuntimeError('ChEESSampler: frozen (timestep_adaption_limit was raised after the freeze)')
        if dist.world()[1] > 1:
            raise NotImplementedError('ChEESSampler: adaption pools all chains into one group and runs on one '
                                      'GPU; a frozen sampler works on shards as it is')
        state = _device_state(self.state)
        if isinstance(state, torch.Tensor):
            C, D = _as2d(state).shape
            if D > _native.CHEES_MAX_DIM:
                raise NotImplementedError('ChEESSampler: adapting with rows beyond %d elements is not supported'
                                          % _native.CHEES_MAX_DIM)
        self.nsteps = ad.begin()
        self._timestep = ad.eps
        self._criterion = True
        try:
            out = super(ChEESSampler, self).sample(p0=p0, u=u)
        finally:
            self._criterion = False
        ws = self._ws
        sums = ws['out'].tolist()                          # the transition's one read-back: 32 bytes
        self.last_accept_prob = ws['alpha'].clone()
        self.last_n_leapfrog = self.nsteps
        self.n_leapfrog_total += self.nsteps
        ad.update(sums, ws['alpha'].numel(), freeze=not self.adapting)     # (counter has moved on)
        self._timestep = ad.eps
        return out

    def sample_n(self, n, thin=1, p0=None, u=None, record=True, out=None):
        """``n`` consecutive ``sample()`` calls; the recorded states ``[n // thin, C, D]`` or None,
        the argument rules of ``HMCSampler.sample_n``.  A frozen sampler without jitter takes the
        base class's one-launch path; otherwise single calls (the step count changes)."""
        if self.graph is not False:
            raise ValueError('ChEESSampler: graph must be False')
        if self._inside:
            # a kind that draws in its kernel makes sample()'s one transition through sample_n(1):
            # nsteps is set, the base class's launch is what it wants
            return super(ChEESSampler, self).sample_n(n, thin=thin, p0=p0, u=u, record=record, out=out)
        if not self.adapting and not self.jitter:
            ad = self.adaption
            if not ad.frozen:
                ad.eps = float(self._timestep)
                ad.freeze()
            self.nsteps, self._timestep = ad.mean_steps(), ad.eps
            before = self.n_leapfrog_total               # (a PDF without a multi-transition kernel comes
            res = super(ChEESSampler, self).sample_n(n, thin=thin, p0=p0, u=u, record=record, out=out)
            self.last_n_leapfrog = self.nsteps           # back through sample(), which counts too)
            self.n_leapfrog_total = before + int(n) * self.nsteps
            return res
        n, thin = int(n), int(thin)
        if n < 1 or thin < 1:
            raise ValueError('sample_n: n >= 1 and thin >= 1 required')
        state = _device_state(self.state)
        shape, dev = tuple(state.shape), state.device
        C, D = _as2d(state).shape
        if p0 is not None:
            p0 = p0.reshape(n, C, D)
        if u is not None:
            u = u.reshape(n, C)
        self._check_record_buffer(out, record, n // thin, C, D, dev)
        return self._sample_n_singles(n, thin, p0, u, record, out, shape, dev)

    # -- checkpoint / resume ---------------------------------------------------------------------
    def state_dict(self):
        d = super(ChEESSampler, self).state_dict()
        d['chees'] = dict(self.adaption.state_dict(), n_leapfrog_total=int(self.n_leapfrog_total),
                          last_n_leapfrog=int(self.last_n_leapfrog))
        d['last_accept_prob'] = self.last_accept_prob
        return d

    def load_state_dict(self, d):
        super(ChEESSampler, self).load_state_dict(d)
        c = d['chees']
        self.adaption.load_state_dict(c)
        self.n_leapfrog_total, self.last_n_leapfrog = int(c['n_leapfrog_total']), int(c['last_n_leapfrog'])
        a = d.get('last_accept_prob')
        self.last_accept_prob = a.to(self.state.device) if isinstance(a, torch.Tensor) else None
        self._timestep = self.adaption.eps
        self._ws, self._ws_key = None, None
