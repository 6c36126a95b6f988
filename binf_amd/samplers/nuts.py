"""
No-U-turn sampler for chain-batched states: every chain grows its own trajectory until it
turns back on itself, and the step sizes are tuned by dual averaging.

``NUTSSampler`` is an :class:`HMCSampler` whose trajectory length is dynamic.  The transition is
iterative multinomial NUTS (``include/binf_hip.h`` states it line by line): sub-tree U-turn
checks through per-depth checkpoints, progressive sampling uniform inside a sub-tree and biased
at the top.  The momenta are the whitened r ~ N(0, I) of every metric here, so the generalised
U-turn criterion is ``r . rho`` for the identity, the diagonal and the dense metric alike and
one tree kernel (``csrc/nuts.hip``) serves all three; the integrator is the existing per-step
kick and drift launches with a SIGNED per-chain step (a chain whose tree is finished gets
step 0, so no leapfrog path needs a per-chain step count).

There is no CPU path: without the HIP library this module raises.
"""
import math

import torch

from binf_amd import _native
from binf_amd.samplers.hmc import HMCSampler, _MODES, _as2d, _as_chain_vector, _device_state


class NUTSSampler(HMCSampler):
    """``NUTSSampler(pdf, state, timestep, max_tree_depth=10, target_accept=0.8, ...)``.

    One ``sample()``: draw r0 and the transition's uniforms (``[C x S]``, ``S = 2 max_tree_depth
    + 2^max_tree_depth - 1``) with the sampler's ``rng`` (``fill_uniform`` where the generator
    has it, so a ``DeviceRNG.for_shard`` shard equals the full batch), evaluate ``pdf.log_prob``
    and ``pdf.gradient`` at the state, ``binf_nuts_begin_f64``; then per leaf half kick, drift,
    ``pdf.gradient``, half kick (plain, ``_scaled`` or ``_dense`` launches with ``dt_chain`` =
    the tree's signed steps, in the sampler's ``mode``), ``pdf.log_prob``, ``binf_nuts_leaf_f64``.

    Host synchronisation: after the leaf totals 2^k - 1 (k = 1 ... max_tree_depth) the host
    reads back the number of chains still growing (``binf_nuts_pending``) and stops at 0.  That
    is the only synchronisation, at most ``max_tree_depth`` reads per transition.

    Step sizes: while ``counter + 1 < timestep_adaption_limit`` every transition ends with a
    dual-averaging update towards ``target_accept`` (per chain; ``gamma``, ``t0``, ``kappa`` as
    in Hoffman & Gelman 2014); the last adapting transition freezes the averaged steps.
    ``restart_step_adaption()`` starts the averaging over around ten times the current steps
    (``WindowedWarmup`` calls it whenever it changes the metric).

    Per-chain attributes (``[C]`` device tensors, of the last transition unless said otherwise):
    ``last_tree_depth``, ``last_n_leapfrog``, ``last_diverging``, ``last_accept_stat``,
    ``last_status`` (``_native.NUTS_TURN`` / ``SUBTURN`` / ``MAXD`` / ``DIV``), ``last_move_accepted``
    (the proposal is not the start), running ``n_divergent``, ``n_accepted``, ``acceptance_rate``.

    Not supported (refused): ``graph`` other than False, ``nsteps``, a subclass ``_leapfrog``;
    rows beyond 8192 elements and ``max_tree_depth`` beyond 12 (the kernel's limits).
    """

    def __init__(self, pdf, state, timestep, max_tree_depth=10, target_accept=0.8, max_delta=1000.0,
                 timestep_adaption_limit=0, variable_name=None, rng=None, mode='exact', metric=None,
                 dense_metric=None, gamma=0.05, t0=10.0, kappa=0.75, **refused):
        if refused.get('graph', False) is not False:
            raise ValueError('NUTSSampler: graph replay of the leaf step is not supported (graph must be False)')
        refused.pop('graph', None)
        if 'nsteps' in refused:
            raise ValueError('NUTSSampler takes no nsteps: the trajectory length is dynamic (max_tree_depth bounds it)')
        if refused:
            raise TypeError('NUTSSampler: unexpected arguments %s' % sorted(refused))
        if type(self)._leapfrog is not HMCSampler._leapfrog:
            raise TypeError('NUTSSampler integrates with the library\'s per-step launches: a subclass '
                            '_leapfrog is not supported')
        md = int(max_tree_depth)
        if not 1 <= md <= _native.NUTS_MAX_DEPTH:
            raise ValueError('max_tree_depth must be 1 ... %d, not %r' % (_native.NUTS_MAX_DEPTH, max_tree_depth))
        if not 0.0 < float(target_accept) < 1.0:
            raise ValueError('target_accept must lie in (0, 1)')
        super(NUTSSampler, self).__init__(pdf, state, timestep, 1, timestep_adaption_limit=timestep_adaption_limit,
                                          variable_name=variable_name, rng=rng, mode=mode, metric=metric,
                                          dense_metric=dense_metric)
        self.max_tree_depth, self.target_accept, self.max_delta = md, float(target_accept), float(max_delta)
        self.gamma, self.t0, self.kappa = float(gamma), float(t0), float(kappa)
        self.n_divergent = 0
        self._ws, self._ws_key = None, None
        self._da, self._da_t = None, 0

    @property
    def variable_name(self):
        return 'NUTS' if self._variable_name is None else self._variable_name

    def _fused_spec(self, name, D, C=None):
        return None                       # the kinds' whole-transition kernels are fixed-length HMC

    # -- workspace: once per (C, D, max_depth, device) ---------------------------------------
    def _workspace(self, C, D, dev):
        key = (C, D, self.max_tree_depth, dev)
        if self._ws_key != key:
            ws = {n: torch.zeros(shape, dtype=dtype, device=dev)
                  for n, (shape, dtype) in _native.nuts_shapes(C, D, self.max_tree_depth).items()}
            ws['count'] = torch.zeros(1, dtype=torch.int64, device=dev)
            if isinstance(self.n_accepted, torch.Tensor) and self.n_accepted.numel() == C:
                ws['n_accepted'].copy_(self.n_accepted)
            if isinstance(self.n_divergent, torch.Tensor) and self.n_divergent.numel() == C:
                ws['n_divergent'].copy_(self.n_divergent)
            self.n_accepted, self.n_divergent = ws['n_accepted'], ws['n_divergent']
            ws['args'] = _native.nuts_args(ws, C, D, self.max_tree_depth, self.max_delta)
            self._ws, self._ws_key = ws, key
        self._ws['args'].max_delta = float(self.max_delta)
        return self._ws

    def _steps(self, C, dev):
        """The per-chain step sizes, a ``[C]`` tensor from the first transition on."""
        if self._dt_chain is None:
            self._dt_chain = torch.full((C,), float(self._timestep), dtype=torch.float64, device=dev)
        return self._dt_chain

    def _averaging(self, C, dev):
        if self._da is None or self._da['hbar'].numel() != C:
            z = lambda: torch.zeros(C, dtype=torch.float64, device=dev)
            self._da = {'hbar': z(), 'logeps': z(), 'logeps_bar': z(), 'mu': z()}
            self._da_t = 0
            self._adapt(1)
        return self._da

    def _adapt(self, action, accept_stat=None):
        d, eps = self._da, self._dt_chain
        t = max(1, self._da_t)
        _native.nuts_adapt_step(eps, accept_stat, d['hbar'], d['logeps'], d['logeps_bar'], d['mu'],
                                self.target_accept, 1.0 / (t + self.t0), math.sqrt(float(t)) / self.gamma,
                                float(t) ** -self.kappa, action)

    def restart_step_adaption(self):
        """Start the dual averaging over: ``mu = log(10 eps)`` at the current steps, averages
        zeroed (after a change of metric, as Stan does at every window's end)."""
        if self._dt_chain is None or not self._dt_chain.is_cuda:
            state = _device_state(self.state)
            q = _as2d(state)
            self._steps(q.shape[0], q.device)
        if self._da is None:
            self._averaging(self._dt_chain.numel(), self._dt_chain.device)     # restarts itself
            return
        self._da_t = 0
        self._adapt(1)

    # -- one transition ------------------------------------------------------------------------
    def sample(self, p0=None, u=None):
        """One NUTS transition per chain.  ``p0`` (``[C x D]``) and ``u`` (``[C x S]``) override
        the random draws (parity tests, pre-generated pools)."""
        name = self._variable_name
        if not isinstance(name, str):
            raise TypeError('NUTSSampler needs variable_name to sample()')
        if self.graph is not False:
            raise ValueError('NUTSSampler: graph must be False')
        state = _device_state(self.state)
        shape = state.shape
        q0 = _as2d(state).contiguous()
        C, D = q0.shape
        dev = q0.device
        _native.require_device(q0, 'the sampler state')
        if D > _native.NUTS_MAX_DIM:
            raise NotImplementedError('NUTSSampler: rows beyond %d elements are not supported' % _native.NUTS_MAX_DIM)
        pdf, mode = self.pdf, _MODES[self.mode]
        ws = self._workspace(C, D, dev)
        a = ws['args']
        eps = self._steps(C, dev)
        if eps.numel() != C or eps.dtype != torch.float64 or not eps.is_contiguous() or eps.device != dev:
            raise ValueError('NUTSSampler: timestep must be a number or a contiguous [C] fp64 tensor on the state\'s device')
        a.eps = eps.data_ptr()
        adapt = (self.counter + 1) < self.timestep_adaption_limit
        if adapt:
            self._averaging(C, dev)
        S = _native.nuts_uniforms_per_chain(self.max_tree_depth)
        q, r, g = ws['q'], ws['r'], ws['g']
        if p0 is None:
            fill = getattr(self.rng, 'fill_normal', None)
            if fill is not None:
                fill(r)
            else:
                r.copy_(self.rng.normal((C, D), dev))
        else:
            r.copy_(_as2d(p0))
        if u is None:
            fill = getattr(self.rng, 'fill_uniform', None)
            if fill is not None:
                fill(ws['u'])
            else:
                ws['u'].copy_(self.rng.uniform(C * S, dev).reshape(C, S))
        else:
            ws['u'].copy_(u.reshape(C, S))
        q.copy_(q0)

        def logp_into():
            lp = _as_chain_vector(pdf.log_prob(**{name: q.view(shape)}))
            if lp.numel() != C:
                raise ValueError('pdf.log_prob returned %d values for %d chains' % (lp.numel(), C))
            ws['logp'].copy_(lp)

        def grad_into():
            gr = pdf.gradient(**{name: q.view(shape)})
            if not isinstance(gr, torch.Tensor) or gr.numel() != q.numel():
                raise ValueError('pdf.gradient(%s=...) returned %s for a state of shape %s'
                                 % (name, tuple(getattr(gr, 'shape', ())) or type(gr).__name__, tuple(shape)))
            g.copy_(gr.reshape(C, D))

        half_kick, drift, _ = self._integrator(mode)     # of the sampler's metric, once per transition
        dt = ws['dt_dir']
        logp_into()
        grad_into()
        _native.nuts_begin(a, dev)
        leaves, checkpoint = 0, 1
        for _ in range((1 << self.max_tree_depth) - 1):
            half_kick(r, g, 0.0, dt)
            drift(q, r, 0.0, dt)
            grad_into()
            half_kick(r, g, 0.0, dt)
            logp_into()
            _native.nuts_leaf(a, dev)
            leaves += 1
            if leaves == checkpoint:
                # the one read-back: leaf totals 1, 3, 7, ... (a tree can only end there or later)
                _native.nuts_pending(ws['status'], ws['count'])
                if int(ws['count'].item()) == 0:
                    break
                checkpoint = 2 * checkpoint + 1
        if adapt:
            self._da_t += 1
            self._adapt(0, ws['accept_stat'])
            if self.counter + 2 >= self.timestep_adaption_limit:
                self._adapt(2)
        self.last_tree_depth = ws['tree_depth'].clone()
        self.last_n_leapfrog = ws['n_leap'].clone()
        self.last_diverging = ws['diverging'].clone().view(torch.bool)
        self.last_accept_stat = ws['accept_stat'].clone()
        self.last_status = ws['status'].clone()
        self._last_move_accepted = ws['moved'].clone().view(torch.bool)
        self.counter += 1
        q_out = ws['q_out'].clone().view(shape)
        self.state = q_out
        return q_out

    def sample_n(self, n, thin=1, p0=None, u=None, record=True, out=None):
        """``n`` consecutive ``sample()`` calls; the recorded states ``[n // thin, C, D]`` (after
        transitions ``thin, 2 thin, ...``) or None.  ``p0`` is ``[n, C, D]`` and ``u`` ``[n, C, S]``
        (a transition's uniforms are a row of S per chain, not one number); ``out`` as for
        ``HMCSampler.sample_n``."""
        n, thin = int(n), int(thin)
        if n < 1 or thin < 1:
            raise ValueError('sample_n: n >= 1 and thin >= 1 required')
        state = _device_state(self.state)
        shape, dev = tuple(state.shape), state.device
        C, D = _as2d(state).shape
        if p0 is not None:
            p0 = p0.reshape(n, C, D)
        if u is not None:
            u = u.reshape(n, C, _native.nuts_uniforms_per_chain(self.max_tree_depth))
        self._check_record_buffer(out, record, n // thin, C, D, dev)
        # (a NUTS transition keeps no energies: the shared loop finds none to stack)
        return self._sample_n_singles(n, thin, p0, u, record, out, shape, dev)

    # -- checkpoint / resume ---------------------------------------------------------------------
    def state_dict(self):
        d = super(NUTSSampler, self).state_dict()
        d['n_divergent'] = self.n_divergent
        d['dual_averaging'] = None if self._da is None else dict(self._da, t=int(self._da_t))
        return d

    def load_state_dict(self, d):
        super(NUTSSampler, self).load_state_dict(d)
        ref = self.state
        n = d.get('n_divergent', 0)
        self.n_divergent = n.to(ref.device) if isinstance(n, torch.Tensor) else n
        self._ws, self._ws_key = None, None            # the counters move into a fresh workspace
        da = d.get('dual_averaging')
        if da is None:
            self._da, self._da_t = None, 0
        else:
            self._da = {k: da[k].to(device=ref.device, dtype=torch.float64).clone()
                        for k in ('hbar', 'logeps', 'logeps_bar', 'mu')}
            self._da_t = int(da['t'])
