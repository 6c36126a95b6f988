"""
Replica exchange across chains: tempered ladders, swaps on the device.

Not in the reference, which has the hooks such a scheme drives -- ``HMCSampler.
last_draw_stats`` is "usually used by a replica exchange scheme"
(``binf/samplers/hmc.py:171-176``) -- and no exchange of its own.

Layout: ``C = n_ladders * R`` chains in one ``[C x D]`` state; chain ``c`` is slot
``r = c % R`` of ladder ``c // R``.  Slots differ in whatever per-chain (``[C]`` tensor)
parameters the PDF holds -- a tempered precision (:func:`ladder_precision`), the ``beta``
of a user's torch PDF -- and the exchange never needs to know which: it evaluates
``pdf.log_prob`` on the state and on the state with every pair's rows exchanged.

A swap round has a parity: slot ``r`` is the lower member of the pair ``(r, r + 1)`` iff
``r >= parity``, ``r - parity`` is even and ``r + 1 < R``.  Rounds alternate parity,
starting at 0 (deterministic even/odd).  STATES move between slots; parameters, the inner
sampler's step sizes and its acceptance counters stay with the slot, so every temperature
keeps its own adapted step.  For a pair ``(i, j)``

    delta = (lp_sw[i] + lp_sw[j]) - (lp_own[i] + lp_own[j])
    accept iff u < exp(clip(delta, -308, 709))

in ``csrc/replica.hip`` (``binf_replica_gather_f64`` / ``binf_replica_swap_f64``).  No host
read-back anywhere in a round: flags and counters stay on the device, parity is host
arithmetic.  There is no CPU path.
"""
import torch

from binf_amd import _native
from binf_amd.samplers.rng import HostLegacyRNG


def geometric_betas(n_replicas, beta_min):
    """``beta_r = beta_min ** (r / (R - 1))``, r = 0 .. R-1: 1 at slot 0 (the target), a
    constant ratio between neighbours, ``beta_min`` at the top.  A list of floats."""
    R, beta_min = int(n_replicas), float(beta_min)
    if R < 1 or not 0.0 < beta_min <= 1.0:
        raise ValueError('geometric_betas: n_replicas >= 1 and 0 < beta_min <= 1 required')
    if R == 1:
        return [1.0]
    return [1.0] + [beta_min ** (r / float(R - 1)) for r in range(1, R - 1)] + [beta_min]


def ladder_precision(betas, precision, n_ladders, device=None):
    """``[C]`` per-chain precision ``beta_r * precision`` of ``n_ladders`` ladders -- the
    likelihood-tempered ladder ``L(x)^beta_r pi(x)`` of a likelihood that takes a per-chain
    precision.  Host arithmetic (one rounding per slot), once at set-up."""
    tau = float(precision)
    row = torch.tensor([float(b) * tau for b in betas], dtype=torch.float64)
    if row.numel() < 1 or int(n_ladders) < 0:
        raise ValueError('ladder_precision: at least one beta and n_ladders >= 0 required')
    return row.repeat(int(n_ladders)).to(device)


def _refuse_pooled_adaption(sampler):
    """A sampler that tunes itself from ALL its chains as one group (an adapting
    ``ChEESSampler``) cannot drive a ladder, whose slots sample different distributions."""
    if getattr(sampler, 'pools_chains_to_adapt', False) and getattr(sampler, 'adapting', False):
        raise TypeError('ReplicaExchangeSampler: an adapting %s pools all chains into one group; freeze it '
                        'first (the slots of a ladder are different distributions)' % type(sampler).__name__)


class ReplicaExchangeSampler(object):
    """Alternates the transitions of ``sampler`` with swap rounds between neighbouring slots.

    ``sampler`` is one single-variable sampler whose state is a ``[C x D]`` device tensor
    and whose ``pdf`` evaluates ``log_prob(**{variable: x}) -> [C]`` with per-chain
    parameters: ``HMCSampler`` on any tier, or a random-walk Metropolis sampler of the same
    shape (``sample()``, ``state``, ``pdf``).

      n_replicas     R, slots per ladder (C must be a multiple)
      swap_interval  inner transitions per swap round (one ``sample_n(swap_interval,
                     record=False)`` of the inner sampler where it has one)
      rng            where the swap uniforms come from; default: the inner sampler's
                     generator.  A generator with ``next_offset`` (``DeviceRNG``): drawn
                     inside the swap kernel, one stream position per round, keyed by the
                     global chain index of the pair's lower member.  Anything else with
                     ``uniform(n, device)``: one ``uniform(C)`` per round, supplied.
      track_walkers  keep ``walker`` (``[C]`` int64): the id (start chain) of the walker now
                     in each slot, exchanged with the states
      variable_name  the PDF's variable; default: the inner sampler's
      record_work    None (off), or the number of swap rounds a ``[record_work x C]`` device
                     record has room for: every round then keeps ``lp_sw[c] -
                     lp_own[partner(c)]`` of its pairs (NaN at unpaired chains), the forward
                     and reverse work values ``free_energy()`` estimates from
                     (``binf_replica_work_f64``: one small launch more, nothing read back).
                     ``work`` is the ``[rounds recorded x C]`` view, ``work_first_round`` the
                     ``round`` of its row 0; ``reset_work()`` starts the record over (after
                     burn-in).  A round that finds the record full raises before anything
                     is launched or changed

    Attributes: ``last_swap_accepted`` (``[C]`` bool, both members of an accepted pair),
    ``n_swap_attempted`` / ``n_swap_accepted`` (``[C]`` int64, at the pair's lower member),
    ``swap_acceptance_rate`` (``[R - 1]``, reduced over ladders when asked for), ``walker``,
    ``round``.
    """

    def __init__(self, sampler, n_replicas, swap_interval=1, rng=None, track_walkers=False,
                 variable_name=None, record_work=None):
        R, k = int(n_replicas), int(swap_interval)
        if R < 1 or k < 1:
            raise ValueError('ReplicaExchangeSampler: n_replicas >= 1 and swap_interval >= 1 required')
        state = sampler.state
        if not isinstance(state, torch.Tensor) or state.dim() != 2:
            raise ValueError('ReplicaExchangeSampler: the inner sampler\'s state must be a [C x D] tensor')
        C = state.shape[0]
        if C % R != 0:
            raise ValueError('ReplicaExchangeSampler: %d chains are no whole number of ladders of %d'
                             % (C, R))
        if variable_name is None:
            variable_name = getattr(sampler, '_variable_name', None)
            if not isinstance(variable_name, str):
                stats = getattr(sampler, 'last_draw_stats', None)
                if isinstance(stats, dict) and len(stats) == 1:
                    variable_name = next(iter(stats))
        if not isinstance(variable_name, str):
            raise TypeError('ReplicaExchangeSampler needs variable_name')
        if rng is None:
            rng = getattr(sampler, 'rng', None)
        _refuse_pooled_adaption(sampler)
        self.sampler = sampler
        self.pdf = sampler.pdf
        self.variable_name = variable_name
        self.n_replicas = R
        self.n_ladders = C // R
        self.swap_interval = k
        self.rng = rng if rng is not None else HostLegacyRNG()
        self.round = 0
        dev = state.device
        self.n_swap_attempted = torch.zeros(C, dtype=torch.int64, device=dev)
        self.n_swap_accepted = torch.zeros(C, dtype=torch.int64, device=dev)
        self.last_swap_accepted = torch.zeros(C, dtype=torch.bool, device=dev)
        self.walker = torch.arange(C, dtype=torch.int64, device=dev) if track_walkers else None
        self._work = None
        if record_work is not None:
            if int(record_work) < 1:
                raise ValueError('ReplicaExchangeSampler: record_work must be None or >= 1')
            self._work = torch.empty((int(record_work), C), dtype=torch.float64, device=dev)
        self._work_fill = 0
        self.work_first_round = 0

    # -- views ---------------------------------------------------------------------------
    @property
    def state(self):
        return self.sampler.state

    def slot(self, x, r):
        """The ``[n_ladders x D]`` view of slot ``r`` of a ``[C x D]`` state (or of a
        ``[n, C, D]`` record: ``[n, n_ladders, D]``; of a ``[C]`` vector: ``[n_ladders]``);
        ``slot(x, 0)`` is the target's samples."""
        R = self.n_replicas
        if not 0 <= int(r) < R:
            raise IndexError('slot %r of a ladder of %d' % (r, R))
        if x.dim() == 1:
            return x.view(self.n_ladders, R)[:, int(r)]
        return x.unflatten(-2, (self.n_ladders, R))[..., int(r), :]

    @property
    def swap_acceptance_rate(self):
        """``[R - 1]``: accepted / attempted swaps of the slot pairs (r, r + 1), over all
        ladders (0 where nothing was attempted).  A reduction: not for the sampling loop."""
        R = self.n_replicas
        att = self.n_swap_attempted.view(self.n_ladders, R).sum(dim=0)[:R - 1].to(torch.float64)
        acc = self.n_swap_accepted.view(self.n_ladders, R).sum(dim=0)[:R - 1].to(torch.float64)
        return acc / att.clamp(min=1.0)

    # -- the work record ---------------------------------------------------------------
    @property
    def work(self):
        """``[rounds recorded x C]``: the view of the filled rows of the work record (row
        ``t`` belongs to round ``work_first_round + t``)."""
        if self._work is None:
            raise ValueError('ReplicaExchangeSampler: no work is recorded (record_work=None)')
        return self._work[:self._work_fill]

    def reset_work(self):
        """Forget the rounds recorded so far; the next swap round writes row 0."""
        if self._work is None:
            raise ValueError('ReplicaExchangeSampler: no work is recorded (record_work=None)')
        self._work_fill = 0
        self.work_first_round = int(self.round)

    def free_energy(self, groups=1):
        """:func:`binf_amd.free_energy.bar` of the rounds recorded so far."""
        from binf_amd import free_energy
        return free_energy.bar(self.work, self.n_replicas, self.work_first_round, groups)

    def _require_work_room(self):
        if self._work is not None and self._work_fill >= self._work.shape[0]:
            raise RuntimeError('ReplicaExchangeSampler: the work record is full (%d rounds); '
                               'reset_work() or a larger record_work' % self._work.shape[0])

    # -- one round -------------------------------------------------------------------------
    def _log_prob(self, x):
        lp = self.pdf.log_prob(**{self.variable_name: x})
        if not isinstance(lp, torch.Tensor):
            raise TypeError('pdf.log_prob must return a tensor with one value per chain, got %r'
                            % type(lp))
        return lp.reshape(-1).contiguous()

    def _transitions(self, inner):
        s, k = self.sampler, self.swap_interval
        inner = inner or {}
        _refuse_pooled_adaption(s)
        if k == 1:
            s.sample(**inner)
        elif hasattr(s, 'sample_n'):
            s.sample_n(k, record=False, **inner)
        else:
            for i in range(k):
                s.sample(**dict((name, v[i]) for name, v in inner.items()))

    def swap(self, u=None):
        """One swap round on the inner sampler's state (``sample()`` without the
        transitions): gather, the two log-prob evaluations, swap; returns the new state."""
        self._require_work_room()
        s = self.sampler
        x = s.state.contiguous()
        C = x.shape[0]
        R, parity = self.n_replicas, self.round & 1
        x_perm = _native.replica_gather(x, R, parity)
        lp_own = self._log_prob(x)
        lp_sw = self._log_prob(x_perm)
        if self._work is not None:
            if self._work_fill == 0:
                self.work_first_round = int(self.round)
            _native.replica_work(lp_own, lp_sw, R, parity, out=self._work[self._work_fill])
            self._work_fill += 1
        seed = offset = coff = 0
        if u is None:
            if hasattr(self.rng, 'next_offset'):
                seed, coff = self.rng.seed, int(getattr(self.rng, 'chain_offset', 0))
                offset = self.rng.next_offset()
            else:
                u = self.rng.uniform(C, x.device)
        if u is not None:
            u = u.reshape(C).contiguous()
        accepted = torch.empty(C, dtype=torch.uint8, device=x.device)
        # a fresh tensor: a state handed out earlier is never written again
        out = _native.replica_swap(x, lp_own, lp_sw, R, parity, accepted, u=u,
                                   n_attempted=self.n_swap_attempted,
                                   n_accepted=self.n_swap_accepted, walker=self.walker,
                                   seed=seed, offset=offset, chain_offset=coff)
        self.last_swap_accepted = accepted.view(torch.bool)
        self.round += 1
        s.state = out
        return out

    def sample(self, u=None, inner=None):
        """``swap_interval`` transitions of the inner sampler, then one swap round.  ``u``
        (``[C]``; a pair reads its lower member's entry) overrides the swap draw; ``inner``
        is a dict of keyword arguments for the inner sampler's ``sample()`` (for
        ``swap_interval > 1``: of its ``sample_n``, i.e. with a leading axis of that
        length), e.g. ``{'p0': ..., 'u': ...}`` -- tests, pre-generated pools."""
        self._require_work_room()
        self._transitions(inner)
        return self.swap(u)

    def sample_n(self, n, thin=1, record=True, out=None, u=None, inner=None):
        """``n`` rounds; returns the states after rounds ``thin, 2 * thin, ...`` as
        ``[n // thin, C, D]`` (None if ``record`` is false), the argument rules of
        ``HMCSampler.sample_n``.  ``u`` is ``[n, C]``, the values of ``inner`` carry a
        leading axis of length ``n``.  Bit-identical to ``n`` calls of ``sample()``."""
        n, thin = int(n), int(thin)
        if n < 1 or thin < 1:
            raise ValueError('sample_n: n >= 1 and thin >= 1 required')
        x0 = self.sampler.state
        C, D = x0.shape
        nrec = n // thin
        if out is not None:
            if not record or nrec < 1:
                raise ValueError('sample_n: out= given but nothing is recorded')
            if out.dtype != torch.float64 or out.device != x0.device or \
                    not out.is_contiguous() or out.numel() != nrec * C * D:
                raise ValueError('sample_n: out must be a contiguous fp64 [%d, %d, %d] '
                                 'tensor on %s' % (nrec, C, D, x0.device))
        if self._work is not None and self._work_fill + n > self._work.shape[0]:
            raise RuntimeError('ReplicaExchangeSampler: %d rounds do not fit the work record '
                               '(%d of %d rows used); reset_work() or a larger record_work'
                               % (n, self._work_fill, self._work.shape[0]))
        if u is not None:
            u = u.reshape(n, C)
        rec = None
        if record:
            rec = out.view(nrec, C, D) if out is not None else \
                torch.empty((nrec, C, D), dtype=torch.float64, device=x0.device)
        for i in range(n):
            x = self.sample(u=None if u is None else u[i],
                            inner=None if inner is None else
                            dict((name, v[i]) for name, v in inner.items()))
            if record and (i + 1) % thin == 0:
                rec[(i + 1) // thin - 1].copy_(x)
        return rec

    # -- checkpoint / resume (binf_amd/checkpoint.py) ----------------------------------
    def state_dict(self):
        rng = getattr(self.rng, 'state_dict', None)
        work = {}
        if self._work is not None:
            work = {'work': self.work.clone(), 'work_fill': int(self._work_fill),
                    'work_first_round': int(self.work_first_round)}
        return {**work, 'inner': self.sampler.state_dict(), 'round': int(self.round),
                # (copies: the swap kernel updates the counters and the walker ids in place)
                'n_swap_attempted': self.n_swap_attempted.clone(),
                'n_swap_accepted': self.n_swap_accepted.clone(),
                'last_swap_accepted': self.last_swap_accepted,
                'walker': None if self.walker is None else self.walker.clone(),
                'rng': rng() if rng is not None else None}

    def load_state_dict(self, d):
        dev = self.n_swap_attempted.device
        # the work record is checked before anything of this sampler is overwritten
        rec = d.get('work') if self._work is not None else None
        if rec is not None:
            if rec.dim() != 2 or rec.shape[1] != self._work.shape[1] or \
                    rec.shape[0] > self._work.shape[0]:
                raise ValueError('ReplicaExchangeSampler checkpoint: a work record of %s does '
                                 'not fit this sampler\'s %s' % (tuple(rec.shape),
                                                                tuple(self._work.shape)))
            if int(d.get('work_fill', rec.shape[0])) != rec.shape[0]:
                raise ValueError('ReplicaExchangeSampler checkpoint: work_fill and the '
                                 'record\'s rows disagree')
            if 'work_first_round' not in d:
                raise ValueError('ReplicaExchangeSampler checkpoint: a work record without '
                                 'work_first_round')
        self.sampler.load_state_dict(d['inner'])
        self.round = int(d['round'])
        # private copies: the counters are updated in place by the swap kernel
        self.n_swap_attempted = d['n_swap_attempted'].to(dev).clone().contiguous()
        self.n_swap_accepted = d['n_swap_accepted'].to(dev).clone().contiguous()
        self.last_swap_accepted = d['last_swap_accepted'].to(dev)
        if (d['walker'] is None) != (self.walker is None):
            raise ValueError('ReplicaExchangeSampler checkpoint %s walkers, this sampler %s'
                             % ('tracks' if d['walker'] is not None else 'does not track',
                                'does' if self.walker is not None else 'does not'))
        if self.walker is not None:
            self.walker = d['walker'].to(dev).clone().contiguous()
        if d.get('rng') is not None and hasattr(self.rng, 'load_state_dict'):
            self.rng.load_state_dict(d['rng'])
        if self._work is not None:
            # a checkpoint without a record (recording was off, or it predates the record):
            # the record starts over at the checkpoint's round
            self.reset_work()
            if rec is not None:
                self._work_fill = int(rec.shape[0])
                self._work[:self._work_fill].copy_(rec)
                self.work_first_round = int(d['work_first_round'])
