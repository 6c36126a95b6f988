"""
Tempered sequential Monte Carlo: adaptive temperature ladders, resampling on the device, an
absolute log-evidence.

Not in the reference, which runs one chain at one temperature.  The ``[C x D]`` batch of an
inner sampler is the particle population; the target path is

    log p_beta(x) = log p_0(x) + beta * l(x),        l = log p_1 - log p_0

with ``p_0`` NORMALISED and the start state drawn from it (for prior -> posterior ``l`` is
the log-likelihood), so the product of the stage-wise mean weights estimates the evidence
``Z = integral p_0(x) exp(l(x)) dx`` itself, with no anchor missing -- what
``free_energy.bar`` over a replica ladder cannot give.  The pdf holds ``beta`` as a ``[C]``
fp64 device tensor that it reads at every call (the ``TemperedDoubleWell`` pattern of
``examples/replica_exchange.py``); the SMC writes that tensor in place, on the device.

Layout: ``C = G * P``, ``G`` independent populations of ``P`` neighbouring chains, population
``g`` the chains ``[g P, (g + 1) P)``.  Every population runs its own adaptive schedule --
the next beta holds the effective sample size of the incremental weights at ``ess_fraction *
P`` -- and has its own beta; the spread of ``log Z`` over populations is the standard error.
Populations never span ranks (``dist.shard_ladders(G, P)`` shards such a layout), and the
resampling draw is keyed by the global chain index of a population's first particle, so a
sharded run repeats the one-GPU run.  No collective is involved.

One stage: ``l`` of the current state; temper (``binf_smc_temper_f64``: weights, next beta,
log Z increment); systematic resampling (``binf_smc_resample_f64``); the row gather
(``binf_smc_gather_f64``) into a fresh state; ``n_mutations`` transitions of the inner
sampler at the new beta.  States move; the inner sampler's step sizes and acceptance
counters stay with the slot (all particles of a population sample one distribution).  Kernels
in ``csrc/smc.hip``, contracts in ``include/binf_hip.h``.  There is no CPU path.
"""
from collections import namedtuple

import torch

from binf_amd import _native
from binf_amd.samplers.rng import HostLegacyRNG

_FIELDS = 'log_evidence log_evidence_mean stderr betas ess n_unique n_stages status'


class SMCResult(namedtuple('SMCResult', _FIELDS)):
    """Device tensors.

      log_evidence       ``[G]``: log Z of every population
      log_evidence_mean  log of the mean of the populations' Z (log-mean-exp)
      stderr             standard deviation of ``log_evidence`` / sqrt(G); NaN for ``G = 1``
      betas              ``[stages x G]``: beta after every stage
      ess                ``[stages x G]``: effective sample size of the stage's weights
      n_unique           ``[stages x G]`` int64: distinct ancestors the resampling kept
      n_stages           ``[G]`` int64: stages in which the population took a step
      status             ``[G]`` int32 of the last stage (``_native.SMC_*``)
    """
    __slots__ = ()

    def cpu(self):
        return SMCResult(*(t.cpu() for t in self))

    def table(self):
        """The estimate as text, one row per population (moves the tensors to the host)."""
        h = self.cpu()
        G = int(h.log_evidence.shape[0])
        rows = ['%-10s %14s %7s %10s %10s %6s'
                % ('population', 'log_evidence', 'stages', 'min ess', 'min unique', 'status')]
        for g in range(G):
            took = h.betas.shape[0] > 0
            rows.append('%-10d %14.6g %7d %10.4g %10d %6d'
                        % (g, float(h.log_evidence[g]), int(h.n_stages[g]),
                           float(h.ess[:, g].min()) if took else float('nan'),
                           int(h.n_unique[:, g].min()) if took else 0, int(h.status[g])))
        rows.append('%-10s %14.6g %7s %10.3g' % ('mean', float(h.log_evidence_mean), '+/-', float(h.stderr)))
        return '\n'.join(rows)

    def __str__(self):
        return self.table()


class TemperedSMC(object):
    """Adaptive tempered SMC around ``sampler``, the mutation kernel.

    ``sampler`` is one single-variable sampler whose state is a ``[C x D]`` device tensor
    and whose ``pdf`` evaluates ``log_prob(**{variable: x}) -> [C]`` reading ``beta``:
    ``HMCSampler``, ``NUTSSampler`` or a frozen ``ChEESSampler``.

      beta            the pdf's ``[C]`` fp64 device tensor, constant within a population (the
                      start of the path, usually all 0); written in place at every stage
      n_populations   G (C must be a multiple)
      ess_fraction    rho in (0, 1]: the ESS every stage's weights are held at, as a fraction
                      of P
      n_mutations     transitions of the inner sampler per stage (one ``sample_n(k,
                      record=False)`` where it has one)
      log_likelihood  ``l(x) -> [C]``; default: ``pdf.log_prob`` with ``beta`` filled with 1
                      minus ``pdf.log_prob`` with ``beta`` filled with 0 (one subtraction),
                      ``beta`` restored afterwards
      rng             where the resampling uniforms come from; default: the inner sampler's.
                      A generator with ``next_offset`` (``DeviceRNG``): drawn inside the
                      kernel, one stream position per stage.  Anything else with
                      ``uniform(n, device)``: one ``uniform(G)`` per stage, supplied
      variable_name   the PDF's variable; default: the inner sampler's
      max_stages      ``run()`` raises when a population has not arrived by then
      n_bisect        halvings of the root search for the next beta
      before_mutation ``f(smc)`` called after the gather and before the transitions, e.g. to
                      set ``smc.sampler.timestep`` from ``smc.beta`` (device arithmetic)

    Attributes: ``beta_population`` (``[G]``), ``log_evidence`` (``[G]``, so far), ``stage``,
    ``last`` (the last stage's ``delta, w, log_z_inc, ess, n_invalid, status, ancestor,
    n_unique, log_likelihood``).
    """

    def __init__(self, sampler, beta, n_populations=1, ess_fraction=0.5, n_mutations=1,
                 log_likelihood=None, rng=None, variable_name=None, max_stages=1000, n_bisect=60,
                 before_mutation=None):
        G, k = int(n_populations), int(n_mutations)
        if G < 1 or k < 0 or int(max_stages) < 1:
            raise ValueError('TemperedSMC: n_populations >= 1, n_mutations >= 0 and max_stages >= 1 required')
        if not 0.0 < float(ess_fraction) <= 1.0:
            raise ValueError('TemperedSMC: ess_fraction must lie in (0, 1]')
        state = getattr(sampler, 'state', None)
        if not isinstance(state, torch.Tensor) or state.dim() != 2:
            raise ValueError('TemperedSMC: the inner sampler\'s state must be a [C x D] tensor')
        if not state.is_cuda:
            raise ValueError('TemperedSMC: the state must live in GPU memory (there is no CPU path)')
        C = state.shape[0]
        if C % G != 0:
            raise ValueError('TemperedSMC: %d chains are no whole number of %d populations' % (C, G))
        P = C // G
        if not 1 <= P <= _native.SMC_MAX_P:
            raise NotImplementedError('TemperedSMC: populations of 1 ... %d particles' % _native.SMC_MAX_P)
        _native.dptr(beta, numel=C, name='beta')
        if beta.device != state.device:
            raise ValueError('TemperedSMC: beta and the state live on different devices')
        if not bool((beta.view(G, P) == beta.view(G, P)[:, :1]).all()):
            raise ValueError('TemperedSMC: beta must be constant within a population')
        if variable_name is None:
            variable_name = getattr(sampler, '_variable_name', None)
            if not isinstance(variable_name, str):
                stats = getattr(sampler, 'last_draw_stats', None)
                if isinstance(stats, dict) and len(stats) == 1:
                    variable_name = next(iter(stats))
        if not isinstance(variable_name, str):
            raise TypeError('TemperedSMC needs variable_name')
        if rng is None:
            rng = getattr(sampler, 'rng', None)
        self.sampler = sampler
        self.pdf = sampler.pdf
        self.variable_name = variable_name
        self.beta = beta
        self.n_populations, self.n_particles = G, P
        self.ess_fraction = float(ess_fraction)
        self.n_mutations = k
        self.n_bisect = int(n_bisect)
        self.max_stages = int(max_stages)
        self.log_likelihood = log_likelihood
        self.before_mutation = before_mutation
        self.rng = rng if rng is not None else HostLegacyRNG()
        if int(getattr(self.rng, 'chain_offset', 0)) % P != 0:
            raise ValueError('TemperedSMC: the generator\'s chain_offset splits a population')
        self._refuse_pooled_adaption()
        dev = state.device
        self.beta_population = beta.view(G, P)[:, 0].clone()
        self.log_evidence = torch.zeros(G, dtype=torch.float64, device=dev)
        self.n_stages = torch.zeros(G, dtype=torch.int64, device=dev)
        self.status = torch.zeros(G, dtype=torch.int32, device=dev)
        self.stage = 0
        self._betas, self._ess, self._n_unique = [], [], []
        self.last = None

    def _refuse_pooled_adaption(self):
        s = self.sampler
        if self.n_populations > 1 and getattr(s, 'pools_chains_to_adapt', False) and \
                getattr(s, 'adapting', False):
            raise TypeError('TemperedSMC: an adapting %s pools all chains into one group; freeze it first '
                            '(the populations are at different temperatures)' % type(s).__name__)

    @property
    def state(self):
        return self.sampler.state

    # -- one stage -----------------------------------------------------------------------
    def _log_prob(self, x):
        lp = self.pdf.log_prob(**{self.variable_name: x})
        if not isinstance(lp, torch.Tensor):
            raise TypeError('pdf.log_prob must return a tensor with one value per chain, got %r' % type(lp))
        return lp.reshape(-1)

    def _log_likelihood(self, x):
        C = x.shape[0]
        if self.log_likelihood is not None:
            ll = self.log_likelihood(x)
        else:
            G, P = self.n_populations, self.n_particles
            try:
                self.beta.fill_(1.0)
                lp1 = self._log_prob(x)
                self.beta.fill_(0.0)
                lp0 = self._log_prob(x)
            finally:
                self.beta.view(G, P).copy_(self.beta_population[:, None])
            ll = lp1 - lp0
        if not isinstance(ll, torch.Tensor) or ll.numel() != C:
            raise TypeError('TemperedSMC: the log-likelihood must be a tensor with one value per chain')
        return ll.reshape(C).to(torch.float64).contiguous()

    def _mutate(self):
        s, k = self.sampler, self.n_mutations
        self._refuse_pooled_adaption()
        if k == 1:
            s.sample()
        elif k > 1 and hasattr(s, 'sample_n'):
            s.sample_n(k, record=False)
        else:
            for _ in range(k):
                s.sample()

    def step(self, u=None):
        """One stage; ``u`` (``[G]``) overrides the resampling draw.  Returns the new state."""
        s = self.sampler
        x = s.state.contiguous()
        G = self.n_populations
        ll = self._log_likelihood(x)
        t = _native.smc_temper(ll, self.beta_population, self.beta, self.ess_fraction, self.n_bisect)
        seed = offset = coff = 0
        if u is None:
            if hasattr(self.rng, 'next_offset'):
                seed, coff = self.rng.seed, int(getattr(self.rng, 'chain_offset', 0))
                offset = self.rng.next_offset()
            else:
                u = self.rng.uniform(G, x.device)
        if u is not None:
            u = u.reshape(G).contiguous()
        ancestor, n_unique = _native.smc_resample(t['w'], G, u=u, status=t['status'], seed=seed,
                                                  offset=offset, chain_offset=coff)
        # a fresh tensor: a state handed out earlier is never written again
        out, side = _native.smc_gather(x, ancestor, side=ll.view(1, -1))
        s.state = out
        self.log_evidence = self.log_evidence + t['log_z_inc']
        stepped = (t['status'] == _native.SMC_OK) | (t['status'] == _native.SMC_STALLED)
        self.n_stages = self.n_stages + stepped.to(torch.int64)
        self.status = t['status']
        self._betas.append(self.beta_population.clone())
        self._ess.append(t['ess'])
        self._n_unique.append(n_unique)
        self.last = dict(t, ancestor=ancestor, n_unique=n_unique, log_likelihood=side[0])
        self.stage += 1
        if self.before_mutation is not None:
            self.before_mutation(self)
        self._mutate()
        return s.state

    def run(self):
        """``step()`` until every population is at beta = 1 (one ``[G]`` read-back per stage,
        the only host synchronisation); returns :meth:`result`."""
        bad = (_native.SMC_NO_FINITE, _native.SMC_INVALID)
        while True:
            if self.stage >= self.max_stages:
                raise RuntimeError('TemperedSMC: not every population reached beta = 1 in %d stages'
                                   % self.max_stages)
            self.step()
            code = (self.status.to(torch.int64) * 2 + (self.beta_population >= 1.0).to(torch.int64)).cpu()
            done = code % 2 == 1
            for b in bad:
                if bool(((code // 2 == b) & ~done).any()):
                    raise RuntimeError('TemperedSMC: a population has %s log-likelihood'
                                       % ('no finite' if b == _native.SMC_NO_FINITE else 'a +inf'))
            if bool(done.all()):
                return self.result()

    def result(self):
        G = self.n_populations
        dev = self.log_evidence.device
        lz = self.log_evidence
        mean = torch.logsumexp(lz, 0) - torch.log(torch.tensor(float(G), dtype=torch.float64, device=dev))
        stderr = lz.std(unbiased=True) / G ** 0.5 if G > 1 else \
            torch.full((), float('nan'), dtype=torch.float64, device=dev)

        def rows(xs, dtype):
            return torch.stack(xs) if xs else torch.empty((0, G), dtype=dtype, device=dev)
        return SMCResult(lz, mean, stderr, rows(self._betas, torch.float64), rows(self._ess, torch.float64),
                         rows(self._n_unique, torch.int64), self.n_stages, self.status)

    # -- checkpoint / resume (binf_amd/checkpoint.py) ----------------------------------
    def state_dict(self):
        rng = getattr(self.rng, 'state_dict', None)
        r = self.result()
        return {'inner': self.sampler.state_dict(), 'stage': int(self.stage),
                'beta_population': self.beta_population.clone(), 'log_evidence': r.log_evidence,
                'betas': r.betas, 'ess': r.ess, 'n_unique': r.n_unique, 'n_stages': r.n_stages,
                'status': r.status, 'rng': rng() if rng is not None else None}

    def load_state_dict(self, d):
        G, P = self.n_populations, self.n_particles
        dev = self.log_evidence.device
        if d['beta_population'].numel() != G:
            raise ValueError('TemperedSMC checkpoint: %d populations, this sampler has %d'
                             % (d['beta_population'].numel(), G))
        self.sampler.load_state_dict(d['inner'])
        self.stage = int(d['stage'])
        self.beta_population = d['beta_population'].to(dev).clone().contiguous()
        self.beta.view(G, P).copy_(self.beta_population[:, None])
        self.log_evidence = d['log_evidence'].to(dev)
        self.n_stages = d['n_stages'].to(dev)
        self.status = d['status'].to(dev)
        self._betas = list(d['betas'].to(dev))
        self._ess = list(d['ess'].to(dev))
        self._n_unique = list(d['n_unique'].to(dev))
        self.last = None
        if d.get('rng') is not None and hasattr(self.rng, 'load_state_dict'):
            self.rng.load_state_dict(d['rng'])
