"""
Free-energy differences between the slots of a tempered ladder, on the device: Bennett's
acceptance ratio (BAR) over the work record of a :class:`ReplicaExchangeSampler`.

Every slot ``r`` of a ladder has a normalising constant ``Z_r = integral exp(log_prob_r(x))
dx``.  A swap round already evaluates, for every pair of neighbours, the log-prob of each
member's draw under the other slot; ``ReplicaExchangeSampler(..., record_work=n)`` keeps
those differences (``[n x C]``, one row per round, nothing evaluated twice), and :func:`bar`
turns the record into ``delta[r] = log Z_r - log Z_{r+1}`` and its sum along the ladder.  On
a precision ladder that is the log-evidence ratio of the models at noise precisions
``beta_r * tau``; on a ``beta`` ladder of a user's pdf a free-energy difference.

The arithmetic is the HIP library's (``csrc/free_energy.hip``, contract in
``include/binf_hip.h``): every sum has one fixed order, so a result is reproducible bit for
bit and independent of ``groups``.  There is no CPU path.  A sharded run estimates from the
gathered record, ``bar(gathered_record, ...)``: the single-GPU result by construction.
"""
from collections import namedtuple

import torch

from binf_amd import _native

_FIELDS = ('delta delta_forward delta_reverse overlap n_samples var_iid status group_delta '
           'stderr cumulative total total_stderr')


class FreeEnergy(namedtuple('FreeEnergy', _FIELDS)):
    """Device tensors.  Per pair ``(r, r + 1)``, ``[R - 1]``, from all ladders pooled:

      delta          BAR estimate of ``log Z_r - log Z_{r+1}``
      delta_forward  the exponential average over the draws of slot ``r + 1`` alone
      delta_reverse  the one over the draws of slot ``r`` alone (with BAR between the two
                     where the slots overlap; far apart where they do not)
      overlap        ``S / n`` in [0, 1/2]: ``S = sum sigma (1 - sigma)`` at ``delta``
      n_samples      samples per direction (int64)
      var_iid        ``1 / S - 2 / n``: the variance of ``delta`` were the draws independent
      status         int32, ``_native.FE_*`` (0: fine; ``FE_NO_OVERLAP``: every logistic
                     underflowed, ``overlap`` is 0 and ``delta`` is not determined)

    From the ``groups`` solve (ladders cut into ``G`` groups, each estimated on its own):

      group_delta    ``[G x (R - 1)]``
      stderr         ``[R - 1]``: standard deviation of the group estimates / sqrt(G); NaN
                     for ``G = 1``.  Autocorrelation along a ladder's rounds is inside it
      cumulative     ``[R]``: ``log Z_r - log Z_0``
      total          ``log Z_0 - log Z_{R-1}``, the sum of ``delta``
      total_stderr   from the per-group totals, so correlations between pairs are inside it
    """
    __slots__ = ()

    def cpu(self):
        return FreeEnergy(*(t.cpu() for t in self))

    def table(self):
        """The estimate as text, one row per pair (moves the tensors to the host)."""
        h = self.cpu()
        P = int(h.delta.shape[0])
        rows = ['%-7s %13s %10s %13s %13s %8s %10s %6s'
                % ('pair', 'delta', 'stderr', 'forward', 'reverse', 'overlap', 'n', 'status')]
        for r in range(P):
            rows.append('%-7s %13.6g %10.3g %13.6g %13.6g %8.4f %10d %6d'
                        % ('%d-%d' % (r, r + 1), float(h.delta[r]), float(h.stderr[r]),
                           float(h.delta_forward[r]), float(h.delta_reverse[r]),
                           float(h.overlap[r]), int(h.n_samples[r]), int(h.status[r])))
        rows.append('%-7s %13.6g %10.3g' % ('total', float(h.total), float(h.total_stderr)))
        return '\n'.join(rows)

    def __str__(self):
        return self.table()


def bar(work, n_replicas, first_round=0, groups=1):
    """:class:`FreeEnergy` of a ``[T x C]`` work record (``ReplicaExchangeSampler.work``; a
    view with unit inner stride is read in place) whose row 0 was written in round
    ``first_round``.  ``groups`` must divide the number of ladders; the pooled solve and the
    grouped one are two calls of ``binf_free_energy_bar_f64``, and the few-element
    arithmetic on top is torch on the device."""
    R, G = int(n_replicas), int(groups)
    pooled = _native.free_energy_bar(work, R, first_round, 1)
    grouped = pooled if G == 1 else _native.free_energy_bar(work, R, first_round, G)
    delta = pooled['delta'][0]
    S = pooled['info'][0]
    n = pooled['n'][0]
    nf = n.to(torch.float64)
    gd = grouped['delta']
    nan = torch.full_like(delta, float('nan'))
    if G > 1:
        stderr = gd.std(dim=0, unbiased=True) / G ** 0.5
        total_stderr = gd.sum(dim=1).std(unbiased=True) / G ** 0.5
    else:
        stderr = nan
        total_stderr = torch.full((), float('nan'), dtype=torch.float64, device=delta.device)
    cumulative = torch.cat([torch.zeros(1, dtype=torch.float64, device=delta.device),
                            -torch.cumsum(delta, 0)])
    return FreeEnergy(delta, pooled['delta_forward'][0], pooled['delta_reverse'][0], S / nf, n,
                      1.0 / S - 2.0 / nf, pooled['status'][0], gd, stderr, cumulative,
                      delta.sum(), total_stderr)
