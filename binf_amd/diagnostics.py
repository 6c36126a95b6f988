"""
Convergence diagnostics over the kept draws of many chains, on the device: split-R^,
effective sample size and Monte-Carlo standard error per dimension.

``draws`` is any ``[T x C x D]`` fp64 device tensor with unit inner stride: the buffer of a
:class:`binf_amd.dist.SampleStore`, what ``sample_n`` returns, a column slice of a Gibbs
slot (``store.local()[:, :, :K]``) or the cold slot of a ladder (``draws[:, 0::R, :]``).
Views are read through their strides; nothing is copied.  A sharded run diagnoses the
gathered record, ``summary(store.gather())``: the result is then the single-GPU result by
construction.

The arithmetic is the HIP library's (``csrc/diagnostics.hip``, contract in
``include/binf_hip.h``): every sum has one fixed order, so a result is reproducible bit for
bit and equal to the host restatement the tests keep.  Everything but :func:`chain_moments`
cuts each chain into its first and last ``T // 2`` draws (split chains), which makes a drift
inside a chain show as between-chain variance.
"""
from collections import namedtuple

from binf_amd import _native

ChainMoments = namedtuple('ChainMoments', 'mean m2 n')


def default_max_lag(n):
    return min(int(n) - 1, 64)


def _segment_length(draws, split):
    return int(draws.shape[0]) // int(split) if int(split) in (1, 2) else 0


def chain_moments(draws, split=1):
    """``ChainMoments(mean, m2, n)``: mean and sum of squared deviations ``[split * C x D]`` of
    every (split) chain over its ``n = T // split`` draws; the sample variance of a chain is
    ``m2 / (n - 1)``.  Available for a single chain too."""
    mean, m2 = _native.chain_moments(draws, split)
    return ChainMoments(mean, m2, _segment_length(draws, split))


def split_rhat(draws):
    """Potential scale reduction ``[D]``: ``sqrt(varplus / W)`` over the split chains.  Needs
    two split chains at least.  A dimension that is constant in every chain gives NaN."""
    mean, m2 = _native.chain_moments(draws, 2)
    return _native.diag_summary(mean, m2, None, _segment_length(draws, 2))['rhat']


def _full(draws, max_lag):
    mean, m2 = _native.chain_moments(draws, 2)
    n = _segment_length(draws, 2)
    K = default_max_lag(n) if max_lag is None else int(max_lag)
    part = _native.chain_autocov(draws, mean, 2, K)
    return _native.diag_summary(mean, m2, part, n)


def effective_sample_size(draws, max_lag=None):
    """Effective sample size ``[D]`` of the ``M * n`` draws (Geyer's initial monotone sequence
    on the multi-chain autocorrelation, lags up to ``max_lag``, default ``min(n - 1, 64)``).
    Where the pair sums stay positive up to ``max_lag`` the sum was cut short and the value is
    an UPPER bound: :func:`summary` reports that as ``truncated``."""
    return _full(draws, max_lag)['ess']


class Summary(namedtuple('Summary', 'mean sd rhat ess mcse truncated')):
    """``[D]`` tensors per dimension: posterior mean over all chains, ``sd = sqrt(varplus)``,
    split-R^, effective sample size, Monte-Carlo standard error of the mean
    (``sd / sqrt(ess)``) and ``truncated`` (uint8: 1 where no negative pair sum was reached
    within ``max_lag``, so that ``ess`` is an upper bound and ``mcse`` a lower one)."""
    __slots__ = ()

    def cpu(self):
        return Summary(*(t.cpu() for t in self))

    def table(self, names=None):
        """The summary as text, one row per dimension (moves the tensors to the host)."""
        h = self.cpu()
        D = int(h.mean.shape[0])
        names = ['[%d]' % i for i in range(D)] if names is None else list(names)
        width = max([4] + [len(s) for s in names])
        rows = ['%-*s %12s %12s %8s %12s %12s' % (width, 'dim', 'mean', 'sd', 'rhat', 'ess', 'mcse')]
        for i in range(D):
            rows.append('%-*s %12.5g %12.5g %8.4f %11.1f%s %12.3g'
                        % (width, names[i], float(h.mean[i]), float(h.sd[i]), float(h.rhat[i]),
                           float(h.ess[i]), '+' if int(h.truncated[i]) else ' ', float(h.mcse[i])))
        if bool(h.truncated.any()):
            rows.append("('+': no negative pair within max_lag; ess is an upper bound)")
        return '\n'.join(rows)

    def __str__(self):
        return self.table()


def summary(draws, max_lag=None):
    """:class:`Summary` of ``draws``: three launches' worth of kernels (moments,
    autocovariance, the across-chain step), no host read-back."""
    r = _full(draws, max_lag)
    return Summary(r['post_mean'], r['sd'], r['rhat'], r['ess'], r['mcse'], r['truncated'])


# ---------------------------------------------------------------------------
# The rank layer (csrc/ranks.hip): a sort of the whole record per dimension on the device,
# and from it quantiles, rank-normalised / folded split-R^ and bulk / tail ESS (Vehtari,
# Gelman, Simpson, Carpenter, Buerkner 2021).
# ---------------------------------------------------------------------------
_Z_TABLES = {}


def rank_z_table(S, device):
    """The ``2 S + 1`` normal scores of doubled ranks: ``ztab[k] = ndtri((k / 2 - 3 / 8) /
    (S + 1 / 4))``, ``k = lo + hi`` of a tie group (twice its average rank), ``2 <= k <= 2 S``.
    The lower half is evaluated on the host in fp64, ``ztab[S + 1]`` is 0.0 and the upper half
    mirrors the lower (the two probabilities add to 1 exactly), so the table is antisymmetric
    bit for bit; entries 0 and 1 are NaN.  Cached per ``(S, device)``."""
    import torch
    S, device = int(S), torch.device(device)
    key = (S, str(device))
    tab = _Z_TABLES.get(key)
    if tab is None:
        if S < 1:
            raise ValueError('rank_z_table: S >= 1 required (got %d)' % S)
        k = torch.arange(2, S + 1, dtype=torch.float64)
        lower = torch.special.ndtri((k / 2.0 - 0.375) / (S + 0.25))
        host = torch.full((2 * S + 1,), float('nan'), dtype=torch.float64)
        host[2:S + 1] = lower
        host[S + 1] = 0.0
        host[S + 2:] = -lower.flip(0)
        if len(_Z_TABLES) >= 8:
            _Z_TABLES.clear()
        tab = _Z_TABLES[key] = host.to(device)
    return tab


def _pooled_size(draws, split):
    return int(split) * _segment_length(draws, split) * int(draws.shape[1])


def rank_normalise(draws, split=2):
    """``z [split * n x C x D]``: every draw of the (split) record replaced by the normal score
    of its rank among the ``S = split * n * C`` draws of its dimension; ties share their
    average rank.  A dimension that holds a NaN is NaN throughout."""
    ztab = rank_z_table(max(_pooled_size(draws, split), 1), draws.device)
    return _native.rank_normalise(draws, split, ztab)[1]


def quantiles(draws, probs):
    """``[Q x D]`` posterior quantiles over every draw of every chain (numpy's linear
    method, bit for bit); ``probs``: up to 16 numbers in [0, 1]."""
    return _native.sorted_quantiles(_native.rank_normalise(draws, 1, want_sorted=True)[0], probs)


class RankSummary(namedtuple('RankSummary', 'mean sd rhat ess_bulk ess_tail mcse quantiles truncated')):
    """``[D]`` tensors per dimension (``quantiles``: ``[Q x D]``): posterior mean, sd and
    Monte-Carlo standard error of the mean as in :class:`Summary`; ``rhat``, the larger of the
    rank-normalised and the folded rank-normalised split-R^; ``ess_bulk``, the ESS of the
    rank-normalised draws; ``ess_tail``, the smaller ESS of the indicators of the pooled 5 %
    and 95 % quantiles; ``truncated`` (uint8): 1 where any of the ESS sums behind ``mcse``,
    ``ess_bulk`` or ``ess_tail`` reached no negative pair within ``max_lag``.  ``probs``: the
    probabilities of the rows of ``quantiles``, as :func:`rank_summary` was given them."""
    probs = (0.05, 0.5, 0.95)

    def cpu(self):
        out = RankSummary(*(t.cpu() for t in self))
        out.probs = self.probs
        return out

    def table(self, names=None):
        """The summary as text, one row per dimension (moves the tensors to the host)."""
        h = self.cpu()
        D, Q = int(h.mean.shape[0]), int(h.quantiles.shape[0])
        labels = ['q%g' % (100.0 * p) for p in self.probs] if len(self.probs) == Q else ['q[%d]' % j for j in range(Q)]
        names = ['[%d]' % i for i in range(D)] if names is None else list(names)
        width = max([4] + [len(s) for s in names])
        rows = ['%-*s %12s %12s %8s %12s %12s %12s' % (width, 'dim', 'mean', 'sd', 'rhat', 'ess_bulk',
                                                       'ess_tail', 'mcse')
                + ''.join(' %12s' % s for s in labels)]
        for i in range(D):
            rows.append('%-*s %12.5g %12.5g %8.4f %12.1f %11.1f%s %12.3g'
                        % (width, names[i], float(h.mean[i]), float(h.sd[i]), float(h.rhat[i]),
                           float(h.ess_bulk[i]), float(h.ess_tail[i]), '+' if int(h.truncated[i]) else ' ',
                           float(h.mcse[i]))
                        + ''.join(' %12.5g' % float(h.quantiles[j, i]) for j in range(Q)))
        if bool(h.truncated.any()):
            rows.append("('+': no negative pair within max_lag; an ess is an upper bound)")
        return '\n'.join(rows)

    def __str__(self):
        return self.table()


def _rank_group(x, probs, max_lag):
    """:func:`rank_summary` of the ``[T x C x Dg]`` view ``x``, a tuple in field order.  One
    record buffer serves the rank-normalised draws, the folded draws and the two indicators
    in turn; the buffer of the sorted values holds the rank-normalised folded draws after them."""
    import torch
    T, C, Dg = (int(s) for s in x.shape)
    n = T // 2
    Sp, dev = 2 * n * C, x.device
    raw = _full(x, max_lag)
    ztab = rank_z_table(max(Sp, 1), dev)
    rec = torch.empty((2 * n, C, Dg), dtype=torch.float64, device=dev)
    flat = torch.empty(Dg * T * C, dtype=torch.float64, device=dev)
    pooled = flat[:Dg * Sp].view(Dg, Sp)
    _native.rank_normalise(x, 2, ztab, z=rec, sorted_out=pooled)
    bulk = _full(rec, max_lag)
    cuts = _native.sorted_quantiles(pooled, (0.5, 0.05, 0.95))
    if T % 2 == 0:                                  # the split record is the whole record
        q = _native.sorted_quantiles(pooled, probs)
    else:
        every = flat.view(Dg, T * C)
        _native.rank_normalise(x, 1, sorted_out=every)
        q = _native.sorted_quantiles(every, probs)
    _native.draws_map(x, 2, _native.DRAWS_MAP_FOLD, cuts[0], out=rec)
    zf = _native.rank_normalise(rec, 2, ztab, z=flat[:Dg * Sp].view(2 * n, C, Dg))[1]
    fmean, fm2 = _native.chain_moments(zf, 2)
    rhat_folded = _native.diag_summary(fmean, fm2, None, n)['rhat']
    _native.draws_map(x, 2, _native.DRAWS_MAP_LE, cuts[1], out=rec)
    lo = _full(rec, max_lag)
    _native.draws_map(x, 2, _native.DRAWS_MAP_LE, cuts[2], out=rec)
    hi = _full(rec, max_lag)
    rhat, ess_tail, truncated = _native.rank_diag_combine(
        bulk['rhat'], rhat_folded, lo['ess'], hi['ess'], raw['truncated'], bulk['truncated'],
        lo['truncated'], hi['truncated'])
    return raw['post_mean'], raw['sd'], rhat, bulk['ess'], ess_tail, raw['mcse'], q, truncated


def rank_summary(draws, probs=(0.05, 0.5, 0.95), max_lag=None, max_scratch_bytes=2 ** 30):
    """:class:`RankSummary` of ``draws``: ``mean``, ``sd`` and ``mcse`` as :func:`summary`
    gives them; rank-normalised split-R^ and bulk ESS from the same kernels run on
    :func:`rank_normalise` of the split record; the folded R^ from the rank-normalised
    distances to the pooled median; tail ESS from the indicators ``x <= q`` at the pooled 5 %
    and 95 % quantiles; ``quantiles`` at ``probs`` over all draws.  Every dimension is
    independent of the others, so the dimensions are walked in groups that keep the
    record-sized scratch (a record, the sorted values and the sort's workspace) under
    ``max_scratch_bytes`` -- one dimension at a time if it must be; the result does not depend
    on the grouping.  No host read-back."""
    import torch
    if not isinstance(draws, torch.Tensor) or draws.dim() != 3:
        raise ValueError('draws must be a [T x C x D] tensor')
    T, C, D = (int(s) for s in draws.shape)
    probs = tuple(float(p) for p in probs)
    S1 = max(T * C, 2)
    per_dim = 8 * 2 * S1 + 12 * (1 << (S1 - 1).bit_length()) + 256
    table = 8 * (2 * S1 + 1)
    Dg = max(1, min(D, (int(max_scratch_bytes) - table) // per_dim))
    parts = [_rank_group(draws[:, :, g:g + Dg], probs, max_lag) for g in range(0, D, Dg)]
    if len(parts) == 1:
        fields = parts[0]
    else:
        fields = [torch.cat([p[f] for p in parts], dim=1 if f == 6 else 0) for f in range(8)]
    out = RankSummary(*fields)
    out.probs = probs
    return out
