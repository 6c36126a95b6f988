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
