"""Host restatement (numpy) of the rank layer of the diagnostics -- ``csrc/ranks.hip`` and
``binf_amd.diagnostics.rank_summary`` -- written from the contract in ``include/binf_hip.h``
on top of ``diagnostics_ref.py``.  Nothing here calls into the library; the table of normal
scores is an argument (the tests pass the one the package builds, and check that table
against 50-digit arithmetic on its own).

Pooled set of dimension i: the ``S = split * n * C`` values of the split record
(:func:`split_record`), element ``e = t' * C + c``.  The sort is ``np.lexsort`` on (is-NaN,
value, not-sign-bit): ascending, -0.0 before +0.0, NaNs last.  The doubled rank of a value is
``lo + hi``, the first and last 1-based positions of its tie group (numeric equality), found
with ``np.searchsorted``.  The quantile is numpy's linear method spelled out:

    h = (S - 1) * p,  lo = floor(h),  g = h - lo,  a = sorted[lo],  b = sorted[min(lo + 1, S - 1)]
    d = b - a,  q = a + d * g if g < 0.5 else b - d * (1 - g)
"""
import numpy as np

import diagnostics_ref as DR

FOLD, LE = 0, 1


def split_record(x, split):
    """[split * n, C, D]: the draws the split chains are made of, in compressed time order."""
    x = np.asarray(x, dtype=np.float64)
    T = x.shape[0]
    assert split in (1, 2) and T // split >= 2
    n = T // split
    return x[:n] if split == 1 else np.concatenate([x[:n], x[T - n:]], axis=0)


def sort_values(v):
    """The 1-D array ``v`` ascending; -0.0 before +0.0; NaNs last."""
    v = np.asarray(v, dtype=np.float64)
    nan = np.isnan(v)
    order = np.lexsort((~np.signbit(v), np.where(nan, 0.0, v), nan))
    return v[order]


def doubled_ranks(v):
    """``lo + hi`` per element of the NaN-free 1-D array ``v`` (int64): twice the average rank."""
    s = np.sort(v)
    return (np.searchsorted(s, v, side='left') + 1 + np.searchsorted(s, v, side='right')).astype(np.int64)


def sorted_pooled(x, split):
    """[D, S]: what ``binf_rank_normalise_f64`` leaves in ``sorted``."""
    rec = split_record(x, split)
    D = rec.shape[2]
    return np.stack([sort_values(rec[:, :, i].reshape(-1)) for i in range(D)], axis=0)


def rank_normalise(x, split, ztab):
    """[split * n, C, D]: ``ztab[lo + hi]``; a dimension that holds a NaN is NaN throughout."""
    rec = split_record(x, split)
    Tp, C, D = rec.shape
    assert ztab.shape == (2 * Tp * C + 1,)
    z = np.empty_like(rec)
    for i in range(D):
        v = rec[:, :, i].reshape(-1)
        z[:, :, i] = np.nan if np.isnan(v).any() else ztab[doubled_ranks(v)].reshape(Tp, C)
    return z


def quantile_sorted(s, p):
    """The quantile of the ascending 1-D array ``s`` at probability ``p``."""
    f = np.float64
    S = s.shape[0]
    if np.isnan(s[S - 1]):
        return f(np.nan)
    with np.errstate(all='ignore'):
        h = f(S - 1) * f(p)
        lo = np.floor(h)
        g = h - lo
        lo = int(lo)
        a, b = s[lo], s[min(lo + 1, S - 1)]
        d = b - a
        return a + d * g if g < 0.5 else b - d * (f(1.0) - g)


def quantiles_sorted(sorted_values, probs):
    """[Q, D] from sorted [D, S]."""
    return np.array([[quantile_sorted(row, p) for row in sorted_values] for p in probs], dtype=np.float64).reshape(
        len(probs), sorted_values.shape[0])


def quantiles(x, probs):
    return quantiles_sorted(sorted_pooled(x, 1), probs)


def draws_map(x, split, op, param):
    rec = split_record(x, split)
    with np.errstate(all='ignore'):
        return np.abs(rec - param) if op == FOLD else (rec <= param).astype(np.float64)


def combine(rhat_bulk, rhat_folded, ess_lo, ess_hi, flags):
    """(rhat, ess_tail, truncated): np.maximum / np.minimum hand a NaN operand on."""
    t = np.zeros(rhat_bulk.shape, dtype=np.uint8)
    for f in flags:
        t |= (np.asarray(f) != 0).astype(np.uint8)
    return np.maximum(rhat_bulk, rhat_folded), np.minimum(ess_lo, ess_hi), t


def rank_summary(x, ztab, probs=(0.05, 0.5, 0.95), max_lag=None):
    """dict(mean, sd, rhat, ess_bulk, ess_tail, mcse, quantiles, truncated) and the pieces
    (rhat_bulk, rhat_folded, ess_lo, ess_hi), as ``binf_amd.diagnostics.rank_summary``
    composes them.  ``ztab``: the table for S = 2 * (T // 2) * C."""
    x = np.asarray(x, dtype=np.float64)
    raw = DR.diagnose(x, 2, max_lag)
    bulk = DR.diagnose(rank_normalise(x, 2, ztab), 2, max_lag)
    pooled = sorted_pooled(x, 2)
    med, q05, q95 = quantiles_sorted(pooled, (0.5, 0.05, 0.95))
    folded = draws_map(x, 2, FOLD, med)
    rhat_folded = DR.diagnose(rank_normalise(folded, 2, ztab), 2, 0)['rhat']
    lo = DR.diagnose(draws_map(x, 2, LE, q05), 2, max_lag)
    hi = DR.diagnose(draws_map(x, 2, LE, q95), 2, max_lag)
    rhat, ess_tail, truncated = combine(bulk['rhat'], rhat_folded, lo['ess'], hi['ess'],
                                        (raw['truncated'], bulk['truncated'], lo['truncated'], hi['truncated']))
    return dict(mean=raw['post_mean'], sd=raw['sd'], rhat=rhat, ess_bulk=bulk['ess'], ess_tail=ess_tail,
                mcse=raw['mcse'], quantiles=quantiles(x, probs), truncated=truncated,
                rhat_bulk=bulk['rhat'], rhat_folded=rhat_folded, ess_lo=lo['ess'], ess_hi=hi['ess'])


FIELDS = ('mean', 'sd', 'rhat', 'ess_bulk', 'ess_tail', 'mcse', 'quantiles', 'truncated')
