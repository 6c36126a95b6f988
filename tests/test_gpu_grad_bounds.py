"""The likelihood force ``G = A . ((theta . A - y) tau)`` of the polynomial and linear kinds
(csrc/poly.hip: ``poly_grad_mfma_kernel``, ``poly_grad_mfma_full_kernel``,
``split_reduce_kernel``, ``split_reduce_kick_drift_kernel``) and the chain-rule contraction
(csrc/jacobian.hip) held to exact arithmetic:

(a) on integer data every product and partial sum is a double in ANY order, so the kernels
    must return the int64 result bit for bit -- a wrong row, column, chain, tile or split
    of the two chained MFMA products is an integer difference;
(b) on four kinds of design matrix the force lies inside the DERIVED bound of
    tests/grad_bounds.py: sample chains against exact integer arithmetic within the bound
    itself, every chain against numpy within twice the bound (numpy's own force lies inside it);
(c) a non-finite coefficient or precision shows numpy's NaN / inf pattern in its own chain
    and leaves every other chain's bits alone, in both kernels;
(d) the fused leapfrog on integer data returns the rational trajectory bit for bit in both
    arithmetic modes;
(e) the contraction lies inside ``gamma_N sum|J||r|``.

The shapes (grad_bounds.force_cases) reach every instantiation of grad_dispatch, both
kernels, one / two chain tiles per wave, full, ragged and empty splits.  No tolerance here
is measured; every case of (b) and (e) prints its worst error / bound."""
import numpy as np
import pytest
import torch

import grad_bounds as GB
from binf_amd import _native

pytestmark = pytest.mark.gpu

CASES = GB.force_cases()


def dev_t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device)


def grad(theta, A, ys, precision, device):
    prec = dev_t(precision, device) if isinstance(precision, np.ndarray) else precision
    out = _native.poly_gauss_grad(dev_t(theta, device), dev_t(A, device), dev_t(ys, device), prec)
    assert tuple(out.shape) == theta.shape
    return out.cpu().numpy()


def trimmed(K, N):
    """grad_whole_tiles of csrc/poly.hip"""
    return N >= 16 and N % 16 == 0 and K * N < 2 ** 28


# ---------------------------------------------------------------------------
# (a) bits on integer data
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('K,N,C', CASES)
def test_force_is_exact_on_integer_data(device, K, N, C):
    """Every chain of every shape equals the int64 force bit for bit, with a host scalar and
    with per-chain power-of-two precisions."""
    assert GB.integer_case_width(K, N) < 53
    A, ys, theta, tau = GB.integer_case(K, N, C, 1000 * K + N + 7 * C)
    for prec in (0.25, 4.0, tau):
        want = GB.integer_force(A, ys, theta, prec)
        got = grad(theta, A, ys, prec, device)
        bad = np.nonzero(got != want)
        assert bad[0].size == 0, ('chain %d coefficient %d: %r, not %r (%d of %d differ)' % (
            bad[0][0], bad[1][0], got[bad][0], want[bad][0], bad[0].size, got.size))


# ---------------------------------------------------------------------------
# (b) the derived bound
# ---------------------------------------------------------------------------
def check_bound(device, kind, K, N, C):
    A, ys, theta, tau = GB.float_case(kind, K, N, C, 1000 * K + N + 7 * C)
    ef = GB.ExactForce(A, ys)
    chains = GB.sample_chains(C, K + N + C)
    assert len(chains) >= min(C, 4)
    worst_exact = worst_numpy = 0.0
    for prec in (2.5, tau):
        got = grad(theta, A, ys, prec, device)
        want, bound = GB.force_float(theta, A, ys, prec)
        with np.errstate(divide='ignore', invalid='ignore'):
            ratio = np.where(bound > 0.0, np.abs(got - want) / (2.0 * bound), np.where(got == want, 0.0, np.inf))
        worst_numpy = max(worst_numpy, float(ratio.max()))
        for c in chains:
            info = ef.chain(theta[c], float(np.broadcast_to(prec, (C,))[c]))
            err = ef.error(info['G'], got[c])
            with np.errstate(divide='ignore', invalid='ignore'):
                re = np.where(info['bound'] > 0.0, err / info['bound'], np.where(err == 0.0, 0.0, np.inf))
            worst_exact = max(worst_exact, float(re.max()))
    print('force K=%d N=%d C=%d %s (%s kernel): worst error / bound %.4f against exact arithmetic '
          '(%d chains), %.4f of twice the bound against numpy (all chains)'
          % (K, N, C, kind, 'trimmed' if trimmed(K, N) else 'general', worst_exact, len(chains), worst_numpy))
    assert worst_exact <= 1.0, worst_exact
    assert worst_numpy <= 1.0, worst_numpy


@pytest.mark.parametrize('K,N,C', CASES)
def test_force_inside_the_derived_bound(device, K, N, C):
    """One design per shape, all four in turn."""
    check_bound(device, GB.DESIGNS[(K + N + C) % 4], K, N, C)


@pytest.mark.parametrize('kind', GB.DESIGNS)
@pytest.mark.parametrize('K,N,C', [(33, 1027, 65), (33, 1040, 65), (34, 35, 4113), (50, 48, 4113),
                                   (17, 1040, 19), (64, 272, 4100)])
def test_force_inside_the_derived_bound_on_every_design(device, kind, K, N, C):
    """Every design on the ragged-split shapes of both kernels and on the VALU-tail
    instantiations under two chain tiles per wave."""
    check_bound(device, kind, K, N, C)


# ---------------------------------------------------------------------------
# (c) non-finite values stay in their chain
# ---------------------------------------------------------------------------
def same_pattern(got, want):
    nan, inf = np.isnan(want), np.isinf(want)
    return (np.array_equal(np.isnan(got), nan) and np.array_equal(np.isinf(got), inf)
            and np.array_equal(got[inf], want[inf]))


@pytest.mark.parametrize('kind', ['normal', 'poly', 'positive'])
@pytest.mark.parametrize('K,N,C', [(7, 37, 40), (33, 1027, 40), (18, 35, 4113), (33, 35, 4113),
                                   (7, 48, 40), (33, 1040, 40), (18, 32, 4113), (33, 48, 4113)])
def test_non_finite_values_stay_in_their_chain(device, kind, K, N, C):
    """+inf, NaN and -inf in single coefficients of a chain of the first 16-chain tile, of a
    wave's second tile and of the last tile; NaN, inf and 0 in single per-chain precisions.
    On the 'normal' and 'poly' designs the infinite residuals have both signs and all but one
    component of a touched chain is NaN; on the 'positive' design every component of the
    +inf chain is +inf and every one of the -inf chain -inf."""
    assert K % 4 != 0 and C in (40, 4113)
    A, ys, theta, tau = GB.float_case(kind, K, N, C, K + N + C)
    clean_host = grad(theta, A, ys, 2.5, device)
    clean = grad(theta, A, ys, tau, device)
    assert np.all(np.isfinite(clean)) and np.all(np.isfinite(clean_host))
    c_inf, c_nan, c_minf = 5, 21, C - 1             # 21: wave 0's second tile at C >= 4096
    assert (c_minf // 16) == (C - 1) // 16 and (C < 4096 or (c_minf % 32) >= 16)
    dirty = theta.copy()
    dirty[c_inf, K - 1] = np.inf                    # K - 1: the VALU tail's coefficient at K = 18, 33
    dirty[c_nan, 2] = np.nan
    dirty[c_minf, K - 1] = -np.inf
    touched = [c_inf, c_nan, c_minf]
    others = np.setdiff1d(np.arange(C), touched)
    for prec, ref in ((2.5, clean_host), (tau, clean)):
        got = grad(dirty, A, ys, prec, device)
        with np.errstate(all='ignore'):
            want = ((dirty @ A - ys) * np.broadcast_to(prec, (C,))[:, None]) @ A.T
        assert np.all(np.isfinite(want[others])) and not np.any(np.isfinite(want[c_nan]))
        for c in touched:
            assert not np.all(np.isfinite(got[c])), c
            assert same_pattern(got[c], want[c]), (c, got[c], want[c])
        if kind == 'positive':
            assert np.all(want[c_inf] == np.inf) and np.all(want[c_minf] == -np.inf)
            assert np.all(got[c_inf] == np.inf) and np.all(got[c_minf] == -np.inf)
        assert np.array_equal(got[others], ref[others])
    # precisions
    t_dirty = tau.copy()
    t_dirty[c_inf], t_dirty[c_nan], t_dirty[c_minf] = np.inf, np.nan, 0.0
    got = grad(theta, A, ys, t_dirty, device)
    with np.errstate(all='ignore'):
        want = ((theta @ A - ys) * t_dirty[:, None]) @ A.T
    for c in (c_inf, c_nan):
        assert same_pattern(got[c], want[c]), (c, got[c], want[c])
    assert np.all(np.isnan(got[c_nan])) and not np.any(np.isfinite(got[c_inf]))
    assert np.array_equal(got[c_minf], np.zeros(K)) and np.array_equal(want[c_minf], np.zeros(K))
    assert np.array_equal(got[others], clean[others])


# ---------------------------------------------------------------------------
# (d) the fused leapfrog on integer data
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('C', [17, 4100])
@pytest.mark.parametrize('K,N,L,k', GB.LEAPFROG_CASES)
def test_fused_leapfrog_is_the_rational_trajectory_on_integer_data(device, K, N, L, k, C):
    """Integer q, p, A, y, power-of-two step and precision: the L + 1 forces, kicks and drifts
    are exact (widths asserted in test_grad_bounds.py), so EXACT and FMA mode both return the
    rational trajectory bit for bit."""
    A, ys, q, p, tau_exp = GB.leapfrog_case(K, N, C, K + N)
    dt_exp = k - (np.arange(C) % 2)
    Ad, yd = dev_t(A, device), dev_t(ys, device)
    for te, de in ((0, k), (tau_exp, k), (tau_exp, dt_exp)):
        want_q, want_p, width = GB.leapfrog_ints(A, ys, q, p, te, de, L)
        assert width < 53
        prec = dev_t(2.0 ** te, device) if isinstance(te, np.ndarray) else 2.0 ** te
        dt_chain = dev_t(2.0 ** -de, device) if isinstance(de, np.ndarray) else None
        timestep = 0.0 if dt_chain is not None else 2.0 ** -de
        for mode in (_native.MODE_EXACT, _native.MODE_FMA):
            qd, pd = dev_t(q, device), dev_t(p, device)
            _native.poly_leapfrog(qd, pd, Ad, yd, prec, timestep, dt_chain, L, mode)
            assert np.array_equal(qd.cpu().numpy(), want_q), (mode, width)
            assert np.array_equal(pd.cpu().numpy(), want_p), (mode, width)


# ---------------------------------------------------------------------------
# (e) the chain-rule contraction
# ---------------------------------------------------------------------------
def contract_case(kind, K, N, C, batched, seed):
    rs = np.random.RandomState(seed)
    if batched:
        J = np.stack([GB.design(kind, K, N, rs) for _ in range(C)])
    else:
        J = GB.design(kind, K, N, rs)
    r = rs.standard_normal((C, N)) * 2.0 ** rs.randint(-8, 9, size=(C, 1))
    return J, r


CONTRACT_SHAPES = [(K, N, 19) for K in (1, 16, 17, 64, 65) for N in (1, 63, 64, 65, 129)]


@pytest.mark.parametrize('batched', [False, True])
@pytest.mark.parametrize('K,N,C', CONTRACT_SHAPES + [(33, 1024, 40), (33, 1027, 70)])
def test_contraction_inside_gamma_n(device, K, N, C, batched):
    """Shared (MFMA, 16-chain workgroups) and per-chain (FMA) Jacobians."""
    check_contraction(device, GB.DESIGNS[(K + N) % 4], K, N, C, batched)


def test_contraction_inside_gamma_n_in_32_chain_workgroups(device):
    """From 8161 chains and 1024 data points on: jac_shared_mfma32_kernel."""
    check_contraction(device, 'normal', 33, 1024, 8192, False)


def check_contraction(device, kind, K, N, C, batched):
    J, r = contract_case(kind, K, N, C, batched, 100 * K + N + C)
    got = _native.jacobian_contract(dev_t(J, device), dev_t(r, device)).cpu().numpy()
    assert got.shape == (C, K)
    want = np.einsum('ckn,cn->ck', J, r) if batched else r.dot(J.T)
    bound = GB.contract_bound(J, r)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(bound > 0.0, np.abs(got - want) / (2.0 * bound), np.where(got == want, 0.0, np.inf))
    chains = GB.sample_chains(C, K + N)
    assert len(chains) >= min(C, 4)
    worst = 0.0
    for c in chains:
        Jc = J[c] if batched else J
        err = GB.contract_error(Jc, r[c], got[c])
        with np.errstate(divide='ignore', invalid='ignore'):
            re = np.where(bound[c] > 0.0, err / bound[c], np.where(err == 0.0, 0.0, np.inf))
        worst = max(worst, float(re.max()))
    print('contraction K=%d N=%d C=%d %s %s: worst error / bound %.4f against exact arithmetic '
          '(%d chains), %.4f of twice the bound against numpy (all chains)'
          % (K, N, C, kind, 'per-chain' if batched else 'shared', worst, len(chains), float(ratio.max())))
    assert worst <= 1.0, worst
    assert float(ratio.max()) <= 1.0, float(ratio.max())
