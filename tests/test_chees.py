"""CPU tests of ChEES-HMC: the Halton jitter, ``TrajectoryAdaption``'s scalar logic driven with sums
from the host restatement (``tests/chees_ref.py``), the trajectory length the scheme must find on
an isotropic Gaussian, and the C-ABI additions (bound, version unchanged, refusals before any
launch)."""
import math

import numpy as np
import pytest

import chees_ref as R
from binf_amd import _native
from binf_amd.samplers.chees import TrajectoryAdaption, halton

f64 = np.float64


def test_halton_values_are_exact():
    want = [0.5, 0.25, 0.75, 0.125, 0.625, 0.375, 0.875, 0.0625, 0.5625, 0.3125]
    assert [halton(t) for t in range(1, 11)] == want
    for t in (1, 2, 3, 1000, 4097, 2 ** 40 + 1):
        bits = bin(t)[2:]
        assert halton(t) == sum(int(b) * 2.0 ** -(len(bits) - i) for i, b in enumerate(bits))   # exact sums of powers of 2
        assert 0.0 < halton(t) < 1.0
    assert halton(2 ** 40 + 1) == 0.5 + 2.0 ** -41


def _sums(seed, C=70, D=6, zero=(), scale=1.0):
    rs = np.random.RandomState(seed)
    q, qp, v = rs.standard_normal((C, D)), scale * rs.standard_normal((C, D)), rs.standard_normal((C, D))
    alpha = rs.uniform(0.1, 1.0, size=C)
    alpha[list(zero)] = 0.0
    return R.criterion(q, qp, v, alpha)[3]


def test_step_count_jitter_and_clipping():
    ad = TrajectoryAdaption(0.1, max_leapfrog_steps=7, target_accept=None)
    assert ad.T == pytest.approx(0.1, rel=1e-15) and ad.eps == 0.1 and ad.index == 0
    assert ad.begin() == 1 and ad.index == 1                          # ceil(0.5 * 0.1 / 0.1) = 1
    ad.log_T = math.log(0.55)
    assert [ad.steps_for(h) for h in (0.5, 0.25, 0.75, 1.0)] == [3, 2, 5, 6]
    ad.log_T = math.log(5.0)
    assert ad.steps_for(0.75) == 7 and ad.mean_steps() == 7             # max_leapfrog_steps
    # a gradient that pushes T beyond either end: clipped to [eps, max_leapfrog_steps eps]
    for sign, end in ((+1.0, 0.7), (-1.0, 0.1)):
        ad = TrajectoryAdaption(0.1, max_leapfrog_steps=7, target_accept=None)
        ad.log_T = math.log(0.3)
        for _ in range(200):
            ad.begin()
            ad.update([sign * 3.0, 1.0, 70.0, 0.0], 70)
            assert 0.1 * (1 - 1e-15) <= ad.T <= 0.7 * (1 + 1e-15)
        assert ad.T == pytest.approx(end, rel=1e-14)
        assert ad.eps == 0.1                                            # target_accept=None: fixed


def test_sums_without_accepted_mass_or_finite_gradient_leave_T_alone():
    ad = TrajectoryAdaption(0.1, target_accept=None)
    ad.log_T = math.log(0.4)
    ad.begin()
    ad.update(list(_sums(0)), 70)
    T, m2, n = ad.T, ad.m2, ad.n_updates
    assert n == 1 and T != pytest.approx(0.4, rel=1e-6)
    all_zero = _sums(1, zero=range(70))
    assert all_zero[1] == 0.0 and all_zero[0] == 0.0 and all_zero[2] == np.inf
    overflow = _sums(2, scale=1e200)
    assert overflow[3] == 70.0 and overflow[1] == 0.0                 # every g overflowed: none is summed
    for s in (all_zero, overflow, [float('nan'), 1.0, 70.0, 0.0], [float('inf'), 1.0, 70.0, 0.0], [1.0, 0.0, 70.0, 0.0]):
        ad.begin()
        ad.update([float(x) for x in s], 70)
        assert ad.T == T and ad.m2 == m2 and ad.n_updates == n
    assert ad.n_skipped == 5 and ad.n_avg == 6


def test_first_adam_step_is_the_learning_rate():
    """beta1 = 0 and the bias-corrected second moment: the first step is lr * sign(g) (up to the 1e-8)."""
    for s0 in (4.0, -4.0):
        ad = TrajectoryAdaption(0.1, target_accept=None, learning_rate=0.03)
        ad.log_T = math.log(0.5)
        assert ad.begin() == 3                                        # ceil(0.25 / 0.1): the time integrated is 0.3
        ad.update([s0, 2.0, 70.0, 0.0], 70)
        g = 0.3 * s0 / 2.0
        assert ad.log_T == pytest.approx(math.log(0.5) + 0.03 * g / (abs(g) + 1e-8), rel=1e-13)


def test_freeze_gives_exp_of_the_bias_corrected_average():
    ad = TrajectoryAdaption(0.1, target_accept=None)
    ad.log_T = math.log(0.5)
    logs, a = [], 0.0
    for i in range(9):
        ad.begin()
        ad.update(list(_sums(10 + i)), 70)
        logs.append(ad.log_T)
    assert len(set(logs)) == 9 and not ad.frozen
    ad.freeze()
    for x in logs:
        a = 0.9 * a + 0.1 * x
    assert ad.frozen and ad.log_T == pytest.approx(a / (1 - 0.9 ** 9), rel=1e-14)
    assert min(logs) < ad.log_T < max(logs) and ad.eps == 0.1
    # ... and the same through update(freeze=True), with the step size's dual average
    ad = TrajectoryAdaption(0.1, target_accept=0.651)
    for i in range(4):
        ad.begin()
        ad.update(list(_sums(10 + i)), 70, freeze=i == 3)
    assert ad.frozen and ad.eps == math.exp(ad.logeps_bar) and ad.eps != 0.1
    assert math.log(ad.eps) * (1 - 1e-15) <= ad.log_T <= math.log(1000 * ad.eps)
    with pytest.raises(RuntimeError):
        ad.update([1.0, 1.0, 70.0, 0.0], 70)
    T, e = ad.T, ad.eps
    ad.freeze()
    assert (ad.T, ad.eps) == (T, e)
    # directly: constant log T -> the average is that constant, whatever the count
    ad = TrajectoryAdaption(0.1, target_accept=None)
    ad.log_T = math.log(0.37)
    for i in range(5):
        ad.begin()
        ad.update([0.0, 0.0, float('inf'), 0.0], 70)                   # skipped: T stays
    ad.freeze()
    assert ad.T == pytest.approx(0.37, rel=1e-14)


def test_step_size_follows_dual_averaging_of_the_harmonic_mean():
    import nuts_ref as N
    ad = TrajectoryAdaption(0.2, target_accept=0.7, gamma=0.05, t0=10.0, kappa=0.75)
    da = N.DualAveraging(np.array([0.2]), target=0.7)
    rs = np.random.RandomState(3)
    for i in range(12):
        alpha = rs.uniform(0.2, 1.0, size=70)
        alpha[3] = 0.0 if i == 5 else alpha[3]
        out = R.sums(alpha, np.zeros(70))
        stat = 70.0 / float(out[2])
        assert stat == pytest.approx(0.0 if i == 5 else 70.0 / np.sum(1.0 / alpha), rel=1e-13)
        ad.begin()
        ad.update([float(x) for x in out], 70)
        da.update(np.array([stat]))
        assert ad.eps == pytest.approx(float(da.eps[0]), rel=1e-13), i
    ad.freeze()
    da.finalise()
    assert ad.eps == pytest.approx(float(da.eps[0]), rel=1e-13)


def test_restart_step_adaption_leaves_the_trajectory_length_alone():
    ad = TrajectoryAdaption(0.1)
    ad.log_T = math.log(0.5)
    for i in range(6):
        ad.begin()
        ad.update(list(_sums(20 + i)), 70)
    keep = (ad.log_T, ad.m2, ad.n_updates, ad.avg, ad.n_avg, ad.index, ad.eps)
    assert ad.da_t == 6 and ad.hbar != 0.0
    ad.restart_step_adaption()
    assert (ad.log_T, ad.m2, ad.n_updates, ad.avg, ad.n_avg, ad.index, ad.eps) == keep
    assert (ad.da_t, ad.hbar, ad.logeps_bar) == (0, 0.0, 0.0) and ad.mu == math.log(10.0 * ad.eps)


def test_state_dict_round_trip_continues_bit_for_bit():
    def run(ad, first, last):
        for i in range(first, last):
            ad.begin()
            ad.update(list(_sums(30 + i)), 70, freeze=i == 9)
        return ad
    whole = run(TrajectoryAdaption(0.1), 0, 12 - 2)
    for cut in (4, 10):
        part = run(TrajectoryAdaption(0.1), 0, cut)
        d = part.state_dict()
        assert all(type(v) in (float, int, bool) for v in d.values())
        other = TrajectoryAdaption(0.1)
        other.load_state_dict(d)
        run(other, cut, 10)
        assert other.state_dict() == whole.state_dict()
        w = _copy(whole)
        assert [other.begin() for _ in range(5)] == [w.begin() for _ in range(5)]


def _copy(ad):
    c = TrajectoryAdaption(0.1)
    c.load_state_dict(ad.state_dict())
    return c


OPTIMUM = 2.2467                  # tan(2x) = 2x
OPTIMUM_SPREAD = 0.1053           # max - min of sqrt(k) T over seeds 0-4 of the settings below


@pytest.mark.parametrize('k,seed', [(1.0, 5), (9.0, 6)])
def test_learnt_length_is_the_derived_optimum_on_an_isotropic_gaussian(k, seed):
    """Exact dynamics on N(0, I / k) turn every coordinate by the angle sqrt(k) tau, so the criterion
    is proportional to sin^2(sqrt(k) tau); with tau uniform on (0, T) its mean peaks where
    tan(2x) = 2x, x = sqrt(k) T = 2.2467 (the next stationary point, 4.49, is a minimum's far side).
    The restatement with a fixed small step 0.05 / sqrt(k), 256 chains x 8 dimensions, 700
    transitions from T0 = eps gives sqrt(k) T = 2.3094, 2.2084, 2.2508, 2.2041, 2.2319 over seeds 0-4
    for k = 1 and the same to four digits for k = 9 (the scheme is scale-free): spread 0.1053,
    so the band is 2.2467 +- 0.316.  Seeds 5 and 6 are run here."""
    half = 3.0 * OPTIMUM_SPREAD
    lo, hi = OPTIMUM - half, OPTIMUM + half
    eps = 0.05 / math.sqrt(k)
    assert not lo <= math.sqrt(k) * eps <= hi and not lo <= 4.49 <= hi      # or the test shows nothing
    ad = R.run_gaussian(np.full(8, 1.0 / math.sqrt(k)), 256, 700, seed, eps, target_accept=None)
    x = math.sqrt(k) * ad.T
    print('sqrt(k) T = %.4f (k = %g, seed %d), %d updates' % (x, k, seed, ad.n_updates))
    assert ad.eps == eps and ad.n_skipped == 0
    assert lo <= x <= hi


def test_abi_version_stays_and_the_new_symbols_are_bound():
    assert _native.ABI_VERSION == 7 and _native.lib().binf_abi_version() == 7
    for name in ('binf_chees_accept_prob_f64', 'binf_chees_means_f64', 'binf_chees_terms_f64',
                 'binf_chees_sums_f64', 'binf_chees_workspace_bytes'):
        assert name in _native.SIGNATURES and hasattr(_native.lib(), name)
    assert _native.CHEES_CHUNK == R.CHUNK == 64
    L = _native.lib()
    for C, D in ((1, 1), (64, 5), (65, 5), (1000, 1025), (129, 1)):
        nch = (C + 63) // 64
        assert L.binf_chees_workspace_bytes(C, D) == nch * max(2 * D, 4) * 8
    assert L.binf_chees_workspace_bytes(0, 4) == 0 and L.binf_chees_workspace_bytes(4, 0) == 0
    assert L.binf_chees_workspace_bytes(1 << 31, 4) == 0


def test_refusals_come_before_any_launch():
    """Sizes, NULL buffers and overlaps are answered on the host: the addresses are never touched."""
    L = _native.lib()
    A = [(i + 1) << 40 for i in range(10)]
    q, qp, v, al, mq, mp, g, slab, out, eb = A
    C, D = 100, 12
    assert L.binf_chees_means_f64(q, qp, al, slab, mq, mp, 0, D, None) == _native.E_ARG
    assert L.binf_chees_means_f64(q, qp, al, slab, mq, mp, C, 0, None) == _native.E_ARG
    assert L.binf_chees_means_f64(q, qp, al, None, mq, mp, C, D, None) == _native.E_ARG
    assert L.binf_chees_means_f64(q, qp, al, slab + 4, mq, mp, C, D, None) == _native.E_ARG
    assert L.binf_chees_means_f64(q, qp, al, slab, mq, mp, 1 << 31, D, None) == _native.E_UNSUPPORTED
    assert L.binf_chees_means_f64(q, qp, al, slab, mq, mp, 1 << 30, 1 << 30, None) == _native.E_UNSUPPORTED
    for bad in (dict(mq=q + 8 * (C * D - 1)), dict(mp=qp), dict(mq=mp + 8 * (D - 1)), dict(slab=q + 16),
                dict(mp=al + 8), dict(slab=mq - 8)):
        a = dict(q=q, qp=qp, al=al, slab=slab, mq=mq, mp=mp)
        a.update(bad)
        rc = L.binf_chees_means_f64(a['q'], a['qp'], a['al'], a['slab'], a['mq'], a['mp'], C, D, None)
        assert rc == _native.E_ALIAS and 'overlaps' in _native.last_error(), bad
    assert L.binf_chees_terms_f64(q, qp, v, al, mq, mp, g, C, 8193, None) == _native.E_UNSUPPORTED
    assert L.binf_chees_terms_f64(q, qp, v, al, mq, mp, None, C, D, None) == _native.E_ARG
    assert L.binf_chees_terms_f64(q, qp, v, al, mq, mp, g, -1, D, None) == _native.E_ARG
    for bad in (al + 8 * (C - 1), v + 8, mq, q + 8 * C * D - 8):
        assert L.binf_chees_terms_f64(q, qp, v, al, mq, mp, bad, C, D, None) == _native.E_ALIAS, hex(bad)
    assert L.binf_chees_sums_f64(al, g, slab, out, 0, None) == _native.E_ARG
    assert L.binf_chees_sums_f64(al, g, slab, None, C, None) == _native.E_ARG
    for s, o in ((slab, slab + 8), (al + 8, out), (slab, g + 8 * (C - 1)), (g - 8, out)):
        assert L.binf_chees_sums_f64(al, g, s, o, C, None) == _native.E_ALIAS
    assert L.binf_chees_accept_prob_f64(eb, g, al, 0, None) == _native.E_ARG
    assert L.binf_chees_accept_prob_f64(eb, None, al, C, None) == _native.E_ARG
    assert L.binf_chees_accept_prob_f64(eb, g, eb + 8, C, None) == _native.E_ALIAS        # a partial overlap
    assert L.binf_chees_accept_prob_f64(eb, g, g - 8, C, None) == _native.E_ALIAS
    with pytest.raises(ValueError):
        _native.check(_native.E_ALIAS, 'x')


def test_sampler_constructor_refusals():
    from binf_amd.samplers import ChEESSampler
    from binf_amd.samplers.chees import ChEESSampler as Direct
    assert ChEESSampler is Direct
    import torch
    x = torch.zeros((4, 3), dtype=torch.float64)
    with pytest.raises(ValueError, match='graph'):
        ChEESSampler(None, x, 0.1, graph=True)
    with pytest.raises(ValueError, match='nsteps'):
        ChEESSampler(None, x, 0.1, nsteps=5)
    with pytest.raises(TypeError):
        ChEESSampler(None, x, 0.1, bogus=1)
    with pytest.raises(ValueError):
        ChEESSampler(None, x, 0.1, target_accept=1.5)
    with pytest.raises(ValueError):
        ChEESSampler(None, x, torch.full((4,), 0.1, dtype=torch.float64))
    s = ChEESSampler(None, x, 0.1, timestep_adaption_limit=5, variable_name='x', graph=False)
    assert s.adapting and s.timestep == 0.1 and s.trajectory_length == pytest.approx(0.1) and s.nsteps == 1
    assert s.variable_name == 'x' and ChEESSampler(None, x, 0.1).variable_name == 'ChEES'
