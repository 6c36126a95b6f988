"""The host restatement ``tests/smc_ref.py`` of the tempered-SMC kernels held to exact
arithmetic (``fractions``, mpmath at 100 digits), the properties every systematic resampler
must have, the recorded yardstick of the end-to-end test, and the C ABI's side that needs
no GPU: the symbols, their bindings, the refusals."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import smc_ref as R
from smc_ref import (PATTERNS, U_EDGE, count_rule_holds, ll_sample, mean_count_rule_holds,
                     weight_pattern)
from binf_amd import _native
from conftest import ROOT

f64 = np.float64


def header_text():
    return open(os.path.join(ROOT, 'include', 'binf_hip.h')).read()


# ---------------------------------------------------------------------------
# the C ABI without a GPU
# ---------------------------------------------------------------------------
def test_symbols_are_exported_and_bound():
    L = _native.lib()
    for name in ('binf_smc_temper_f64', 'binf_smc_resample_f64', 'binf_smc_gather_f64'):
        assert name in _native.SIGNATURES
        assert getattr(L, name).argtypes == _native.SIGNATURES[name][1]
    assert L.binf_abi_version() == 7
    text = header_text()
    for name, ref, nat in (('OK', R.OK, _native.SMC_OK), ('FINISHED', R.FINISHED, _native.SMC_FINISHED),
                           ('NO_FINITE', R.NO_FINITE, _native.SMC_NO_FINITE),
                           ('INVALID', R.INVALID, _native.SMC_INVALID),
                           ('STALLED', R.STALLED, _native.SMC_STALLED), ('MAX_P', 65536, _native.SMC_MAX_P)):
        val = int(re.search(r'#define\s+BINF_SMC_%s\s+(\d+)' % name, text).group(1))
        assert val == ref == nat, name
    from binf_amd.samplers import TemperedSMC
    from binf_amd.samplers.smc import SMCResult
    assert SMCResult._fields == ('log_evidence', 'log_evidence_mean', 'stderr', 'betas', 'ess', 'n_unique',
                                 'n_stages', 'status')
    assert TemperedSMC.__init__.__code__.co_varnames[1:10] == (
        'sampler', 'beta', 'n_populations', 'ess_fraction', 'n_mutations', 'log_likelihood', 'rng',
        'variable_name', 'max_stages')


def test_refusals_come_before_any_launch():
    """Every pointer here is a made-up address: a call that got as far as a launch (or a
    host read) would fault, a refusal returns its code and the text."""
    L = _native.lib()
    p = [0x10000 * (i + 1) for i in range(12)]

    def temper(C=8, P=4, G=2, rho=0.5, nb=60, ll=p[0], beta=p[1], w=p[4], bc=p[3]):
        return L.binf_smc_temper_f64(ll, beta, C, P, G, rho, nb, p[2], bc, w, p[5], p[6], p[7], p[8], None)
    assert temper(C=-1) == _native.E_ARG
    assert temper(C=9) == _native.E_ARG
    assert temper(C=0, P=0, G=0) == _native.E_UNSUPPORTED
    assert temper(C=2 * 65537, P=65537) == _native.E_UNSUPPORTED
    assert temper(rho=0.0) == _native.E_ARG
    assert temper(rho=1.5) == _native.E_ARG
    assert temper(rho=float('nan')) == _native.E_ARG
    assert temper(nb=0) == _native.E_ARG
    assert temper(nb=129) == _native.E_ARG
    assert temper(ll=None) == _native.E_ARG
    assert temper(w=p[0] + 8) == _native.E_ALIAS
    assert temper(bc=p[4] + 56) == _native.E_ALIAS
    assert 'smc_temper' in _native.last_error()
    assert temper(C=0, P=4, G=0) == 0                       # nothing to do, nothing launched

    def resample(C=8, P=4, G=2, w=p[0], anc=p[1], nu=p[2], coff=0):
        return L.binf_smc_resample_f64(w, None, None, C, P, G, 1, 2, coff, anc, nu, None)
    assert resample(C=7) == _native.E_ARG
    assert resample(P=0, C=0) == _native.E_UNSUPPORTED
    assert resample(coff=-4) == _native.E_ARG
    assert resample(w=None) == _native.E_ARG
    assert resample(nu=None) == _native.E_ARG
    assert resample(anc=p[0] + 16) == _native.E_ALIAS
    assert resample(C=0, G=0) == 0

    def gather(C=8, D=4, x=p[0], anc=p[1], out=p[2], si=None, so=None, K=0):
        return L.binf_smc_gather_f64(x, anc, out, si, so, K, C, D, None)
    assert gather(C=-1) == _native.E_ARG
    assert gather(K=5) == _native.E_ARG
    assert gather(K=-1) == _native.E_ARG
    assert gather(anc=None) == _native.E_ARG
    assert gather(out=None) == _native.E_ARG
    assert gather(K=1, si=p[3]) == _native.E_ARG
    assert gather(out=p[0]) == _native.E_ALIAS
    assert gather(out=p[0] + 8 * 31) == _native.E_ALIAS
    assert gather(K=2, si=p[3], so=p[3] + 8 * 15) == _native.E_ALIAS
    assert gather(out=p[1] - 8) == _native.E_ALIAS          # out runs into the ancestors
    assert 'smc_gather' in _native.last_error()
    assert gather(C=0) == 0
    assert gather(D=0, x=None, out=None) == 0


# ---------------------------------------------------------------------------
# THE SUM and the weights against exact arithmetic
# ---------------------------------------------------------------------------
def exact_sum(x):
    return sum(Fraction(float(v)) for v in x)


@pytest.mark.parametrize('P', [1, 2, 64, 255, 256, 257, 1000, 4096])
def test_block_sum_against_fractions(P):
    """Each addition rounds a partial sum <= the total by half an ulp; the longest path has
    sum_depth(P) additions."""
    rs = np.random.RandomState(P)
    x = rs.uniform(size=P) ** 8
    got, want = R.block_sum(x), exact_sum(x)
    assert abs(Fraction(float(got)) - want) <= Fraction(R.sum_depth(P) * 0.5 * R.EPS) * want


def test_block_sum_order_is_the_headers():
    """Inputs whose sum depends on the order: a thread adds its terms j, j + 256, ... one after
    the other (1 + 2^-53 + 2^-53 stays 1), neighbouring lanes join as a tree ((1 + 0) + (2^-53 +
    2^-53) is 1 + 2^-52), the waves one after the other."""
    h = 2.0 ** -53
    x = np.zeros(768)
    x[0], x[256], x[512] = 1.0, h, h
    assert R.block_sum(x) == 1.0
    x = np.zeros(4)
    x[:] = 1.0, 0.0, h, h
    assert R.block_sum(x) == 1.0 + 2.0 * h
    x = np.zeros(256)
    x[0], x[64], x[128] = 1.0, h, h
    assert R.block_sum(x) == 1.0


@pytest.mark.parametrize('P', [2, 64, 257, 4096])
def test_restatement_ess_against_mpmath(P):
    """ESS of the restatement at a step against 100-digit arithmetic, inside ess_bound(sides=1)
    (derivation: smc_ref.sum_bounds / ess_bound)."""
    import mpmath
    ll = ll_sample(P, 'holes', 3 * P)
    for d in (1.0, 0.37, 2.0 ** -7):
        m, e = R.shifted(ll)
        w, s1, s2, ess = R.sums(e, d)
        assert np.all(w[~np.isfinite(ll)] == 0.0)
        exact = R.exact_ess(ll, d)
        assert abs(mpmath.mpf(float(ess)) - exact) <= R.ess_bound(P, s1, s2, sides=1)


@pytest.mark.parametrize('P,beta,n_bisect', [(2, 0.0, 60), (64, 0.0, 60), (257, 0.25, 60), (4096, 0.0, 60),
                                             (257, 0.0, 20)])
def test_restatement_step_brackets_the_exact_root(P, beta, n_bisect):
    """The discrete choice of the restatement, as the GPU test asks of the device: with exact
    arithmetic ESS(delta) >= rho P - eps and ESS(delta + hi0 2^-n) <= rho P + eps, eps =
    ess_bound(sides=1) + slope_bound * 2^-52 * hi0 + 2^-53 rho P (the rounding of rho * P)."""
    import mpmath
    ll = ll_sample(P, 'plain', 11 * P)
    rho = 0.5
    t = R.temper(ll, beta, rho, n_bisect)
    if P == 2:
        assert t['status'] == R.OK and t['beta'] == 1.0      # ESS >= 1 = rho P at any step
        return
    assert t['status'] == R.OK and 0.0 < t['delta'] < 1.0 - beta
    m, e = R.shifted(ll)
    _, s1, s2, _ = R.sums(e, t['delta'])
    hi0 = 1.0 - beta
    eps = R.ess_bound(P, s1, s2, sides=1) + R.slope_bound(P, e) * R.EPS * hi0 + 0.5 * R.EPS * rho * P
    d = mpmath.mpf(float(t['delta']))
    assert R.exact_ess(ll, d) >= rho * P - eps
    assert R.exact_ess(ll, d + mpmath.mpf(hi0) * mpmath.mpf(2) ** -n_bisect) <= rho * P + eps
    assert eps < 1e-6 * P


def test_restatement_status_paths():
    ll = np.array([0.0, -1.0, -2.0, -np.inf])
    assert R.temper(ll, 1.0, 0.5)['status'] == R.FINISHED
    assert R.temper(np.array([0.0, np.inf, np.nan]), 0.0, 0.5)['status'] == R.INVALID
    none = R.temper(np.array([-np.inf, np.nan, -np.inf]), 0.0, 0.5)
    assert none['status'] == R.NO_FINITE and none['n_invalid'] == 1 and np.all(none['w'] == 1.0)
    st = R.temper(np.array([0.0] + [-1e30] * 7), 0.0, 0.5)
    assert st['status'] == R.STALLED and st['delta'] == 2.0 ** -60 and st['beta'] == 2.0 ** -60
    last = R.temper(np.array([0.0, -0.1, -0.2, -0.3]), 0.75, 0.5)
    assert last['status'] == R.OK and last['beta'] == 1.0 and last['delta'] == 0.25


# ---------------------------------------------------------------------------
# systematic resampling
# ---------------------------------------------------------------------------


@pytest.mark.parametrize('P', [1, 2, 63, 64, 65, 255, 256, 257, 1000, 4096])
def test_restatement_resampling_properties(P):
    for k, kind in enumerate(PATTERNS):
        w = weight_pattern(P, kind, 100 * P + k)
        cs = R.prefix_sums(w)
        # the prefix sums against exact arithmetic, and flat wherever the weight is 0
        run = Fraction(0)
        for i in range(P):
            run += Fraction(float(w[i]))
            assert abs(Fraction(float(cs[i])) - run) <= Fraction((P // 256 + 258) * R.EPS) * run
        assert np.all(np.diff(cs) >= 0.0)
        assert np.all(np.diff(np.concatenate([[0.0], cs]))[w == 0.0] == 0.0)
        for u in U_EDGE:
            a, n_unique = R.resample(w, u)
            assert np.all(np.diff(a) >= 0) and a.min() >= 0 and a.max() < P
            assert np.all(w[a] > 0.0)
            assert n_unique == len(set(a.tolist()))
            assert count_rule_holds(w, a)


@pytest.mark.parametrize('P', [63, 257, 1000])
def test_restatement_mean_counts_are_unbiased(P):
    w = weight_pattern(P, 'zero_runs', 5 * P)
    us = np.random.RandomState(P).uniform(size=256)
    rows = np.stack([R.resample(w, u)[0] for u in us])
    assert mean_count_rule_holds(w, rows)
    # the bound has teeth: a resampler whose targets sit half a slot late fails it
    late = np.stack([np.minimum(np.searchsorted(R.prefix_sums(w), R.targets(P, min(u + 0.5, 0.999), w.sum()),
                                                side='right'), P - 1) for u in us])
    assert not mean_count_rule_holds(w, late)


# ---------------------------------------------------------------------------
# the yardstick of the end-to-end test
# ---------------------------------------------------------------------------
def test_end_to_end_yardstick_is_the_recorded_one():
    """200 seeds of the whole-loop restatement: the sd the GPU test's tolerance is built from
    (recorded in smc_ref.E2E_SD), and the control's miss."""
    assert abs(R.e2e_analytic() - (-8.98987)) < 1e-5
    y = R.e2e_yardstick(200)
    assert abs(y['sd'] - R.E2E_SD) <= 0.05 * R.E2E_SD
    assert y['stages_max'] <= 12
    bound = R.e2e_bound()
    assert abs(y['mean'] - R.e2e_analytic()) <= bound
    assert abs(y['control_mean'] - R.e2e_analytic()) > 10.0 * bound
