"""CPU tests of the generalised-linear error models: the host restatement of the term
(tests/glm_ref.py) against 50-digit arithmetic within the derived bound (tests/glm_bounds.py),
its overflow behaviour, the models' constructors and plumbing, the registry, and the host-side
refusals of the C entry points (decided before any launch)."""
import math

import numpy as np
import pytest

import glm_bounds as G
import glm_ref as R
import grad_bounds as GB
from binf_amd import _native, native
from binf_amd.model import glm, linear
from binf_amd.model.glm import BinomialLogitErrorModel, PoissonLogErrorModel

ETAS = [0.0, 2.0 ** -60, -2.0 ** -60, 1.0, -1.0, 36.7, -36.7, 40.0, -40.0, 708.0, -708.0, 745.0, -745.0]
BINOMIAL_DATA = [(0.0, 1.0), (1.0, 1.0), (0.0, 7.0), (3.0, 7.0), (7.0, 7.0)]
POISSON_DATA = [(0.0, 1.0), (1.0, 1.0), (5.0, 1.0), (40.0, 1.0)]


def _grid(family):
    etas = ETAS + ([800.0, -800.0] if family == R.BINOMIAL_LOGIT else [])
    data = BINOMIAL_DATA if family == R.BINOMIAL_LOGIT else POISSON_DATA
    return [(e, y, m) for e in etas for y, m in data]


@pytest.mark.parametrize('family', R.FAMILIES)
def test_restatement_against_truth(family):
    """glm_ref's ll (numpy, the kernel's expressions in its order) against mpmath at 50 digits
    on the eta grid, within glm_bounds' per-datum bound for an exact eta (delta = 0)."""
    worst = 0.0
    for eta, y, m in _grid(family):
        ll, _ = R.term(family, eta, y, m)
        B, _, _, _ = G.term_bounds(family, np.float64(eta), 0.0, y, m)
        e = G.err(ll, R.exact_ll(family, eta, y, m)) if np.isfinite(ll) else 0.0
        if not np.isfinite(ll):
            assert family == R.POISSON_LOG and eta > 709.78, (eta, y, m)
            continue
        assert e <= B, (family, eta, y, m, e, float(B))
        worst = max(worst, e / float(B))
    print('largest fraction of the bound: %.3f' % worst)
    assert worst > 0.0          # a bound that nothing comes near shows nothing


@pytest.mark.parametrize('family', R.FAMILIES)
def test_gradient_against_high_precision_differences(family):
    """g equals -d ll / d eta from mpmath central differences at 50 digits, to the bound; the
    differences agree with the closed form far inside it."""
    for eta, y, m in _grid(family):
        _, g = R.term(family, eta, y, m)
        if not np.isfinite(g):
            assert family == R.POISSON_LOG and eta > 709.78
            continue
        _, rho, _, _ = G.term_bounds(family, np.float64(eta), 0.0, y, m)
        want = R.exact_g_by_differences(family, eta, y, m)
        closed = R.exact_g(family, eta, y, m)
        scale = max(1.0, float(abs(closed)))
        assert float(abs(want - closed)) <= 1e-25 * scale * max(1.0, abs(eta)) ** 2, (eta, y, m)
        assert G.err(g, want) <= float(rho) + 1e-25 * scale * max(1.0, abs(eta)) ** 2, (family, eta, y, m)


def test_overflow_behaviour():
    """A Poisson eta beyond 709.78 gives ll = -inf exactly and g = +inf, never NaN, for y >= 0; a
    binomial term stays finite for every finite eta.  (y eta itself must be a double: at
    y eta > 1.8e308 the expression's inf - inf is NaN, as for any model of this form.)"""
    for eta in (709.79, 745.0, 1e4, 1e300):
        for y in (0.0, 1.0, 1e6):
            ll, g = R.term(R.POISSON_LOG, eta, y)
            assert ll == -np.inf and g == np.inf, (eta, y, ll, g)
    for eta in (709.78, -745.0, -1e4):
        for y in (1.0, 1e6):
            ll, g = R.term(R.POISSON_LOG, eta, y)
            assert np.isfinite(ll) and np.isfinite(g), (eta, y)
    big = np.finfo(np.float64).max
    for eta in (0.0, 745.0, -745.0, 800.0, -800.0, 1e300, -1e300, big / 8.0, -big / 8.0):
        for y, m in BINOMIAL_DATA:
            ll, g = R.term(R.BINOMIAL_LOGIT, eta, y, m)
            assert np.isfinite(ll) and np.isfinite(g), (eta, y, m)
            assert ll <= 0.0 and -y <= g <= m - y


def test_bounds_self_test():
    """numpy's own results lie inside the bounds; a moved mock datum, a dropped m and a flipped
    force lie outside them."""
    figs = G.self_test()
    assert len(figs) == 4
    for f in figs:
        assert f['lp'] <= 1.0 and f['force'] <= 1.0 and f['moved'] > 1.0 and f['flipped'] > 1.0, f


def _em(family, ys, m, off):
    return BinomialLogitErrorModel(ys, m, off) if family == R.BINOMIAL_LOGIT else PoissonLogErrorModel(ys, off)


def test_table_restatement_and_cases_reach_every_row():
    """The host restatement of the dispatch tables at every K, and the rows the generated cases
    reach: all thirteen at CT = 1 and all thirteen at CT = 2."""
    want = {1: (1, 0), 4: (1, 0), 5: (2, 0), 8: (2, 0), 9: (4, 0), 16: (4, 0), 17: (4, 1), 18: (4, 2), 19: (8, 0),
            32: (8, 0), 33: (8, 1), 34: (8, 2), 35: (9, 0), 36: (9, 0), 37: (12, 0), 48: (12, 0), 49: (12, 1),
            50: (12, 2), 51: (16, 0), 64: (16, 0)}
    assert sorted(want) == sorted(GB.K_LIST)
    for K, row in want.items():
        assert G.table_row(K) == row
    for K in range(1, 65):
        KS, KV = G.table_row(K)
        assert 4 * KS + KV >= K and (KV == 0 or 4 * KS + KV == K), K      # no coefficient left out
    assert len(set(G.TABLE_ROWS)) == 13
    reached = set((G.table_row(K), G.chain_tiles(C)) for K, N, C in G.force_cases())
    assert reached == set((row, ct) for row in G.TABLE_ROWS for ct in (1, 2))
    for K, N, C in G.force_cases():
        assert N <= 2049 and C <= 4113 and len(G.exact_chains(C, N)) <= 6


@pytest.mark.parametrize('K', GB.K_LIST)
def test_a_dropped_coefficient_leaves_the_bound(K):
    """What makes a wrong row of a dispatch table visible to the GPU test, checked here: numpy's
    own log-prob and force of every generated case of this K with the last coefficient dropped,
    and with each coefficient of the VALU tail dropped, lie outside the exact bound on one of the
    chains the GPU test compares exactly -- both families, with and without trials and offset."""
    least = np.inf
    for Kc, N, C in G.force_cases():
        if Kc != K:
            continue
        for family in R.FAMILIES:
            for extras in (True, False):
                for k, (a, b) in G.dropped_visibility(family, K, N, C, extras).items():
                    assert a > 1.0 and b > 1.0, (family, K, N, C, extras, k, a, b)
                    least = min(least, a, b)
    print('K = %d: the least multiple of the bound a dropped coefficient reaches: %.3g' % (K, least))
    assert np.isfinite(least)


@pytest.mark.parametrize('family', R.FAMILIES)
def test_edge_ladder_on_the_host(family):
    """The checks the GPU test applies to the device's values, applied to numpy's restatement: it
    lies inside every bound that is asserted, the overflowed Poisson data fall as stated, and the
    number of edges asserted is the length of the ladder."""
    ladder = G.edge_ladder()
    assert len(ladder) == 32 and len(set(ladder)) == 31 and 0.0 in ladder      # +-0.0 are one value
    lo, hi = G._either_side(53 * R.mp().log(2))
    assert 1.0 + math.exp(-lo) > 1.0 and 1.0 + math.exp(-hi) == 1.0 and 36.73 < lo < hi < 36.74
    with np.errstate(over='ignore'):
        assert math.exp(G.exp_max()) < np.inf and np.exp(np.nextafter(G.exp_max(), np.inf)) == np.inf
    data = G.edge_case(family, 1)
    A, ys, m, off, theta = data
    assert theta.shape == (32, 1) and A.shape == (1, 17) and 1.0 in A[0]
    eta = G.edge_eta(data)
    # the mock tensor carries each edge as the ladder has it, the sign of -0.0 included
    assert ladder[0] == 0.0 and ladder[1] == 0.0 and not np.signbit(ladder[0]) and np.signbit(ladder[1])
    assert not np.signbit(eta[0]).any() and np.signbit(eta[1]).all()
    assert np.array_equal(np.signbit(eta), np.repeat(np.signbit(theta), 17, axis=1))
    assert G._same_bits(eta[:, A[0] == 1.0], np.repeat(theta, int((A[0] == 1.0).sum()), axis=1))
    assert not G._same_bits(eta[0], eta[1])
    ll, g = R.term(family, eta, ys, m)
    fig = G.edge_pointwise_check(family, data, eta, ll, g)
    print('pointwise', fig)
    assert fig['edges'] == len(ladder)
    assert (fig['overflowed'] > 0) == (family == R.POISSON_LOG)
    # a mock tensor that lost the sign of zero (a matrix product's +0.0 accumulator) is refused
    with np.errstate(all='ignore'), pytest.raises(AssertionError):
        G.edge_pointwise_check(family, data, theta.dot(A), ll, g)
    for variant in (1, 2, 3):
        data = G.edge_case(family, variant)
        A, ys, m, off, theta = data
        ln = _em(family, ys, m, off).log_norm
        with np.errstate(all='ignore'):
            ll, g = R.term(family, G.edge_eta(data), ys, m)
            lp, grad = R.sum_in_kernel_order(ll, ln), g.dot(A.T)
        fig = G.edge_chain_check(family, data, ln, lp, grad)
        print('variant', variant, fig)
        want = G.edge_counts(family, data)
        assert (fig['edges'], fig['full'], fig['overflowed'], fig['pointwise_only']) == want
        assert fig['edges'] + fig['pointwise_only'] == len(ladder) and fig['full'] >= 20
        assert (fig['pointwise_only'] > 0) == (family == R.POISSON_LOG and variant == 3)
        assert len(G.edge_moderate_chains(data)) >= 16
        # a sign lost at zero, or one rounding more at an edge, leaves the bound
        if variant == 1 and family == R.BINOMIAL_LOGIT:
            bad = g.copy()
            bad[0] = -bad[0]
            with pytest.raises(AssertionError):
                G.edge_pointwise_check(family, data, eta, ll, bad)


def test_underflow_allowance_carries_the_trial_count():
    """The case that set the binomial bound's underflow term: eta the double just below
    -1075 log 2 (t = exp(-|eta|) rounds up to the smallest subnormal, twice its true value),
    y = 0, m = 2**20.  ll = -m log1p(t) is then m TINY / 2 off whatever the library: outside the
    bound with a flat 4 TINY (right for m = 1), inside it with (2 m + 2) TINY."""
    eta = -G._either_side(1075 * R.mp().log(2))[0]
    y, m = 0.0, 2.0 ** 20
    assert math.exp(eta) == G.TINY and R.mp().exp(eta) < R.mp().mpf(G.TINY) * 0.75
    ll, _ = R.term(R.BINOMIAL_LOGIT, eta, y, m)
    e = G.err(ll, R.exact_ll(R.BINOMIAL_LOGIT, eta, y, m))
    B, _, mag, _ = G.term_bounds(R.BINOMIAL_LOGIT, np.float64(eta), 0.0, y, m)
    flat = float(B) - (2 * m + 2 - 4) * G.TINY
    assert 0.0 < flat <= 5 * G.TINY
    assert e > 1e4 * flat and e > float(G.pointwise_bound(flat, mag, None))
    assert e <= float(B) and e <= float(G.pointwise_bound(B, mag, None))


def test_kernel_order_sum_is_a_sum():
    rs = np.random.RandomState(3)
    for N in (1, 15, 16, 17, 1024, 1025, 2049):
        x = rs.standard_normal((2, N)) * 2.0 ** rs.randint(-8, 9, size=(2, N))
        got = R.sum_in_kernel_order(x, 0.5)
        for c in range(2):
            want = math.fsum(x[c]) + 0.5
            assert abs(got[c] - want) <= G.gamma(N + 1) * float(np.sum(np.abs(x[c])) + 0.5)


# ---------------------------------------------------------------------------
# the models
# ---------------------------------------------------------------------------
def test_constructor_refusals():
    for bad in ([0.5, 1.0], [-1.0, 0.0], [float('nan'), 1.0]):
        with pytest.raises(ValueError):
            BinomialLogitErrorModel(bad)
        with pytest.raises(ValueError):
            PoissonLogErrorModel(bad)
    with pytest.raises(ValueError):
        BinomialLogitErrorModel([0, 2])                       # ys > trials (one trial each)
    with pytest.raises(ValueError):
        BinomialLogitErrorModel([0, 3], trials=[1, 2])
    with pytest.raises(ValueError):
        BinomialLogitErrorModel([0, 0], trials=[1, 0])        # trials < 1
    with pytest.raises(ValueError):
        BinomialLogitErrorModel([0, 1], trials=[1.5, 2])
    with pytest.raises(ValueError):
        BinomialLogitErrorModel([0, 1], trials=[1, 2, 3])     # shapes that disagree
    with pytest.raises(ValueError):
        BinomialLogitErrorModel([0, 1], offset=[0.0])
    with pytest.raises(ValueError):
        PoissonLogErrorModel([0, 1, 2], offset=[0.0, 1.0])
    with pytest.raises(ValueError):
        PoissonLogErrorModel([[0, 1], [2, 3]])
    m = BinomialLogitErrorModel([0, 1, 1])
    assert m.trials is None and m.offset is None and sorted(m.variables) == ['mock_data']
    assert PoissonLogErrorModel([0, 7], offset=[0.1, 0.2]).trials is None


def test_log_norm_against_truth():
    rs = np.random.RandomState(5)
    trials = rs.randint(1, 60, size=40).astype(np.float64)
    ys = np.floor(rs.uniform(size=40) * (trials + 1)).clip(0, trials)
    b = BinomialLogitErrorModel(ys, trials)
    p = PoissonLogErrorModel(ys)
    M = R.mp()
    for model, family in ((b, R.BINOMIAL_LOGIT), (p, R.POISSON_LOG)):
        want = R.exact_log_norm_terms(family, ys, trials)
        for got, w, y, m in zip(model.pointwise_constants, want, ys, trials):
            parts = (m + 1, y + 1, m - y + 1) if family == R.BINOMIAL_LOGIT else (y + 1,)
            allow = sum(G.lgamma_bound(x) for x in parts) + 2 * G.U * sum(abs(math.lgamma(x)) for x in parts)
            assert G.err(got, w) <= allow, (family, y, m)
        total = M.fsum(M.mpf(float(v)) for v in model.pointwise_constants)
        assert G.err(model.log_norm, total) <= G.U * float(abs(total))
    assert BinomialLogitErrorModel([0, 1, 1, 0]).log_norm == 0.0      # unit trials: log C = 0
    assert PoissonLogErrorModel([0, 1, 1, 0]).log_norm == 0.0


def test_native_spec_and_clone():
    b = BinomialLogitErrorModel([0, 1, 2], trials=[1, 1, 3], offset=[0.0, 0.5, -0.5])
    p = PoissonLogErrorModel([0, 1, 2], offset=[0.0, 0.5, -0.5])
    assert b.native_spec() == ('binomial_logit', b) and p.native_spec() == ('poisson_log', p)
    assert b.family == _native.GLM_BINOMIAL_LOGIT and p.family == _native.GLM_POISSON_LOG
    for model in (b, p):
        c = model.clone()
        assert type(c) is type(model) and c is not model
        assert c._dev is model._dev                    # device data shared with clones
        assert np.array_equal(c.ys, model.ys) and c.log_norm == model.log_norm
        assert c.native_spec()[0] == model.kind

    class MyLogProb(BinomialLogitErrorModel):
        def _evaluate_log_prob(self, mock_data):
            return mock_data.sum(-1)

    class MyGradient(PoissonLogErrorModel):
        def _evaluate_gradient(self, mock_data):
            return mock_data

    class Untouched(PoissonLogErrorModel):
        pass

    assert MyLogProb([0, 1]).native_spec() is None
    assert MyGradient([0, 1]).native_spec() is None
    assert Untouched([0, 1]).native_spec()[0] == 'poisson_log'
    assert MyLogProb([0, 1]).clone().native_spec() is None


def test_registry():
    """The new pairs resolve; ('linear', 'gaussian') resolves to what it resolved to before; the
    'linear' kind is consulted before 'linear_glm'."""
    assert native.likelihood_hooks('linear', 'binomial_logit') == (glm.log_prob, glm.gradient)
    assert native.likelihood_hooks('linear', 'poisson_log') == (glm.log_prob, glm.gradient)
    assert native.likelihood_hooks('linear', 'gaussian') == (linear.log_prob, linear.gradient)
    assert native.likelihood_hooks('polynomial', 'binomial_logit') is None
    names = [k.name for k in native.kinds()]
    assert names.index('linear') < names.index('linear_glm')
    assert native.get('linear').match_leapfrog is linear.posterior_leapfrog_spec
    assert native.get('linear').leapfrog is linear.leapfrog
    assert native.get('linear_glm').match_leapfrog is glm.posterior_leapfrog_spec


def test_log_prob_hook_declines_where_the_grid_leaves_the_chip_idle():
    """One workgroup per piece of 1024 points and per 64 (128 from 4096 on) chains: fused from
    256 workgroups (binomial) / 128 (Poisson) on, as written below (DESIGN 4.7's measurements)."""
    b, p = glm.BINOMIAL_LOGIT, glm.POISSON_LOG
    assert glm.logp_covers(b, 4096, 8192) and not glm.logp_covers(b, 4096, 4096)
    assert glm.logp_covers(p, 4096, 4096) and not glm.logp_covers(p, 4096, 2048)
    assert glm.logp_covers(b, 4095, 4096) and not glm.logp_covers(b, 4096, 7168)
    assert glm.logp_covers(b, 8192, 16384) and glm.logp_covers(p, 512, 16384) and not glm.logp_covers(b, 512, 16384)
    assert not glm.logp_covers(b, 1, 1) and not glm.logp_covers(p, 512, 24)


def _posterior(em, prior=True, second=False, variable='coefficients'):
    from binf_amd.pdf import IsotropicGaussian
    from binf_amd.pdf.likelihoods import Likelihood
    from binf_amd.pdf.posteriors import Posterior
    fwm = linear.LinearForwardModel('covariates', np.ones((2, len(em.ys))), variable=variable)
    priors = {}
    if prior:
        priors['prior'] = IsotropicGaussian(0.25, 0.5, name='prior', variable_name=variable)
    if second:
        priors['prior2'] = IsotropicGaussian(1.0, 0.0, name='prior2', variable_name=variable)
    return Posterior({'lik': Likelihood('lik', fwm, em)}, priors)


def test_leapfrog_matching_on_the_host():
    """Recognition needs no device: one GLM likelihood and at most one isotropic Gaussian on the
    same variable; the Gaussian 'linear' posteriors still go to their own kind."""
    from binf_amd.example.likelihood import GaussianErrorModel
    b = BinomialLogitErrorModel([0, 1, 1])
    spec = _posterior(b).native_leapfrog_spec('coefficients')
    assert spec[0] == 'linear_glm' and spec[2] is b and spec[1].native_spec()[0] == 'linear'
    assert spec[3] == (0.25, 0.5)
    spec = _posterior(PoissonLogErrorModel([0, 1, 4]), prior=False).native_leapfrog_spec('coefficients')
    assert spec[0] == 'linear_glm' and spec[3] is None
    assert _posterior(b, second=True).native_leapfrog_spec('coefficients') is None
    assert _posterior(b).native_leapfrog_spec('something_else') is None
    assert _posterior(b).native_hmc_spec('coefficients') is None

    class Mine(BinomialLogitErrorModel):
        def _evaluate_gradient(self, mock_data):
            return mock_data

    assert _posterior(Mine([0, 1, 1])).native_leapfrog_spec('coefficients') is None
    g = GaussianErrorModel(np.zeros(3))
    post = _posterior_gauss(g)
    assert post.native_leapfrog_spec('coefficients')[0] == 'linear'


def _posterior_gauss(em):
    from binf_amd.pdf.likelihoods import Likelihood
    from binf_amd.pdf.posteriors import Posterior
    fwm = linear.LinearForwardModel('covariates', np.ones((2, 3)))
    lik = Likelihood('lik', fwm, em)
    post = Posterior({'lik': lik}, {})
    return post.conditional_factory(precision=2.0)


# ---------------------------------------------------------------------------
# host-side refusals of the C entry points: decided before anything is launched or touched
# ---------------------------------------------------------------------------
def test_refusals_without_gpu():
    L = _native.lib()
    base = 1 << 40
    th, A, ys, tr, off, out, ws, q, p = (base + (i << 34) for i in range(9))
    C, K, N = 5, 3, 2049
    need = L.binf_linear_glm_logp_workspace_bytes(C, K, N)
    assert need == 3 * C * 8 and L.binf_linear_glm_logp_workspace_bytes(C, K, 1024) == 0
    assert L.binf_linear_glm_logp_workspace_bytes(C, K, 1025) == 2 * C * 8

    def logp(th_=th, A_=A, ys_=ys, fam=0, out_=out, ws_=ws, wb=need, K_=K, C_=C, N_=N):
        return L.binf_linear_glm_logp_f64(th_, A_, ys_, tr, off, fam, 0.0, out_, ws_, wb, C_, K_, N_, None)
    assert logp(fam=2) == _native.E_ARG and 'family' in _native.last_error()
    assert logp(fam=-1) == _native.E_ARG
    assert logp(th_=None) == _native.E_ARG and logp(ys_=None) == _native.E_ARG
    assert logp(out_=None) == _native.E_ARG and logp(A_=None) == _native.E_ARG
    assert logp(ws_=None) == _native.E_ARG and 'workspace' in _native.last_error()
    assert logp(wb=need - 8) == _native.E_ARG
    assert logp(K_=65) == _native.E_UNSUPPORTED
    assert logp(C_=65535 * 64 + 1, wb=1 << 60) == _native.E_UNSUPPORTED
    assert logp(N_=(1 << 31) - 16, wb=1 << 60) == _native.E_UNSUPPORTED
    assert logp(out_=th + 8) == _native.E_ALIAS and logp(out_=tr) == _native.E_ALIAS
    assert logp(ws_=out - 8) == _native.E_ALIAS and logp(ws_=off) == _native.E_ALIAS
    with pytest.raises(ValueError):
        _native.check(logp(fam=7), 'x')
    with pytest.raises(NotImplementedError):
        _native.check(logp(K_=65), 'x')

    C = 17
    gneed = L.binf_linear_glm_grad_workspace_bytes(C, K, N)
    assert gneed == 64 * C * K * 8                       # the Gaussian gradient's splits
    assert gneed == L.binf_poly_gauss_grad_workspace_bytes(C, K, N)
    for c, n in ((1, 1), (17, 35), (4096, 1024), (4113, 17), (8192, 16384)):
        assert L.binf_linear_glm_grad_workspace_bytes(c, K, n) == L.binf_poly_gauss_grad_workspace_bytes(c, K, n)
        assert L.binf_linear_glm_leapfrog_workspace_bytes(c, K, n) == L.binf_poly_leapfrog_workspace_bytes(c, K, n)

    def grad(th_=th, fam=1, out_=out, ws_=ws, wb=gneed, K_=K):
        return L.binf_linear_glm_grad_f64(th_, A, ys, tr, off, fam, out_, ws_, wb, C, K_, N, None)
    assert grad(fam=5) == _native.E_ARG and grad(th_=None) == _native.E_ARG and grad(out_=None) == _native.E_ARG
    assert grad(ws_=None) == _native.E_ARG and grad(wb=gneed - 8) == _native.E_ARG
    assert grad(K_=65) == _native.E_UNSUPPORTED
    assert grad(out_=th + 16) == _native.E_ALIAS and grad(ws_=out + 8) == _native.E_ALIAS

    lneed = L.binf_linear_glm_leapfrog_workspace_bytes(C, K, N)

    def leap(q_=q, p_=p, fam=0, hp=1, ws_=ws, wb=lneed, nsteps=3, mode=0, K_=K):
        return L.binf_linear_glm_leapfrog_f64(q_, p_, A, ys, tr, off, fam, hp, 1.0, 0.0, ws_, wb, C, K_, N,
                                              0.1, None, nsteps, mode, None)
    assert leap(fam=3) == _native.E_ARG and leap(hp=2) == _native.E_ARG and leap(nsteps=0) == _native.E_ARG
    assert leap(mode=9) == _native.E_ARG and leap(q_=None) == _native.E_ARG and leap(ws_=None) == _native.E_ARG
    assert leap(wb=lneed - 8) == _native.E_ARG
    assert leap(K_=65) == _native.E_UNSUPPORTED
    assert leap(p_=q + 8) == _native.E_ALIAS and leap(ws_=p + 8) == _native.E_ALIAS and leap(q_=A + 8) == _native.E_ALIAS

    S = 4

    def point(mock=th, ll=out, g=ws, fam=0, S_=S, N_=N, ys_=ys):
        return L.binf_glm_pointwise_f64(mock, ys_, tr, off, None, fam, ll, g, S_, N_, None)
    assert point(ll=None, g=None) == _native.E_ARG and 'no output' in _native.last_error()
    assert point(fam=2) == _native.E_ARG and point(mock=None) == _native.E_ARG and point(ys_=None) == _native.E_ARG
    assert point(S_=-1) == _native.E_ARG
    assert point(N_=(1 << 31) - 1) == _native.E_UNSUPPORTED
    assert point(S_=1 << 40, N_=1 << 20) == _native.E_UNSUPPORTED
    assert point(ll=th + 8) == _native.E_ALIAS and point(g=out + 8) == _native.E_ALIAS
    assert point(S_=0) == 0 and point(N_=0) == 0
