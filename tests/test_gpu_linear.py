"""The linear forward model and its kind ``'linear'`` on the GPU
(``binf_linear_forward_f64``, ``binf_linear_gauss_logp_f64``, and the gradient / leapfrog
kernels the kind shares with the polynomial one).

Every tolerance is a DERIVED bound (tests/linear_bounds.py, tests/poly_bounds.py): the
error-free value comes from exact integer arithmetic on the doubles (and mpmath's log),
the bound from the number of roundings.  Chains that are not compared with exact
arithmetic are compared with numpy's float64 result within twice the bound, numpy's own
result being inside it."""
import os

import numpy as np
import pytest
import torch

import linear_bounds as LB
import poly_bounds as PB
from binf_amd import _native
from binf_amd.example.likelihood import POLYVAL, ForwardModel, GaussianErrorModel
from binf_amd.example.priors import GammaPrior, GaussianPrior
from binf_amd.example.samplers import make_hmc_sampler
from binf_amd.model.linear import LinearForwardModel
from binf_amd.pdf.likelihoods import Likelihood
from binf_amd.pdf.posteriors import Posterior
from binf_amd.samplers import BinfState
from binf_amd.samplers.hmc import HMCSampler
from binf_amd.samplers.rng import DeviceRNG
from conftest import GOLDEN_DIR, load_golden
from test_gpu_guards import Guarded, plain

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (4, 20, 5), (7, 37, 3), (33, 1000, 20), (33, 16384, 130), (36, 129, 3),
          (64, 320, 9), (17, 50, 2100), (33, 1024, 4097)]


def dev_t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device)


def make_likelihood(A, ys, cls=LinearForwardModel):
    return Likelihood('points', cls('basis', A), GaussianErrorModel(ys))


def exact_chains(C):
    """First, last, one in the last (ragged) 16-chain tile, one in a middle tile."""
    if C <= 4:
        return list(range(C))
    tiles = (C + 15) // 16
    last_tile = 16 * (tiles - 1)
    middle = min(C - 1, 16 * (tiles // 2) + 5)
    chains = {0, C - 1, min(C - 1, last_tile + (C - 1 - last_tile) // 2), middle}
    c = 1
    while len(chains) < 4:                    # few tiles: the picks coincide, take neighbours
        chains.add(c)
        c += 1
    return sorted(chains)


def random_case(K, N, C, seed=None):
    rs = np.random.RandomState(1000 * K + N + 7 * C if seed is None else seed)
    A = rs.standard_normal((K, N))                       # dense, not Vandermonde
    truth = rs.standard_normal(K)
    ys = truth.dot(A) + 0.3 * rs.standard_normal(N)
    theta = truth + 0.2 * rs.standard_normal((C, K))
    tau = rs.uniform(0.5, 4.0, size=C)
    return A, ys, theta, tau


# ---------------------------------------------------------------------------
# 1. the reference's own fixtures
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['k4_n20', 'k7_n37', 'k33_n1000'])
def test_reference_fixtures(device, name):
    z = load_golden(os.path.join(GOLDEN_DIR, 'ref_example_models_%s.npz' % name))
    A, ys, theta, tau = z['jacobi'], z['ys'], z['theta'], z['precision']
    C, K = theta.shape
    N = len(ys)
    lik = make_likelihood(A, ys)
    th, tt = dev_t(theta, device), dev_t(tau, device)
    lp = lik.log_prob(coefficients=th, precision=tt).cpu().numpy()
    mock = lik.forward_model(coefficients=th).cpu().numpy()
    assert mock.shape == (C, N)
    ex = LB.Exact(A, ys)
    for c in range(C):
        info = ex.chain(theta[c])
        want, bound = LB.logp_exact_and_bound(info['chi2'], info['chi2_bound'], tau[c], N)
        err = LB.logp_error(lp[c], want)
        print('%s chain %d: log-prob error %.3g, bound %.3g' % (name, c, err, bound))
        assert err <= bound, (c, err, bound)
        assert abs(lp[c] - z['error_logp'][c]) <= 2 * bound
        merr = ex.mock_error(theta[c], mock[c])
        assert np.all(merr <= info['delta']), (c, float(np.max(merr / info['delta'])))
    # the gradient is the polynomial kind's kernel: the same bits on the same inputs
    g = lik.gradient(coefficients=th, precision=tt)
    assert torch.equal(g, _native.poly_gauss_grad(th, dev_t(A, device), dev_t(ys, device), tt))
    if np.array_equal(A, np.vstack([z['xs'] ** i for i in range(K)])):
        poly = Likelihood('points', ForwardModel(z['xs'], POLYVAL), GaussianErrorModel(ys))
        assert torch.equal(g, poly.gradient(coefficients=th, precision=tt))
    else:                                                 # pragma: no cover
        pytest.fail('the fixture\'s jacobi is not vstack([xs**i]) on this numpy')


# ---------------------------------------------------------------------------
# 2. shapes: ragged K and N, N % 16 != 0, C not a multiple of 16
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('K,N,C', SHAPES)
def test_shapes_inside_the_bounds(device, K, N, C):
    A, ys, theta, tau = random_case(K, N, C)
    lik = make_likelihood(A, ys)
    th, tt = dev_t(theta, device), dev_t(tau, device)
    lp_host = lik.log_prob(coefficients=th, precision=2.5).cpu().numpy()
    lp_chain = lik.log_prob(coefficients=th, precision=tt).cpu().numpy()
    mock = lik.forward_model(coefficients=th).cpu().numpy()
    assert lp_host.shape == lp_chain.shape == (C,) and mock.shape == (C, N)
    # every chain against numpy, twice the bound
    delta = LB.mock_bound_float(theta, A)
    assert np.all(np.abs(mock - theta.dot(A)) <= 2 * delta)
    for got, t in ((lp_host, 2.5), (lp_chain, tau)):
        want, bound = LB.logp_float(theta, A, ys, t)
        bad = np.abs(got - want) > 2 * bound
        assert not bad.any(), (np.nonzero(bad)[0][:5], np.max(np.abs(got - want) / bound))
    # some chains against exact arithmetic, the bound itself
    ex = LB.Exact(A, ys)
    chains = exact_chains(C)
    assert len(chains) >= min(C, 4)
    for c in chains:
        info = ex.chain(theta[c])
        merr = ex.mock_error(theta[c], mock[c])
        assert np.all(merr <= info['delta']), (c, float(np.max(merr / info['delta'])))
        for got, t in ((lp_host[c], 2.5), (lp_chain[c], tau[c])):
            want, bound = LB.logp_exact_and_bound(info['chi2'], info['chi2_bound'], t, N)
            err = LB.logp_error(got, want)
            print('K=%d N=%d C=%d chain %d: log-prob error %.3g, bound %.3g, mock error / bound %.3g'
                  % (K, N, C, c, err, bound, float(np.max(merr / info['delta']))))
            assert err <= bound, (c, err, bound)


def test_one_chain_as_a_vector(device):
    """A ``[K]`` state (one chain) goes through the same kernels."""
    A, ys, theta, _ = random_case(7, 37, 1)
    lik = make_likelihood(A, ys)
    v = dev_t(theta[0], device)
    lp1 = lik.log_prob(coefficients=v, precision=2.0)
    lp2 = lik.log_prob(coefficients=v.reshape(1, -1), precision=2.0)
    assert torch.equal(lp1.reshape(-1), lp2.reshape(-1))
    assert lik.forward_model(coefficients=v).shape == (37,)
    assert lik.gradient(coefficients=v, precision=2.0).shape == (7,)


# ---------------------------------------------------------------------------
# 3. the summation order is a function of (K, N) only
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('K,N', [(33, 1024), (17, 2500), (33, 4096), (64, 100)])
def test_order_depends_on_k_and_n_only(device, K, N):
    C = 4097
    A, ys, theta, tau = random_case(K, N, C)
    Ad, yd = dev_t(A, device), dev_t(ys, device)
    th, tt = dev_t(theta, device), dev_t(tau, device)
    full = _native.linear_gauss_logp(th, Ad, yd, tt)
    assert torch.equal(full, _native.linear_gauss_logp(th, Ad, yd, tt))      # two calls, the same bits
    fwd = _native.linear_forward(th, Ad)
    assert torch.equal(fwd, _native.linear_forward(th, Ad))
    for start, n in ((0, 1), (4096, 1), (33, 1), (0, 16), (2000, 16), (7, 17), (4080, 17),
                     (0, 512), (3001, 512), (5, 4090)):
        rows = slice(start, start + n)
        part = _native.linear_gauss_logp(th[rows].contiguous(), Ad, yd, tt[rows].contiguous())
        assert torch.equal(part, full[rows]), (start, n)
        assert torch.equal(_native.linear_forward(th[rows].contiguous(), Ad), fwd[rows]), (start, n)
    # a chain at another place of a batch
    perm = torch.randperm(C, generator=torch.Generator().manual_seed(1)).to(device)
    moved = _native.linear_gauss_logp(th[perm].contiguous(), Ad, yd, tt[perm].contiguous())
    assert torch.equal(moved, full[perm])
    # the host scalar and the per-chain precision are the same arithmetic
    same = _native.linear_gauss_logp(th, Ad, yd, torch.full((C,), 2.5, dtype=torch.float64, device=device))
    assert torch.equal(same, _native.linear_gauss_logp(th, Ad, yd, 2.5))


# ---------------------------------------------------------------------------
# 4. non-finite coefficients behave as in numpy and stay in their chain
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('K,N,C,k_inf,k_nan', [(7, 37, 40, 6, 2), (33, 2501, 40, 32, 3), (5, 19, 4100, 0, 4)])
def test_non_finite_coefficients(device, K, N, C, k_inf, k_nan):
    assert N % 16 != 0 and K % 4 != 0
    A, ys, theta, tau = random_case(K, N, C)
    c_inf, c_nan, c_minf = 5, 21, C - 2
    dirty = theta.copy()
    dirty[c_inf, k_inf] = np.inf
    dirty[c_nan, k_nan] = np.nan
    dirty[c_minf, k_inf] = -np.inf
    Ad, yd, tt = dev_t(A, device), dev_t(ys, device), dev_t(tau, device)
    clean_lp = _native.linear_gauss_logp(dev_t(theta, device), Ad, yd, tt).cpu().numpy()
    dirty_lp = _native.linear_gauss_logp(dev_t(dirty, device), Ad, yd, tt).cpu().numpy()
    clean_fw = _native.linear_forward(dev_t(theta, device), Ad).cpu().numpy()
    dirty_fw = _native.linear_forward(dev_t(dirty, device), Ad).cpu().numpy()
    with np.errstate(all='ignore'):
        mock = dirty @ A
        want = -0.5 * np.sum((mock - ys) ** 2, axis=1) * tau + N * 0.5 * np.log(tau)
    touched = [c_inf, c_nan, c_minf]
    assert np.isnan(want[c_nan]) and np.isneginf(want[c_inf]) and np.isneginf(want[c_minf])
    for c in touched:
        assert np.isnan(dirty_lp[c]) == np.isnan(want[c]) and np.isinf(dirty_lp[c]) == np.isinf(want[c]), c
        assert not np.isfinite(dirty_lp[c]) and (np.isnan(want[c]) or dirty_lp[c] == want[c])
        assert np.array_equal(np.isnan(dirty_fw[c]), np.isnan(mock[c])), c
        inf = np.isinf(mock[c])
        assert np.array_equal(np.isinf(dirty_fw[c]), inf) and np.array_equal(dirty_fw[c][inf], mock[c][inf]), c
    others = np.setdiff1d(np.arange(C), touched)
    assert np.array_equal(dirty_lp[others], clean_lp[others])
    assert np.array_equal(dirty_fw[others], clean_fw[others])
    assert np.all(np.isfinite(clean_lp)) and np.all(np.isfinite(clean_fw))


# ---------------------------------------------------------------------------
# 5. guard zones
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('K,N,C', SHAPES)
def test_kernels_stay_inside_their_buffers(device, K, N, C):
    A, ys, theta, tau = random_case(K, N, C)
    L = _native.lib()
    need = L.binf_linear_gauss_logp_workspace_bytes(C, K, N)
    assert (need > 0) == (N > 1024)
    st = _native.stream_handle(device)
    outs = []
    for make in (Guarded(device), None):
        t = make if make is not None else (lambda a: plain(a, device))
        th, Ad, yd, tt = t(theta), t(A), t(ys), t(tau)
        lp_h, lp_c, fw = t(np.zeros(C)), t(np.zeros(C)), t(np.zeros((C, N)))
        ws = t(np.zeros(max(1, need // 8)))
        wsp = ws.data_ptr() if need > 0 else None
        assert L.binf_linear_gauss_logp_f64(th.data_ptr(), Ad.data_ptr(), yd.data_ptr(), 2.5, None,
                                            lp_h.data_ptr(), wsp, need, C, K, N, st) == 0
        assert L.binf_linear_gauss_logp_f64(th.data_ptr(), Ad.data_ptr(), yd.data_ptr(), 0.0, tt.data_ptr(),
                                            lp_c.data_ptr(), wsp, need, C, K, N, st) == 0
        assert L.binf_linear_forward_f64(th.data_ptr(), Ad.data_ptr(), fw.data_ptr(), C, K, N, st) == 0
        if make is not None:
            make.check()
        outs.append([x.clone().cpu() for x in (lp_h, lp_c, fw, th, Ad, yd, tt)])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
        assert not torch.isnan(a).any()


# ---------------------------------------------------------------------------
# 6. leapfrog
# ---------------------------------------------------------------------------
def posterior_of(lik, K, var=5.0):
    return Posterior({lik.name: lik},
                     {'precision_prior': GammaPrior(1.0, 0.2),
                      'coefficients_prior': GaussianPrior(np.zeros(K), np.full(K, var))})


def poly_bound(A, ys, K, var=5.0):
    """tests/poly_bounds.PolyBound for a general design matrix: it needs J, aJ, JJt, y."""
    pb = object.__new__(PB.PolyBound)
    pb.J = np.asarray(A, dtype=np.float64)
    pb.aJ = np.abs(pb.J)
    pb.y = np.asarray(ys, dtype=np.float64)
    pb.K, pb.N = K, len(ys)
    pb.mu, pb.var = np.zeros(K), np.full(K, var)
    pb.JJt = pb.J.dot(pb.J.T)
    return pb


class Spy(object):
    def __init__(self, monkeypatch, name):
        self.calls = 0
        self.fn = getattr(_native, name)
        monkeypatch.setattr(_native, name, self)

    def __call__(self, *a, **kw):
        self.calls += 1
        return self.fn(*a, **kw)


@pytest.mark.parametrize('K,N,C,dt,L,per_chain', [(7, 37, 50, 0.02, 10, False), (33, 1000, 130, 0.004, 10, True),
                                                  (4, 20, 4100, 0.02, 5, True)])
def test_leapfrog_takes_the_kinds_hook(device, monkeypatch, K, N, C, dt, L, per_chain):
    A, ys, theta, tau = random_case(K, N, C)
    rs = np.random.RandomState(9)
    p0 = rs.standard_normal((C, K))
    tau_v = dev_t(tau, device) if per_chain else 2.5
    cond = posterior_of(make_likelihood(A, ys), K).conditional_factory(precision=tau_v)
    spec = cond.native_leapfrog_spec('coefficients')
    assert spec is not None and spec[0] == 'linear'
    s = HMCSampler(cond, dev_t(theta, device), dt, L, variable_name='coefficients')
    spy = Spy(monkeypatch, 'poly_leapfrog')
    q, p = dev_t(theta, device), dev_t(p0, device)
    s._leapfrog(q, p, dt, L)
    assert spy.calls == 1
    # the per-step sequence on the same batch: the same bits
    Ad, yd = dev_t(A, device), dev_t(ys, device)
    q2, p2 = dev_t(theta, device), dev_t(p0, device)
    grad = lambda x: _native.poly_gauss_grad(x, Ad, yd, tau_v)
    _native.leapfrog_kick(p2, grad(q2), dt, None, half=True)
    _native.leapfrog_drift(q2, p2, dt, None)
    for _ in range(L - 1):
        _native.leapfrog_kick_drift(q2, p2, grad(q2), dt, None)
    _native.leapfrog_kick(p2, grad(q2), dt, None, half=True)
    assert torch.equal(q, q2) and torch.equal(p, p2)
    # ... and through the sampler's own per-step loop
    s.fused_leapfrog = False
    q3, p3 = dev_t(theta, device), dev_t(p0, device)
    s._leapfrog(q3, p3, dt, L)
    assert spy.calls == 1 and torch.equal(q, q3) and torch.equal(p, p3)
    # inside the propagated bound of the numpy trajectory
    pb = poly_bound(A, ys, K)
    qn, pn = q.cpu().numpy(), p.cpu().numpy()
    for c in exact_chains(C) + [C // 3]:
        b = pb.transition(theta[c], p0[c], tau[c] if per_chain else 2.5, dt, L)
        assert np.all(np.abs(qn[c] - b['q']) <= b['bq'] + 4 * PB.U * np.abs(b['q'])), c
        assert np.all(np.abs(pn[c] - b['p']) <= b['bp'] + 4 * PB.U * np.abs(b['p'])), c


# ---------------------------------------------------------------------------
# 7. a model from outside the package
# ---------------------------------------------------------------------------
class Fourier(LinearForwardModel):
    """What a user writes: the design matrix, built in ``__init__``.  No kernel, no registry
    call."""

    def __init__(self, xs, n_modes):
        self.xs, self.n_modes = np.asarray(xs, dtype=np.float64), n_modes
        rows = [np.ones_like(self.xs)]
        for m in range(1, n_modes + 1):
            rows += [np.cos(m * self.xs), np.sin(m * self.xs)]
        super(Fourier, self).__init__('fourier', np.vstack(rows))


class PlainFourier(Fourier):
    """The same model evaluated as the user wrote it: the plug-in path."""

    def _evaluate(self, coefficients):
        return torch.matmul(coefficients, self.design_matrix(coefficients.shape[-1], coefficients.device))


def fourier_case(N=40, n_modes=3, tau=2.5, seed=5):
    rs = np.random.RandomState(seed)
    xs = np.linspace(0.0, 2 * np.pi, N, endpoint=False) + 0.05 * rs.standard_normal(N)
    truth = np.array([1.0, 2.0, -1.0, 0.5, 0.0, -0.7, 0.3])[:2 * n_modes + 1]
    A = Fourier(xs, n_modes).design
    ys = truth.dot(A) + rs.standard_normal(N) / np.sqrt(tau)
    return xs, ys, A


def test_user_model_runs_on_the_fused_hooks_and_agrees_with_the_plug_in_path(device, monkeypatch):
    n_modes, tau, dt, L, C = 3, 2.5, 0.03, 12, 37
    K = 2 * n_modes + 1
    xs, ys, A = fourier_case(n_modes=n_modes, tau=tau)
    rs = np.random.RandomState(6)
    theta = rs.standard_normal((C, K))
    p0, u = rs.standard_normal((C, K)), rs.uniform(size=C)
    spies = {n: Spy(monkeypatch, n) for n in ('linear_gauss_logp', 'poly_leapfrog', 'gauss_err_logp',
                                              'jacobian_contract', 'linear_forward')}
    count = lambda: {n: s.calls for n, s in spies.items()}
    pb = poly_bound(A, ys, K)
    results = {}
    for label, cls in (('fused', Fourier), ('plug-in', PlainFourier)):
        lik = Likelihood('points', cls(xs, n_modes), GaussianErrorModel(ys))
        assert (lik._native_pair() is not None) == (label == 'fused')
        cond = posterior_of(lik, K).conditional_factory(precision=tau)
        s = HMCSampler(cond, dev_t(theta, device), dt, L, variable_name='coefficients', record_energies=True)
        before = count()
        q, p = dev_t(theta, device), dev_t(p0, device)
        s._leapfrog(q, p, dt, L)
        out = s.sample(p0=dev_t(p0, device), u=dev_t(u, device))
        d = {n: v - before[n] for n, v in count().items()}
        if label == 'fused':
            assert d['poly_leapfrog'] == 2 and d['linear_gauss_logp'] == 2
            assert d['gauss_err_logp'] == d['jacobian_contract'] == d['linear_forward'] == 0
        else:
            assert d['poly_leapfrog'] == d['linear_gauss_logp'] == d['linear_forward'] == 0
            assert d['jacobian_contract'] == 2 * (L + 1) and d['gauss_err_logp'] == 2
        gp = cond.priors['precision_prior']
        results[label] = (q.cpu().numpy(), p.cpu().numpy(), s.last_e_before.cpu().numpy(),
                          s.last_e_after.cpu().numpy(), out.cpu().numpy(), (gp.shape, gp.rate))

    def np_energy(q, p, gamma):
        shape, rate = gamma
        lp = -0.5 * np.sum((q.dot(A) - ys) ** 2) * tau + len(ys) * 0.5 * np.log(tau)
        lp = lp + -0.5 * np.sum((q - 0.0) ** 2 / 5.0) + ((shape - 1.0) * np.log(tau) - tau * rate)
        return -lp + 0.5 * np.sum(p ** 2)
    for c in range(C):
        b = pb.transition(theta[c], p0[c], tau, dt, L)
        for label in ('fused', 'plug-in'):
            q, p, eb, ea, _, gamma = results[label]
            assert np.all(np.abs(q[c] - b['q']) <= b['bq'] + 4 * PB.U * np.abs(b['q'])), (label, c)
            assert np.all(np.abs(p[c] - b['p']) <= b['bp'] + 4 * PB.U * np.abs(b['p'])), (label, c)
            assert abs(eb[c] - np_energy(theta[c], p0[c], gamma)) <= b['be_before'], (label, c)
            assert abs(ea[c] - np_energy(b['q'], b['p'], gamma)) <= b['be_after'], (label, c)
        assert np.all(np.abs(results['fused'][0][c] - results['plug-in'][0][c]) <=
                      2 * (b['bq'] + 4 * PB.U * np.abs(b['q'])))
    # the accepted / rejected states agree wherever the acceptance test is not a coin toss
    # at rounding level (it is not, for these draws)
    assert np.all(np.abs(results['fused'][4] - results['plug-in'][4]) <= 1e-9)


def test_user_model_samples_its_analytic_gaussian(device, monkeypatch):
    """At fixed tau the coefficient conditional is Gaussian with precision matrix
    tau A A^T + diag(1 / prior variance): the rule and the numbers of
    test_gpu_statistics.py::test_polynomial_conditional_matches_its_analytic_gaussian."""
    n_modes, tau, C = 3, 2.5, 4096
    K = 2 * n_modes + 1
    xs, ys, A = fourier_case(n_modes=n_modes, tau=tau)
    P = tau * A @ A.T + np.eye(K) / 5.0
    cov = np.linalg.inv(P)
    mean = cov @ (tau * A @ ys)
    rs = np.random.RandomState(5)
    lik = Likelihood('points', Fourier(xs, n_modes), GaussianErrorModel(ys))
    cond = posterior_of(lik, K).conditional_factory(precision=tau)
    start = torch.from_numpy(mean + rs.standard_normal((C, K)) @ np.linalg.cholesky(cov).T).to(device)
    s = HMCSampler(cond, start, 0.03, 40, variable_name='coefficients', rng=DeviceRNG(3, device))
    logp, leap = Spy(monkeypatch, 'linear_gauss_logp'), Spy(monkeypatch, 'poly_leapfrog')
    sweeps, burn = 120, 40
    kept = []
    for i in range(sweeps):
        x = s.sample()
        if i >= burn and i % 5 == 0:
            kept.append(x.clone())
    assert leap.calls == sweeps and logp.calls == 2 * sweeps
    acc = float(s.acceptance_rate.mean())
    assert 0.6 < acc <= 1.0
    x = torch.stack(kept).cpu().numpy()
    se = np.sqrt(np.diag(cov) / C)
    assert (np.abs(x.mean((0, 1)) - mean) < 6 * se).all()
    emp = np.cov(x.reshape(-1, K).T)
    assert np.abs(emp - cov).max() < 0.15 * np.abs(cov).max()


def test_gibbs_with_gamma_sampler_runs_through_the_fused_hook(device, monkeypatch):
    n_modes, C, sweeps, L = 3, 300, 50, 20
    K = 2 * n_modes + 1
    xs, ys, A = fourier_case(n_modes=n_modes)
    lik = Likelihood('points', Fourier(xs, n_modes), GaussianErrorModel(ys))
    post = posterior_of(lik, K)
    start = BinfState(dict(coefficients=torch.ones((C, K), dtype=torch.float64, device=device),
                           precision=torch.ones(C, dtype=torch.float64, device=device)))
    gips = make_hmc_sampler(post, 0.03, L, start, rng=DeviceRNG(1, device))
    logp, leap = Spy(monkeypatch, 'linear_gauss_logp'), Spy(monkeypatch, 'poly_leapfrog')
    plug = Spy(monkeypatch, 'gauss_err_logp')
    for _ in range(sweeps):
        state = gips.sample()
    # per sweep: E_before, E_after and the precision sampler's unit-precision log-prob
    assert logp.calls == 3 * sweeps and leap.calls == sweeps and plug.calls == 0
    th, pr = state.variables['coefficients'], state.variables['precision']
    assert th.shape == (C, K) and pr.shape == (C,)
    assert bool(torch.isfinite(th).all()) and bool((pr > 0).all())
    assert float(gips.subsamplers['coefficients'].acceptance_rate.mean()) > 0.5
    # the chains have found the data: residual scale ~ the noise's
    resid = (th.cpu().numpy() @ A - ys).std()
    assert resid < 1.0


# ---------------------------------------------------------------------------
# 8. HIP graph
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('K,N,C', [(7, 37, 5), (33, 4096, 300)])
def test_log_prob_captured_in_a_graph_replays_the_eager_bits(device, K, N, C):
    A, ys, theta, tau = random_case(K, N, C)
    Ad, yd, tt = dev_t(A, device), dev_t(ys, device), dev_t(tau, device)
    static = dev_t(theta, device)
    eager0 = _native.linear_gauss_logp(static, Ad, yd, tt).clone()        # also warms up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = _native.linear_gauss_logp(static, Ad, yd, tt)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager0)
    other = dev_t(theta[::-1] * 1.5, device)
    static.copy_(other)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, _native.linear_gauss_logp(other, Ad, yd, tt))


def test_graphed_sampler_on_the_linear_posterior(device):
    n_modes, tau, dt, L, C = 3, 2.5, 0.03, 6, 64
    K = 2 * n_modes + 1
    xs, ys, A = fourier_case(n_modes=n_modes, tau=tau)
    rs = np.random.RandomState(8)
    theta = rs.standard_normal((C, K))
    samplers = []
    for graph in (True, False):
        lik = Likelihood('points', Fourier(xs, n_modes), GaussianErrorModel(ys))
        cond = posterior_of(lik, K).conditional_factory(precision=tau)
        samplers.append(HMCSampler(cond, dev_t(theta, device), dt, L, variable_name='coefficients',
                                   graph=graph, record_energies=True))
    for i in range(4):
        p0, u = rs.standard_normal((C, K)), rs.uniform(size=C)
        a = samplers[0].sample(p0=dev_t(p0, device), u=dev_t(u, device))
        b = samplers[1].sample(p0=dev_t(p0, device), u=dev_t(u, device))
        assert torch.equal(a, b), i
        assert torch.equal(samplers[0].last_e_after, samplers[1].last_e_after)
    assert samplers[0]._graphs, 'the transition was not captured'


# ---------------------------------------------------------------------------
# the example script
# ---------------------------------------------------------------------------
def test_example_linear_basis_recovers_the_signal(device):
    import importlib.util
    path = os.path.join(os.path.dirname(GOLDEN_DIR), os.pardir, 'examples', 'linear_basis.py')
    spec = importlib.util.spec_from_file_location('linear_basis', os.path.normpath(path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    coeffs, prec = mod.main(['--chains', '256', '--iterations', '300', '--burn-in', '100', '--thin', '20',
                             '--modes', '3', '--data', '150'])
    assert coeffs.shape == (10, 256, 7) and prec.shape[:2] == (10, 256)
    # the data of the script (seed 0): the posterior mean is within a few posterior standard
    # deviations of the coefficients that made them, the precision near the true one
    rs = np.random.RandomState(0)
    truth = rs.standard_normal(7) / (1.0 + np.arange(7) // 2)
    c = coeffs.reshape(-1, 7).cpu().numpy()
    assert np.all(np.abs(c.mean(0) - truth) < 5 * c.std(0) + 0.05)
    assert 2.0 < float(prec.mean()) < 8.0
