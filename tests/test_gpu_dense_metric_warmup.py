"""``WindowedWarmup(..., dense=True)`` on the device: the driver against the restated warm-up
(``tests/dense_metric_ref.py``) bit for bit -- the factor after every window, the flags, the
states and step sizes --, a checkpoint in the middle of a window, a replica ladder, and the
rotated-Gaussian experiment of ``tests/test_dense_metric.py`` at one seed with its bars."""
import numpy as np
import pytest
import torch

import dense_metric_ref as DM
import metric_ref as MR
from binf_amd import checkpoint
from binf_amd.pdf import IsotropicGaussian
from binf_amd.samplers.hmc import HMCSampler
from binf_amd.samplers.replica import ReplicaExchangeSampler
from binf_amd.samplers.rng import DeviceRNG
from binf_amd.samplers.warmup import WindowedWarmup, warmup

pytestmark = pytest.mark.gpu


def bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_driver(device, G, graph, C, D):
    """60 warm-up transitions, windows [10, 20) and [20, 50), then five kept draws; the draws
    are handed to both sides."""
    n, keep = 60, 5
    rs = np.random.RandomState(31 + G)
    width = 10.0 ** (np.arange(D) / (D - 1.0) - 0.5)
    q0 = 0.25 + rs.standard_normal((C, D)) * width
    p0, u = rs.standard_normal((n + keep, C, D)), rs.uniform(size=(n + keep, C))
    ref = DM.DenseHMC(MR.GaussTarget(2.5, 0.25), q0, 0.2, 3, np.eye(D)[None].repeat(G, 0), uprate=1.02, downrate=0.9)
    rw = DM.DenseWarmup(ref, n, 10, 10, 10)
    s = HMCSampler(IsotropicGaussian(k=2.5, x0=0.25), torch.from_numpy(q0).to(device), 0.2, 3, variable_name='x',
                   adaption_uprate=1.02, adaption_downrate=0.9, graph=graph)
    t = [0]

    def advance():
        x = s.sample(p0=torch.from_numpy(p0[t[0]]).to(device), u=torch.from_numpy(u[t[0]]).to(device))
        t[0] += 1
        return x
    w = WindowedWarmup(s, n, init_buffer=10, term_buffer=10, base_window=10, groups=G, advance=advance, dense=True)
    assert w.windows == rw.windows == [(10, 20), (20, 50)] and w.dense and w.groups == G
    assert tuple(s.metric_chol.shape) == (G, D, D) and bits(s.metric_chol.cpu().numpy(), ref.chol)
    address, seen = s.metric_chol.data_ptr(), 0
    for i in range(n):
        x = w.step()
        want = rw.step(p0[i], u[i])
        assert bits(x.cpu().numpy(), want), i
        assert w.n_window == (rw.mom.n if any(a <= i < b - 1 for a, b in rw.windows) else 0)
        if len(rw.factors) > seen:                                       # a window ended
            seen += 1
            assert bits(s.metric_chol.cpu().numpy(), rw.factors[-1]), i
            assert bits(w.status.cpu().numpy(), rw.status) and not rw.status.any()
    assert seen == 2 and w.done and s.metric_chol.data_ptr() == address
    assert not bits(rw.factors[0], rw.factors[1]) and isinstance(w.status, torch.Tensor) and w.status.is_cuda
    assert bits(s.timestep.cpu().numpy(), ref.dt_chain) and np.array_equal(s.n_accepted.cpu().numpy(), ref.n_accepted)
    for i in range(n, n + keep):
        assert bits(advance().cpu().numpy(), ref.sample(p0[i], u[i])), i
    up = np.triu(np.ones((D, D), dtype=bool), 1)
    assert np.all(s.metric_chol.cpu().numpy()[:, up] == 0.0)


@pytest.mark.parametrize('graph', [False, 'always'])
@pytest.mark.parametrize('G', [1, 2])
def test_driver_equals_the_restated_warmup(device, G, graph):
    """16 chains x 8 dimensions."""
    check_driver(device, G, graph, 16, 8)


@pytest.mark.parametrize('C,D', [(1040, 8), (12, 140)])
@pytest.mark.parametrize('graph', [False, 'always'])
@pytest.mark.parametrize('G', [1, 2])
def test_driver_equals_the_restated_warmup_at_width_and_batch(device, G, graph, C, D):
    """1040 chains: 1040 or 520 to a group, so the co-moment kernel sums a second round of blocks
    onto wave 0's total.  140 dimensions: i-tiles of 256 in the leapfrog, and the first window's
    10 transitions give 120 or 60 draws to a group, fewer than dimensions: the factor exists by
    the shrinkage alone."""
    check_driver(device, G, graph, C, D)


class Harmonic(object):
    """A user's torch PDF: log p_c(x) = -1/2 beta_c x^T P x."""

    def __init__(self, beta, precision):
        self.beta, self.P = beta, precision

    def log_prob(self, x):
        return -0.5 * self.beta * (x * (x @ self.P)).sum(dim=1)

    def gradient(self, x):
        return self.beta[:, None] * (x @ self.P)


def rotated(device):
    S, P, Ls = DM.rotated_target()
    return torch.from_numpy(P).to(device), torch.from_numpy(Ls).to(device), Ls


def _warm_run(device, graph=False):
    C = 8
    P, Lt, _ = rotated(device)
    D = P.shape[0]
    rng = DeviceRNG(77, device)
    x0 = 2.0 * torch.from_numpy(np.random.RandomState(8).standard_normal((C, D))).to(device) @ Lt.T
    s = HMCSampler(Harmonic(torch.ones(C, dtype=torch.float64, device=device), P), x0, 0.3, 4,
                   adaption_uprate=1.02, adaption_downrate=0.9, variable_name='x', rng=rng, graph=graph)
    return s, WindowedWarmup(s, 70, init_buffer=10, term_buffer=10, base_window=10, dense=True)


@pytest.mark.parametrize('graph', [False, 'always'])
def test_checkpoint_in_the_middle_of_a_window(device, graph):
    """40 of 70 warm-up transitions (windows [10, 20), [20, 60): the second is open), the
    state of sampler and driver through the host into fresh objects, the rest and five kept
    draws equal the uninterrupted run bit for bit."""
    a, wa = _warm_run(device, graph)
    assert wa.windows == [(10, 20), (20, 60)] and a.timestep_adaption_limit == 71
    for _ in range(40):
        wa.step()
    ck = checkpoint.state_dict(sampler=a, warmup=wa)
    assert 'metric_chol' in ck['sampler'] and not ck['sampler']['metric_chol'].is_cuda
    assert ck['warmup']['dense'] and tuple(ck['warmup']['s2'].shape) == (1, 8, 8) and ck['warmup']['n_window'] == 20
    b, wb = _warm_run(device, graph)
    checkpoint.load_state_dict(ck, sampler=b, warmup=wb)
    assert wb.t == 40 and wb.n_window == 20 and torch.equal(a.metric_chol, b.metric_chol)
    wa.run(), wb.run()
    assert wa.done and wb.done and a.counter == b.counter == 70
    assert torch.equal(a.metric_chol, b.metric_chol) and torch.equal(a.timestep, b.timestep)
    assert torch.equal(wa.status, wb.status) and not bool(wa.status.any())
    for _ in range(5):
        assert torch.equal(a.sample(), b.sample())
    assert not torch.equal(a.metric_chol, torch.eye(8, dtype=torch.float64, device=device)[None])
    with pytest.raises(RuntimeError):
        wa.step()
    # a diagonal driver does not take a dense checkpoint
    c = HMCSampler(IsotropicGaussian(), torch.zeros(8, 8, dtype=torch.float64, device=device), 0.3, 4, variable_name='x')
    with pytest.raises(ValueError):
        WindowedWarmup(c, 70, init_buffer=10, term_buffer=10, base_window=10).load_state_dict(ck['warmup'])


def test_a_ladder_gets_one_factor_per_slot(device):
    """4 ladders x 3 slots at beta = 1, 1/4, 1/16: the inner sampler gets three factors, they
    differ, and a hotter slot's M^-1 is the wider one (covariance ~ Sigma / beta)."""
    R, n_ladders = 3, 4
    C = R * n_ladders
    sigma = np.array([1.0, 2.0, 5.0, 0.5, 10.0])
    D = len(sigma)
    Q, _ = np.linalg.qr(np.random.RandomState(2).standard_normal((D, D)))
    P = torch.from_numpy((Q / sigma ** 2) @ Q.T).to(device)
    Lt = torch.from_numpy(np.linalg.cholesky((Q * sigma ** 2) @ Q.T)).to(device)
    beta = torch.tensor([1.0, 0.25, 0.0625], dtype=torch.float64, device=device).repeat(n_ladders)
    rng = DeviceRNG(5, device)
    x0 = (rng.normal((C, D), device) @ Lt.T) / beta.sqrt()[:, None]
    inner = HMCSampler(Harmonic(beta, P), x0, 0.3, 5, variable_name='x', rng=rng)
    rex = ReplicaExchangeSampler(inner, R)
    w = warmup(rex, 120, init_buffer=10, term_buffer=10, base_window=20, dense=True)
    assert w.groups == R and w.hmc is inner and tuple(inner.metric_chol.shape) == (R, D, D)
    assert rex.round == 120 and inner.counter == 120 and w.status.cpu().tolist() == [0, 0, 0]
    L = inner.metric_chol.cpu().numpy()
    assert np.isfinite(L).all() and (L[:, np.eye(D, dtype=bool)] > 0).all()
    logdet = 2.0 * np.log(L[:, np.eye(D, dtype=bool)]).sum(axis=1)
    for r in range(R - 1):
        assert not np.array_equal(L[r], L[r + 1])
        assert (logdet[r + 1] - logdet[r]) / D > 0.4                    # expected log 4 = 1.39 per dimension
    rex.sample()                                                        # goes on with the metric in place


def _device_experiment(device, dense, seed=0, C=16, n_warmup=300, n_keep=200):
    P, Lt, Ls = rotated(device)
    D = P.shape[0]
    rng = DeviceRNG(1234 + seed, device)
    x0 = 3.0 * rng.normal((C, D), device) @ Lt.T
    s = HMCSampler(Harmonic(torch.ones(C, dtype=torch.float64, device=device), P), x0, 0.5, 5, variable_name='x',
                   adaption_uprate=1.02, adaption_downrate=0.9, rng=rng)
    warmup(s, n_warmup, init_buffer=20, term_buffer=40, base_window=20, dense=dense)
    kept = torch.stack([s.sample() for _ in range(n_keep)]).cpu().numpy()
    chol = s.metric_chol[0].cpu().numpy() if dense else np.diag(s.metric_scale[0].cpu().numpy())
    return MR.max_split_rhat(kept), DM.whitened_eigenvalues(chol, Ls)


def test_the_rotated_gaussian_on_the_device(device):
    """The CPU test's experiment and bars at one seed, the device drawing for itself: dense max
    split-R^ <= 1.1 and whitened eigenvalues in [0.5, 2]; the diagonal metric >= 2."""
    rd, ed = _device_experiment(device, True)
    rg, eg = _device_experiment(device, False)
    print('dense: max split-R^ %.3f, eigenvalues %.3g ... %.3g; diagonal: %.3f, %.3g ... %.3g'
          % (rd, ed.min(), ed.max(), rg, eg.min(), eg.max()))
    assert rd <= 1.1 and ed.min() >= 0.5 and ed.max() <= 2.0
    assert rg >= 2.0
