"""The one integrator route of the samplers (``HMCSampler._integrator``): for the identity, a
diagonal and a dense metric, ``HMCSampler._leapfrog`` and a ``NUTSSampler`` transition launch the
plain, ``_scaled`` or ``_dense`` entry points -- those and no others, the stated number of times
-- and equal the numpy restatements bit for bit.

The PDF's gradient is plain torch (one subtraction, one multiplication per element: numpy's
bits), so no kind's fused leapfrog applies and every kick and drift is a launch of its own.
C = 6 chains in G = 3 groups; D = 5 takes the scalar variant of the element-wise kernel, D = 6
the 16-byte one."""
import numpy as np
import pytest
import torch

import dense_metric_ref as DM
import metric_ref as MR
import nuts_ref as N
from binf_amd import _native
from binf_amd.samplers import NUTSSampler
from binf_amd.samplers.hmc import HMCSampler

pytestmark = pytest.mark.gpu

f64 = np.float64
K_, X0 = 0.7, 0.3
C, G, NSTEPS = 6, 3, 3
PIECES = ('leapfrog_kick', 'leapfrog_drift', 'leapfrog_kick_drift')
SUFFIX = {'identity': '', 'diag': '_scaled', 'dense': '_dense'}


class TorchGauss(object):
    """log p(x) = -1/2 k sum (x - x0)^2 in torch operations whose roundings are numpy's: the
    row sum is added up from the left, as numpy sums fewer than eight elements."""

    def log_prob(self, x):
        sq = (x - X0) * (x - X0)
        acc = sq[:, 0]
        for j in range(1, sq.shape[1]):
            acc = acc + sq[:, j]
        return (-0.5 * K_) * acc

    def gradient(self, x):
        return K_ * (x - X0)


def host_logp(q):
    with np.errstate(all='ignore'):
        return (f64(-0.5) * f64(K_)) * np.sum((q - f64(X0)) ** 2, axis=1)


def host_grad(q):
    return f64(K_) * (q - f64(X0))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def metric_of(kind, D, seed):
    rs = np.random.RandomState(seed)
    if kind == 'diag':
        return 2.0 ** rs.uniform(-1.0, 1.0, size=(G, D))
    if kind == 'dense':
        L = np.tril(0.2 * rs.standard_normal((G, D, D)))
        i = np.arange(D)
        L[:, i, i] = 2.0 ** rs.uniform(-1.0, 1.0, size=(G, D))
        return L
    return None


class Spy(object):
    def __init__(self, monkeypatch, name):
        self.calls, self.fn = 0, getattr(_native, name)
        monkeypatch.setattr(_native, name, self)

    def __call__(self, *a, **kw):
        self.calls += 1
        return self.fn(*a, **kw)


def spies(monkeypatch, extra=()):
    names = [p + s for s in SUFFIX.values() for p in PIECES] + list(extra)
    return {n: Spy(monkeypatch, n) for n in names}


def counts(sp, kind, kick, drift, kick_drift):
    """The launches under ``kind``'s suffix, and none under the other two."""
    want = {p + s: (n if s == SUFFIX[kind] else 0)
            for s in SUFFIX.values() for p, n in zip(PIECES, (kick, drift, kick_drift))}
    return {n: sp[n].calls for n in want} == want


def sampler_kw(kind, param, up):
    return {'metric': up(param)} if kind == 'diag' else {'dense_metric': up(param)} if kind == 'dense' else {}


@pytest.mark.parametrize('mode', ['exact', 'fma'])
@pytest.mark.parametrize('D', [5, 6])
@pytest.mark.parametrize('kind', sorted(SUFFIX))
def test_leapfrog_takes_the_metrics_launches_and_equals_the_restatement(device, monkeypatch, kind, D, mode):
    rs = np.random.RandomState(100 + D)
    q0, p0 = rs.standard_normal((2, C, D))
    dtc = rs.uniform(0.05, 0.3, size=C)
    param = metric_of(kind, D, 7)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)
    s = HMCSampler(TorchGauss(), up(q0), 0.1, NSTEPS, variable_name='x', mode=mode, **sampler_kw(kind, param, up))
    fma = mode == 'fma'
    for dt, dc in ((0.173, None), (0.0, dtc)):
        if kind == 'dense':
            wq, wp = DM.leapfrog(q0, p0, host_grad, param, dt, dc, NSTEPS, fma)
        else:
            scale = param if kind == 'diag' else np.ones((1, D))
            wq, wp = MR.leapfrog(q0, p0, host_grad, scale, dt, dc, NSTEPS, fma)
        with monkeypatch.context() as m:
            sp = spies(m)
            q, p = up(q0), up(p0)
            s._leapfrog(q, p, dt if dc is None else up(dc), NSTEPS)
        assert counts(sp, kind, 2, 1, NSTEPS - 1), {n: x.calls for n, x in sp.items()}
        assert same_bits(q.cpu().numpy(), wq) and same_bits(p.cpu().numpy(), wp), (dt, dc is not None)


@pytest.mark.parametrize('mode', ['exact', 'fma'])
@pytest.mark.parametrize('D', [5, 6])
@pytest.mark.parametrize('kind', sorted(SUFFIX))
def test_a_nuts_transition_takes_the_metrics_launches_and_equals_the_restatement(device, monkeypatch, kind, D, mode):
    md, eps = 2, 0.3
    rs = np.random.RandomState(200 + D)
    q0 = X0 + rs.standard_normal((C, D)) / np.sqrt(K_)
    p0, u = rs.standard_normal((C, D)), rs.uniform(size=(C, N.n_uniforms(md)))
    param = metric_of(kind, D, 8)
    ref = N.NUTS(host_logp, host_grad, q0, eps, md, N.Integrator(kind, param, fma=mode == 'fma'))
    want = ref.sample(p0, u)
    assert ref.tree.min_margin > 1e-9               # no selection hangs on an ulp of an exponential
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)
    s = NUTSSampler(TorchGauss(), up(q0), eps, max_tree_depth=md, variable_name='x', mode=mode,
                    **sampler_kw(kind, param, up))
    sp = spies(monkeypatch, extra=('nuts_leaf',))
    got = s.sample(p0=up(p0), u=up(u))
    leaves = sp['nuts_leaf'].calls
    assert leaves in (1, 3)                         # the host stops at a leaf total of 2^k - 1
    assert counts(sp, kind, 2 * leaves, leaves, 0), {n: x.calls for n, x in sp.items()}
    assert same_bits(got.cpu().numpy(), want)
    assert np.array_equal(s.last_n_leapfrog.cpu().numpy(), ref.tree.n_leap)
    assert np.array_equal(s.last_status.cpu().numpy(), ref.tree.status)
