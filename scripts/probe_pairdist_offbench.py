"""Pair-distance kernels no other benchmark prices (development aid): a sample() through
pairdist_leapfrog_sym_kernel<*, false, *, *> (a bead count that is no multiple of 64), one through
pairdist_tiles_update_kernel (a wave per tile, 1000 and 2048 beads) and the unpacked gradient
beyond 1024 beads (pairdist_grad_kernel<256>); medians of five repeats, ms.  For an A/B of two
libraries run it under BINF_LIB_OVERRIDE (profiles/r11_a_pairdist_ab.jsonl)."""
import json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from binf_amd import _native
from binf_amd.example.distance import make_distance_likelihood
from binf_amd.pdf import IsotropicGaussian
from binf_amd.pdf.posteriors import Posterior
from binf_amd.samplers.hmc import HMCSampler
from binf_amd.samplers.rng import DeviceRNG
dev = torch.device('cuda:0')
out = {}


def med(fn, k, reps=5):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        for _ in range(k): fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) / k * 1e3)
    return round(sorted(ts)[reps // 2], 4)


for n, C in ((200, 256), (200, 2048), (100, 2048), (1000, 8), (2048, 16)):
    rs = np.random.RandomState(0)
    truth = rs.standard_normal((n, 3)) * 2.0
    d = np.sqrt(((truth[:, None, :] - truth[None, :, :]) ** 2).sum(-1))
    iu = np.triu_indices(n, 1)
    ys = np.abs(d[iu] + 0.05 * rs.standard_normal(len(iu[0])))
    lik = make_distance_likelihood(ys, n)
    prior = IsotropicGaussian(0.05, 0.0, name='coordinates_prior', variable_name='coordinates')
    cond = Posterior({lik.name: lik}, {prior.name: prior}).conditional_factory(precision=4.0)
    x = torch.from_numpy(truth.reshape(-1)[None, :] + 0.1 * rs.standard_normal((C, 3 * n))).to(dev)
    s = HMCSampler(cond, x, 0.001, 20, variable_name='coordinates', rng=DeviceRNG(0, dev))
    out['sample_ms n=%d C=%d' % (n, C)] = med(s.sample, 10)

n, C = 1100, 64
rs = np.random.RandomState(1)
truth = rs.standard_normal((n, 3)) * 2.0
d = np.sqrt(((truth[:, None, :] - truth[None, :, :]) ** 2).sum(-1))
ymat = torch.from_numpy(np.abs(d + 0.05 * rs.standard_normal((n, n)))).to(dev)
x = torch.from_numpy(truth.reshape(-1)[None, :] + 0.1 * rs.standard_normal((C, 3 * n))).to(dev)
out['grad_unpacked_ms n=%d C=%d' % (n, C)] = med(lambda: _native.pairdist_gauss_grad(x, ymat, 4.0), 10)
print(json.dumps(out))
