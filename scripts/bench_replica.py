"""The replica-exchange kernels (csrc/replica.hip) against binf_accept_select_f64 at the same
C x D in the same process -- an existing kernel that moves the same bytes, one row read and one
row written per chain -- and a whole swap round against one sample() of the inner sampler at
BASELINE's C5 (2048 chains x 256 beads) and C2 (4096 x 1024 Gaussian) shapes.

Device events around windows of launches; the three kernels take turns window by window
(other people's work shares the host), the median window is reported with the spread.
Expectation (stated before any run): gather and swap each at most 1.15 x accept_select.
A report: no test depends on it.  Needs the GPU; writes one JSON file.

  python scripts/bench_replica.py --out profiles/r07_x_bench_replica.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from binf_amd import _native
from binf_amd.pdf import IsotropicGaussian
from binf_amd.samplers.hmc import HMCSampler
from binf_amd.samplers.replica import ReplicaExchangeSampler, geometric_betas, ladder_precision
from binf_amd.samplers.rng import DeviceRNG

EXPECTED_RATIO = 1.15
R = 4


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / n


def graphed(fn, n):
    """n launches of fn captured once as a HIP graph (the entry points are capturable): a replay
    is the kernels back to back, without the host's enqueue time between them."""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n):
            fn()
    return g.replay


def alternate(fns, n, repeats, warm=3, graph=False):
    """{name: sorted per-launch times of `repeats` windows of n launches}, the functions taking
    turns.  ``graph``: every window is one replay of the n captured launches."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    if graph:
        replays = dict((name, graphed(fn, n)) for name, fn in fns.items())
        for r in replays.values():
            r()
        torch.cuda.synchronize()
        times = dict((name, []) for name in fns)
        for _ in range(repeats):
            for name, r in replays.items():
                times[name].append(window(r, 1) / n)
        return dict((name, sorted(t)) for name, t in times.items())
    times = dict((name, []) for name in fns)
    for _ in range(repeats):
        for name, fn in fns.items():
            times[name].append(window(fn, n))
    return dict((name, sorted(t)) for name, t in times.items())


def kernels(C, D, dev, n, repeats):
    g = torch.Generator(device=dev).manual_seed(C + D)
    x = torch.randn((C, D), dtype=torch.float64, device=dev, generator=g)
    y = torch.randn((C, D), dtype=torch.float64, device=dev, generator=g)
    out = torch.empty_like(x)
    lp_own = torch.randn(C, dtype=torch.float64, device=dev, generator=g)
    lp_sw = torch.randn(C, dtype=torch.float64, device=dev, generator=g)
    u = torch.rand(C, dtype=torch.float64, device=dev, generator=g)
    acc = torch.empty(C, dtype=torch.uint8, device=dev)
    att = torch.zeros(C, dtype=torch.int64, device=dev)
    nacc = torch.zeros(C, dtype=torch.int64, device=dev)
    fns = {
        # e_after - e_before = lp_own - lp_sw: about half of the chains take the proposal's row
        'accept_select': lambda: _native.accept_select(x, y, lp_sw, lp_own, u, out, acc, nacc, None,
                                                       False, 1.05, 0.95),
        'gather': lambda: _native.replica_gather(x, R, 0, out=out),
        'swap': lambda: _native.replica_swap(x, lp_own, lp_sw, R, 0, acc, u=u, out=out, n_attempted=att,
                                             n_accepted=nacc),
        'swap_generated_u': lambda: _native.replica_swap(x, lp_own, lp_sw, R, 0, acc, out=out, n_attempted=att,
                                                         n_accepted=nacc, seed=1, offset=2),
    }
    nbytes = 16.0 * C * D
    res = {'bytes': nbytes, 'launches_per_window': n, 'windows': repeats}
    # 'graph_replay': kernel time (the figure the expectation is about); 'eager': what a Python
    # caller sees per launch, enqueue included
    for mode in ('graph_replay', 'eager'):
        t = alternate(fns, n, repeats, graph=mode == 'graph_replay')
        base = statistics.median(t['accept_select'])
        r = {}
        for name, ts in t.items():
            med = statistics.median(ts)
            r[name] = {'median_us': med * 1e6, 'min_us': ts[0] * 1e6, 'max_us': ts[-1] * 1e6,
                       'TBps': nbytes / med / 1e12, 'ratio_to_accept_select': med / base}
        r['meets_expectation'] = dict((name, r[name]['ratio_to_accept_select'] <= EXPECTED_RATIO)
                                      for name in ('gather', 'swap', 'swap_generated_u'))
        res[mode] = r
    return res


def round_vs_sample(inner, n_replicas, n, repeats):
    re = ReplicaExchangeSampler(inner, n_replicas)
    t = alternate({'sample': inner.sample, 'swap_round': re.swap}, n, repeats, warm=2)
    s, r = statistics.median(t['sample']), statistics.median(t['swap_round'])
    return {'sample_ms': s * 1e3, 'swap_round_ms': r * 1e3, 'round_over_sample': r / s,
            'chains': int(inner.state.shape[0]), 'dims': int(inner.state.shape[1]), 'n_replicas': n_replicas}


def c5(dev, chains=2048, beads=256, n_replicas=8):
    from binf_amd.example.distance import make_distance_likelihood
    from binf_amd.pdf.posteriors import Posterior
    rs = np.random.RandomState(0)
    truth = np.cumsum(rs.standard_normal((beads, 3)), axis=0) * 0.5
    I, J = np.triu_indices(beads, 1)
    ys = np.abs(np.sqrt(((truth[I] - truth[J]) ** 2).sum(1)) + 0.5 * rs.standard_normal(I.shape))
    lik = make_distance_likelihood(ys, beads)
    prior = IsotropicGaussian(0.01, 0.0, name='coordinates_prior', variable_name='coordinates')
    tau = ladder_precision(geometric_betas(n_replicas, 0.05), 4.0, chains // n_replicas, dev)
    cond = Posterior({lik.name: lik}, {prior.name: prior}).conditional_factory(precision=tau)
    rng = DeviceRNG(1, dev)
    start = torch.from_numpy(truth.reshape(1, -1)).to(dev) + 0.3 * rng.normal((chains, 3 * beads), dev)
    return HMCSampler(cond, start, 0.002, 20, variable_name='coordinates', rng=rng)


def c2(dev, chains=4096, dims=1024):
    rng = DeviceRNG(2, dev)
    return HMCSampler(IsotropicGaussian(), rng.normal((chains, dims), dev), 0.05, 20, variable_name='x', rng=rng)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'r07_x_bench_replica.json'))
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=15)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bench_replica: needs the GPU (nothing is measured on the host)')
    dev = torch.device('cuda', torch.cuda.current_device())
    out = {'expected_ratio': EXPECTED_RATIO, 'n_replicas': R, 'kernels': {}}
    for C, D in ((4096, 1024), (2048, 768), (4096, 33)):
        out['kernels']['%dx%d' % (C, D)] = kernels(C, D, dev, args.launches, args.repeats)
    out['round_vs_sample'] = {'C5': round_vs_sample(c5(dev), 8, 20, 7), 'C2': round_vs_sample(c2(dev), 8, 20, 7)}
    text = json.dumps(out, indent=1, sort_keys=True)
    d = os.path.dirname(args.out)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
