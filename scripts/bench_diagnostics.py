"""The diagnostics kernels (csrc/diagnostics.hip) against their bounds.

  moments   one pass over a [256 x 4096 x 1024] record (8.6 GB) against the 6.29 TB/s copy
            ceiling, with torch.var_mean(draws, dim=0) -- what a user writes today -- taking
            turns with it window by window;
  autocov   the polynomial shape [1000 x 4096 x 34], max_lag = 64, split = 2, against the FP64
            VALU rate (39.3 T lane-operations/s: the contract's multiply and add are two);
  summary   the across-chain step and the whole `diagnostics.summary` at that shape.

Device events around windows of launches, the median window with the spread.  A report: no
test depends on it.  Needs the GPU; writes one JSON file.

  python scripts/bench_diagnostics.py --out profiles/r08_d_bench_diagnostics.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from binf_amd import _native, diagnostics

HBM_COPY = 6.29e12
FP64_LANE_OPS = 39.3e12


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / n


def alternate(fns, n, repeats, warm=2):
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            times[k].append(window(fn, n))
    return {k: sorted(v) for k, v in times.items()}


def report(t):
    return dict(median_s=statistics.median(t), min_s=t[0], max_s=t[-1])


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--store', type=int, nargs=3, default=[256, 4096, 1024])
    ap.add_argument('--poly', type=int, nargs=3, default=[1000, 4096, 34])
    ap.add_argument('--max-lag', type=int, default=64)
    ap.add_argument('--repeats', type=int, default=7)
    args = ap.parse_args(argv)
    dev = torch.device('cuda', torch.cuda.current_device())
    res = {'device': torch.cuda.get_device_name(dev)}

    T, C, D = args.store
    draws = torch.randn((T, C, D), dtype=torch.float64, device=dev)
    nbytes = T * C * D * 8
    t = alternate({'moments_split1': lambda: _native.chain_moments(draws, 1),
                   'moments_split2': lambda: _native.chain_moments(draws, 2),
                   'torch_var_mean': lambda: torch.var_mean(draws, dim=0)}, 10, args.repeats)
    res['moments'] = {'shape': [T, C, D], 'bytes': nbytes}
    for k, v in t.items():
        r = report(v)
        r['bytes_per_s'] = nbytes / r['median_s']
        r['of_copy_ceiling'] = r['bytes_per_s'] / HBM_COPY
        res['moments'][k] = r
    del draws

    T, C, D = args.poly
    K = args.max_lag
    draws = torch.randn((T, C, D), dtype=torch.float64, device=dev)
    n, M = T // 2, 2 * C
    mean, m2 = _native.chain_moments(draws, 2)
    part = _native.chain_autocov(draws, mean, 2, K)
    t = alternate({'autocov': lambda: _native.chain_autocov(draws, mean, 2, K),
                   'moments': lambda: _native.chain_moments(draws, 2),
                   'summary_step': lambda: _native.diag_summary(mean, m2, part, n),
                   'summary_whole': lambda: diagnostics.summary(draws, max_lag=K)}, 10, args.repeats)
    terms = M * D * sum(n - k for k in range(K + 1))
    res['autocov'] = {'shape': [T, C, D], 'max_lag': K, 'split': 2, 'multiply_adds': terms}
    for k, v in t.items():
        res['autocov'][k] = report(v)
    a = res['autocov']['autocov']
    a['lane_ops_per_s'] = 2 * terms / a['median_s']
    a['of_fp64_valu'] = a['lane_ops_per_s'] / FP64_LANE_OPS
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    return res


if __name__ == '__main__':
    main()
