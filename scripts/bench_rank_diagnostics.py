"""The rank layer (csrc/ranks.hip) beside torch.sort.

  rank_normalise   the segmented sort, the ranks and the scatter of the normal scores, for a
                   [1000 x 4096 x 8] record (S = 4.1 M values per dimension, P = 2**22) and a
                   [400 x 64 x 1024] one (S = 25600, P = 2**15);
  torch.sort       of the same values, transposed to [D x S] beforehand (the transposition is
                   not timed): the yardstick, because nothing else in the library sorts;
  rank_summary     the whole composition at both shapes.

The bytes a pass of the sort moves are counted from the shapes: every compare-exchange pass
and every LDS tile pass reads and writes the 12 bytes of each of the D * P (key, index)
pairs.  Device events around windows of launches, the candidates taking turns, the median
window with the spread.  A report: no test depends on it.  Needs the GPU; writes one JSON file.

  python scripts/bench_rank_diagnostics.py --out profiles/r09_k_bench_rank_diagnostics.json
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
TILE = 8192


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


def sort_passes(P):
    """(passes over the workspace, passes through LDS tiles) of the network for P padded values."""
    if P <= TILE:
        return 0, 1
    glob, lds, k = 0, 1, 2 * TILE
    while k <= P:
        j = k // 2
        while j >= TILE:
            glob += 1
            j //= min(8, 2 * j // TILE)                 # up to three strides per pass
        lds += 1
        k *= 2
    return glob, lds


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--shapes', type=int, nargs='+', default=[1000, 4096, 8, 400, 64, 1024])
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--launches', type=int, default=3)
    args = ap.parse_args(argv)
    dev = torch.device('cuda', torch.cuda.current_device())
    res = {'device': torch.cuda.get_device_name(dev), 'cases': []}
    for T, C, D in zip(args.shapes[0::3], args.shapes[1::3], args.shapes[2::3]):
        draws = torch.randn((T, C, D), dtype=torch.float64, device=dev)
        S = 2 * (T // 2) * C
        P = 1 << (S - 1).bit_length()
        ztab = diagnostics.rank_z_table(S, dev)
        z = torch.empty((2 * (T // 2), C, D), dtype=torch.float64, device=dev)
        srt = torch.empty((D, S), dtype=torch.float64, device=dev)
        rows = draws[:2 * (T // 2)].reshape(S, D).t().contiguous()
        t = alternate({'rank_normalise': lambda: _native.rank_normalise(draws, 2, ztab, z=z),
                       'sorted_only': lambda: _native.rank_normalise(draws, 2, sorted_out=srt),
                       'torch_sort': lambda: torch.sort(rows, dim=1),
                       'rank_summary': lambda: diagnostics.rank_summary(draws),
                       'summary': lambda: diagnostics.summary(draws)}, args.launches, args.repeats)
        glob, lds = sort_passes(P)
        pass_bytes = 2 * 12 * D * P
        case = {'shape': [T, C, D], 'S': S, 'P': P, 'record_bytes': 8 * S * D, 'passes_over_workspace': glob,
                'passes_through_lds_tiles': lds, 'bytes_per_pass': pass_bytes,
                'sort_bytes': (glob + lds) * pass_bytes,
                'sort_floor_s_at_copy_ceiling': (glob + lds) * pass_bytes / HBM_COPY}
        for k, v in t.items():
            case[k] = report(v)
        case['rank_normalise']['over_torch_sort'] = case['rank_normalise']['median_s'] / case['torch_sort']['median_s']
        case['sorted_only']['of_sort_floor'] = case['sort_floor_s_at_copy_ceiling'] / case['sorted_only']['median_s']
        res['cases'].append(case)
        del draws, z, srt, rows
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    return res


if __name__ == '__main__':
    main()
