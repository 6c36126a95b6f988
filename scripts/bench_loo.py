#!/usr/bin/env python3
"""Times of the three stages of loo() -- the pointwise record, the sort per observation, the
PSIS kernels -- at S = 51200 draws x N in {150, 16384} observations, with the numpy
restatement of ONE observation on one host core beside them (tests/loo_ref.py; its time is
per column, the device's for all N).  Device times are medians over --repeat runs between
device events after a warm-up; the numbers go to DESIGN.md, none is a threshold.

  python scripts/bench_loo.py [--repeat 5] [--json out.json]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from binf_amd import _native  # noqa: E402


def timed(fn, repeat):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--S', type=int, default=51200)
    ap.add_argument('--N', type=int, nargs='+', default=[150, 16384])
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--json', default=None)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), 'bench_loo.py needs a GPU'
    dev = torch.device('cuda:0')
    import loo_ref as R
    S, rows = args.S, []
    for N in args.N:
        g = torch.Generator(device=dev).manual_seed(N)
        c = torch.randn((S, 4), dtype=torch.float64, device=dev, generator=g) * 0.05 + \
            torch.tensor([2.0, -4.0, 1.0, 1.5], dtype=torch.float64, device=dev)
        tau = 2.5 + 0.3 * torch.rand(S, dtype=torch.float64, device=dev, generator=g)
        xs = torch.linspace(-2, 2, N, dtype=torch.float64, device=dev)
        mock = _native.poly_forward(c, xs)
        ys = mock[0] + torch.randn(N, dtype=torch.float64, device=dev, generator=g) / math.sqrt(2.5)
        t_rec, ll = timed(lambda: _native.gauss_pointwise_loglik(mock, tau, ys, R.HALF_LOG_2PI), args.repeat)
        draws = ll.unsqueeze(1)
        t_sort, srt = timed(lambda: _native.rank_normalise(draws, 1, want_sorted=True)[0], args.repeat)
        t_psis, out = timed(lambda: _native.psis_loo(srt), args.repeat)
        col = srt[N // 2].cpu().numpy()
        t0 = time.perf_counter()
        ref = R.psis_column(col)
        t_host = (time.perf_counter() - t0) * 1e3
        M, m, _ = R.plan(S)
        row = dict(S=S, N=N, tail_len=M, candidates=m, record_ms=t_rec, sort_ms=t_sort, psis_ms=t_psis,
                   host_one_column_ms=t_host, host_all_columns_s=t_host * N / 1e3,
                   record_GBps=16.0 * S * N / t_rec / 1e6, psis_exp_per_s=2.0 * S * N / t_psis * 1e3,
                   khat_dev=float(out['khat'][N // 2]), khat_host=float(ref['khat']),
                   elpd_dev=float(out['elpd_loo'][N // 2]), elpd_host=float(ref['elpd_loo']))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(rows, fh, indent=1)


if __name__ == '__main__':
    main()
