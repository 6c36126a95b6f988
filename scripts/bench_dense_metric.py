#!/usr/bin/env python3
"""The dense-metric kernels at 4096 chains, D = 32, 128, 256, G = 1 (bench_metric.py's sibling):

  binf_leapfrog_kick_drift_dense_f64 (FMA and EXACT mode) beside
  binf_leapfrog_kick_drift_scaled_f64 at the same shape, and beside the FP64 FMA floor of its
  C * D * (D + 1) multiply-adds: 256 CUs x 64 FMA per cycle at the shader clock read while the
  kernel runs (the nominal 2400 MHz where the clock cannot be read: `clock_source` says which);
  binf_metric_comoments_f64 beside the floor of its C * D * (D + 1) / 2 products + adds;
  binf_metric_factor_f64, once per window.

Device events around `reps` calls, median over rounds.  Prints one JSON line per D."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from binf_amd import _native

CUS, FMA_PER_CU_CYCLE, NOMINAL_MHZ = 256, 64, 2400.0


def device_us(fn, reps, rounds=5, probe=None):
    """Median over rounds of the device time of one call (events around `reps` calls)."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        if probe is not None:
            probe()                                   # while the queue is still busy
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--chains', type=int, default=4096)
    ap.add_argument('--dims', type=int, nargs='+', default=[32, 128, 256])
    ap.add_argument('--reps', type=int, default=100)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    C = a.chains
    clocks = []

    def probe():
        try:
            clocks.append(float(torch.cuda.clock_rate(dev)))
        except Exception:                             # noqa: BLE001 -- no SMI library: nominal clock
            pass
    for D in a.dims:
        q, p, g = (torch.randn(C, D, dtype=torch.float64, device=dev) for _ in range(3))
        scale = torch.rand(1, D, dtype=torch.float64, device=dev) + 0.5
        chol = torch.tril(torch.randn(D, D, dtype=torch.float64, device=dev)) / D ** 0.5
        del clocks[:]
        t_fma = device_us(lambda: _native.leapfrog_kick_drift_dense(q, p, g, chol, 1e-4, mode=_native.MODE_FMA), a.reps,
                          probe=probe)
        mhz = float(np.median(clocks)) if clocks else NOMINAL_MHZ
        t_exact = device_us(lambda: _native.leapfrog_kick_drift_dense(q, p, g, chol, 1e-4), a.reps)
        t_scaled = device_us(lambda: _native.leapfrog_kick_drift_scaled(q, p, g, scale, 1e-4), a.reps)
        per_us = CUS * FMA_PER_CU_CYCLE * mhz                          # multiply-adds per microsecond
        floor = C * D * (D + 1) / per_us
        x = torch.randn(C, D, dtype=torch.float64, device=dev)
        k0, s1 = (torch.zeros(1, D, dtype=torch.float64, device=dev) for _ in range(2))
        s2, work, L = (torch.zeros(1, D, D, dtype=torch.float64, device=dev) for _ in range(3))
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        _native.metric_comoments(x, k0, s1, s2, True)
        t_com = device_us(lambda: _native.metric_comoments(x, k0, s1, s2, False), a.reps)
        t_fac = device_us(lambda: _native.metric_factor(s1, s2, a.reps * 5 + 2, C, L, work, status), 10)
        assert int(status[0]) == 0
        print(json.dumps(dict(
            chains=C, dims=D, clock_mhz=mhz, clock_source='read under load' if clocks else 'nominal',
            kick_drift_dense_fma_us=t_fma, kick_drift_dense_exact_us=t_exact, kick_drift_scaled_us=t_scaled,
            dense_fma_over_scaled=t_fma / t_scaled, fma_floor_us=floor, dense_fma_over_floor=t_fma / floor,
            comoments_us=t_com, comoments_floor_us=C * D * (D + 1) / 2 / per_us,
            comoments_over_floor=t_com / (C * D * (D + 1) / 2 / per_us), factor_us=t_fac)), flush=True)


if __name__ == '__main__':
    main()
