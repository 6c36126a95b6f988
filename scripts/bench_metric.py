#!/usr/bin/env python3
"""The diagonal-metric kernels at 4096 chains x 1024 dimensions, G = 1:
binf_leapfrog_kick_drift_scaled_f64 against binf_leapfrog_kick_drift_f64 (40 bytes per element
either way, plus the 8 KB scale row), binf_metric_accumulate_f64 (56 bytes per element) against
a device copy of the same bytes, and one sample() of the polynomial kind's coefficients (K = 4,
20 points, 50 leapfrog steps, per-step tier) with and without a metric.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from binf_amd import _native
from binf_amd.example.misc import make_posterior
from binf_amd.example.samplers import make_hmc_sampler
from binf_amd.samplers import BinfState
from binf_amd.samplers.rng import DeviceRNG


def device_us(fn, reps, rounds=5):
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
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    return float(np.median(out))


def poly_sampler(C, dev, metric):
    np.random.seed(0)
    xs = np.linspace(-2, 2, 20)
    poly = np.polynomial.polynomial.polyval
    ys = np.random.normal(loc=poly(xs, np.array([2.0, -4.0, 1.0, 1.5])), scale=1.0 / np.sqrt(2.5))
    st = BinfState(dict(coefficients=torch.ones((C, 4), dtype=torch.float64, device=dev),
                        precision=torch.ones(C, dtype=torch.float64, device=dev)))
    g = make_hmc_sampler(make_posterior(xs, ys, poly), 0.02, 50, st, rng=DeviceRNG(0, dev))
    s = g.subsamplers['coefficients']
    s.fused_transition = False                      # the per-step tier either way
    if metric:
        s.set_metric(torch.ones(4, dtype=torch.float64, device=dev))
    g._update_subsampler_states()
    g._update_conditional_pdf_params()
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--chains', type=int, default=4096)
    ap.add_argument('--dims', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=200)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    C, D = a.chains, a.dims
    q, p, g, k0, s1, s2 = (torch.randn(C, D, dtype=torch.float64, device=dev) for _ in range(6))
    scale = torch.rand(1, D, dtype=torch.float64, device=dev) + 0.5
    n = C * D
    t_plain = device_us(lambda: _native.leapfrog_kick_drift(q, p, g, 1e-3), a.reps)
    t_scaled = device_us(lambda: _native.leapfrog_kick_drift_scaled(q, p, g, scale, 1e-3), a.reps)
    _native.metric_accumulate(q, k0, s1, s2, True)
    t_acc = device_us(lambda: _native.metric_accumulate(q, k0, s1, s2, False), a.reps)
    src, dst = torch.empty(n * 56 // 16, dtype=torch.float64, device=dev), torch.empty(n * 56 // 16, dtype=torch.float64, device=dev)
    t_copy = device_us(lambda: dst.copy_(src), a.reps)       # reads 28 and writes 28 bytes per element: 56
    line = dict(chains=C, dims=D,
                kick_drift_us=t_plain, kick_drift_scaled_us=t_scaled, scaled_over_plain=t_scaled / t_plain,
                kick_drift_scaled_GBps=n * 40 / t_scaled / 1e3,
                accumulate_us=t_acc, accumulate_GBps=n * 56 / t_acc / 1e3,
                copy_same_bytes_us=t_copy, copy_GBps=n * 56 / t_copy / 1e3, accumulate_over_copy=t_acc / t_copy)
    for name, metric in (('poly_sample_us', False), ('poly_sample_metric_us', True)):
        s = poly_sampler(C, dev, metric)
        for _ in range(3):
            s.sample()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            s.sample()
        torch.cuda.synchronize()
        line[name] = (time.perf_counter() - t0) / 20 * 1e6
    print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
