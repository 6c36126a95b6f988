#!/usr/bin/env python3
"""The no-U-turn sampler's tree kernel and transition, measured (nothing here is a bar).

1. ``binf_nuts_leaf_f64`` beside ``binf_leapfrog_kick_drift_f64`` (40 B per element) at the same
   C x D, even and odd leaves separately.  Every timed call gets device events of its own, the
   candidates take turns, medians with [min, max].  Expected from the bytes a leaf moves per
   element (stated before the run, printed beside the result):
     even leaf  the dot pass reads r (8); the row pass reads q, r, rho_sub and writes rho_sub and
                the two checkpoint rows (48; r again from cache): 56 B, 1.4x kick_drift -- 64 B
                (1.6x) where the leaf also becomes the candidate;
     odd leaf   the dot pass reads r, rho_sub and one checkpoint pair per level (32 at one
                level); the row pass reads q, r, rho_sub and writes rho_sub (32): 64 B, 1.6x.
2. ``NUTSSampler`` beside ``HMCSampler`` on the per-step tier with ``nsteps`` = the measured mean
   ``n_leapfrog`` over chains and transitions, on the same torch PDF: time per transition, leapfrog
   steps per chain and second (a chain's own steps: the useful work) and, for NUTS, launch rounds
   per second (every transition launches as many leaves as its LONGEST tree has).
3. The share of a NUTS transition spent in the ``pending`` read-backs: the number of read-backs
   times the cost of one (launch, copy of 8 bytes, wait), measured on an idle queue.

Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from binf_amd import _native
from binf_amd.samplers import NUTSSampler
from binf_amd.samplers.hmc import HMCSampler
from binf_amd.samplers.rng import DeviceRNG


def stats(x):
    return dict(median=float(np.median(x)), min=float(np.min(x)), max=float(np.max(x)))


def leaf_bench(C, D, md, reps, dev):
    ws = {n: torch.zeros(shape, dtype=dtype, device=dev) for n, (shape, dtype) in _native.nuts_shapes(C, D, md).items()}
    a = _native.nuts_args(ws, C, D, md)
    for n in ('q', 'r', 'g', 'rho_sub', 'rho_tree', 'ck_r', 'edge_r', 'cand', 'prop'):
        ws[n].copy_(torch.rand(ws[n].shape, dtype=torch.float64, device=dev) + 0.1)    # every dot positive
    ws['eps'].fill_(0.1)
    ws['u'].fill_(0.999)                               # the leaf does not become the candidate
    H0 = 0.5 * (ws['r'] * ws['r']).sum(dim=1)
    q, p, g = (torch.randn(C, D, dtype=torch.float64, device=dev) for _ in range(3))

    def reset(n_sub):
        ws['n_sub'].fill_(n_sub); ws['j'].fill_(3); ws['status'].fill_(0); ws['n_leap'].fill_(n_sub)
        ws['w_sub'].fill_(float(n_sub)); ws['w_tree'].fill_(1.0); ws['acc'].fill_(0.0)
        ws['H0'].copy_(H0); ws['href'].copy_(H0); ws['v'].fill_(1)

    cands = {'leaf_even': lambda: _native.nuts_leaf(a, dev), 'leaf_odd_1_level': lambda: _native.nuts_leaf(a, dev),
             'leaf_odd_2_levels': lambda: _native.nuts_leaf(a, dev),
             'kick_drift': lambda: _native.leapfrog_kick_drift(q, p, g, 1e-4)}
    start = {'leaf_even': 2, 'leaf_odd_1_level': 1, 'leaf_odd_2_levels': 3, 'kick_drift': None}
    times = {k: [] for k in cands}
    for rep in range(reps + 3):
        for name, fn in cands.items():                 # the candidates take turns
            if start[name] is not None:
                reset(start[name])
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if rep >= 3:
                times[name].append(e0.elapsed_time(e1) * 1e3)
            if start[name] is not None:
                assert int((ws['status'] != 0).sum()) == 0, 'a chain left the timed path'
    base = np.median(times['kick_drift'])
    expected = {'leaf_even': 56.0 / 40.0, 'leaf_odd_1_level': 64.0 / 40.0, 'leaf_odd_2_levels': 80.0 / 40.0}
    for name in cands:
        row = dict(bench='leaf', chains=C, dims=D, kernel=name, us=stats(times[name]))
        if name in expected:
            row.update(over_kick_drift=float(np.median(times[name]) / base), expected_from_bytes=expected[name])
        print(json.dumps(row), flush=True)


class DiagGauss(object):
    def __init__(self, sigma):
        self.sigma = sigma

    def log_prob(self, x):
        z = x / self.sigma
        return -0.5 * (z * z).sum(dim=1)

    def gradient(self, x):
        return x / (self.sigma * self.sigma)


def transition_bench(C, D, md, n, dev):
    sigma = torch.tensor(np.exp(np.linspace(0.0, np.log(10.0), D)), dtype=torch.float64, device=dev)
    x0 = sigma * torch.randn(C, D, dtype=torch.float64, device=dev)
    pdf = DiagGauss(sigma)
    s = NUTSSampler(pdf, x0.clone(), 0.5, max_tree_depth=md, variable_name='x', rng=DeviceRNG(1, dev))
    for _ in range(3):
        s.sample()
    torch.cuda.synchronize()
    leaps, rounds, t = [], [], []
    for _ in range(n):
        t0 = time.perf_counter()
        s.sample()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e6)
        leaps.append(float(s.last_n_leapfrog.double().mean()))     # the useful work: steps of a chain's own tree
        rounds.append(int(s.last_n_leapfrog.max()))                # launch rounds follow the longest tree
    mean_leap, mean_rounds = float(np.mean(leaps)), float(np.mean(rounds))
    # a read-back after leaf totals 1, 3, 7, ... up to the first total at or beyond the longest tree
    reads = float(np.mean([int(np.ceil(np.log2(r + 1))) for r in rounds]))
    ws = s._ws
    one = []
    for _ in range(50):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _native.nuts_pending(ws['status'], ws['count'])
        ws['count'].item()
        one.append((time.perf_counter() - t0) * 1e6)
    h = HMCSampler(pdf, x0.clone(), 0.5, max(1, int(round(mean_leap))), variable_name='x', rng=DeviceRNG(1, dev))
    h.fused_transition = False
    for _ in range(3):
        h.sample()
    torch.cuda.synchronize()
    th = []
    for _ in range(n):
        t0 = time.perf_counter()
        h.sample()
        torch.cuda.synchronize()
        th.append((time.perf_counter() - t0) * 1e6)
    print(json.dumps(dict(
        bench='transition', chains=C, dims=D, max_tree_depth=md, n_leapfrog_mean=mean_leap,
        launch_rounds_mean=mean_rounds, nuts_us=stats(t),
        nuts_leapfrog_per_chain_per_s=mean_leap / (np.median(t) * 1e-6),
        nuts_launch_rounds_per_s=mean_rounds / (np.median(t) * 1e-6),
        hmc_nsteps=h.nsteps, hmc_us=stats(th), hmc_leapfrog_per_chain_per_s=h.nsteps / (np.median(th) * 1e-6),
        pending_reads_per_transition=reads, pending_read_us=stats(one),
        pending_share=float(reads * np.median(one) / np.median(t)))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--chains', type=int, default=4096)
    ap.add_argument('--dims', type=int, nargs='+', default=[1024, 33])
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--transitions', type=int, default=30)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    for D in a.dims:
        leaf_bench(a.chains, D, 6, a.reps, dev)
    for D in a.dims:
        transition_bench(a.chains, D, 6, a.transitions, dev)


if __name__ == '__main__':
    main()
