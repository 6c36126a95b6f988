"""Randomised differential soak of the device draw streams (development aid, run on the
GPU): random seed, offset, window and shape of every stand-alone stream, random
(transitions, chains, D, chain offset) of the fused and the long-chain generator, each
held against the host restatement of tests/draw_streams.py -- bits where the value is an
exact product, the derived bound elsewhere; marginal decisions are counted, not compared.
  python tests/soak/fuzz_draws.py [n_cases] [seed]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import draw_streams as ds  # noqa: E402
from binf_amd import _native  # noqa: E402

dev = torch.device('cuda:0')
n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 100
rs = np.random.RandomState(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
bad = marginal = compared = 0
worst = {}
t0 = time.time()


def rand64(bits=64):
    return int(rs.randint(0, 2 ** 32)) << 32 & (2 ** bits - 1) | int(rs.randint(0, 2 ** 32))


def hold(what, got, d, **kw):
    global bad, marginal, compared
    rep = ds.compare(got, d)
    marginal += rep['marginal']
    compared += rep['n']
    worst[what] = max(worst.get(what, 0.0), rep['max_of_bound'])
    if len(rep['mismatches']):
        bad += 1
        print('MISMATCH', what, kw, ds.describe(rep, got, d), flush=True)


def window():
    e0 = int(rs.choice([0, 1, 2, 255, 12345, 2 ** 32 - 1, 2 ** 33 + 2, 2 ** 40 + 1])) + int(rs.randint(0, 4))
    n = int(rs.choice([1, 2, 3, 255, 1023, 1024, 1025, 4099, 65537, 300001]))
    return e0, n


def fill(kind, n, seed, off, e0, shape=None):
    shifted = rs.rand() < 0.5
    buf = torch.full((n + 2,), float('nan'), dtype=torch.float64, device=dev)
    out = buf[1:n + 1] if shifted else buf[:n]
    _native.rng_fill(kind, out, seed, off, shape=shape, elem_offset=e0)
    host = buf.cpu().numpy()
    if not np.isnan(np.concatenate([host[:1], host[n + 1:]]) if shifted else host[n:]).all():
        raise SystemExit('%s wrote outside its window: %r' % (kind, (n, seed, off, e0, shifted)))
    return host[1:n + 1] if shifted else host[:n]


for case in range(n_cases):
    seed, (e0, n) = rand64(), window()
    off = rand64()
    hold('uniform', fill('uniform', n, seed, off, e0), ds.uniform_stream(seed, off, e0, n), seed=seed, off=off, e0=e0, n=n)
    hold('normal', fill('normal', n, seed, off, e0), ds.box_muller_stream(seed, off, e0, n), seed=seed, off=off, e0=e0, n=n)
    zoff = rand64(48)
    hold('normal_zig', fill('normal_zig', n, seed, zoff, e0), ds.zig_stream(seed, zoff, e0, n),
         seed=seed, off=zoff, e0=e0, n=n)
    shape = float(rs.choice([0.01, 0.3, 0.5, 0.999, 1.0, 1.5, 2.5, 11.0, 500.5, 8193.0, 1e8])) * (1 + 0.1 * rs.rand())
    m = min(n, 65537)
    hold('gamma', fill('gamma', m, seed, off, e0, shape=shape), ds.gamma_stream(shape, seed, off, e0, m),
         seed=seed, off=off, e0=e0, n=m, shape=shape)
    D = int(rs.choice([1, 7, 8, 33, 64, 96, 127, 128, 129, 200, 258, 768, 920, 1000, 1023, 1024, 2048, 3000, 7000, 8192]))
    C = int(rs.randint(1, max(2, 200000 // D)))
    nt = int(rs.randint(1, 4))
    coff = int(rs.choice([0, 1, 11, 2 ** 33 + 5]))
    p0, u = _native.hmc_gauss_rng_draws(nt, C, D, seed, off, dev, chain_offset=coff)
    dp, du = ds.fused_streams(nt, C, D, seed, off, coff)
    hold('fused momenta', p0.cpu().numpy(), dp, nt=nt, C=C, D=D, seed=seed, off=off, coff=coff)
    hold('fused uniforms', u.cpu().numpy(), du, nt=nt, C=C, D=D, seed=seed, off=off, coff=coff)
    D = 8193 + int(rs.randint(0, 30000))
    C = int(rs.randint(1, 8))
    p0, u = _native.hmc_gauss_big_rng_draws(C, D, seed, off, dev, chain_offset=coff)
    dp, du = ds.big_streams(C, D, seed, off, coff)
    hold('long-chain momenta', p0.cpu().numpy(), dp, C=C, D=D, seed=seed, off=off, coff=coff)
    hold('long-chain uniforms', u.cpu().numpy(), du, C=C, D=D, seed=seed, off=off, coff=coff)
    if case % 20 == 19:
        print('%d cases, %d mismatches, %.0f s' % (case + 1, bad, time.time() - t0), flush=True)

print('fuzz_draws: %d cases, %d elements compared, %d marginal, %d mismatches, %.0f s'
      % (n_cases, compared, marginal, bad, time.time() - t0))
print('largest error as a fraction of its bound:', dict((k, round(v, 3)) for k, v in sorted(worst.items())))
sys.exit(1 if bad else 0)
