"""The replica-exchange kernels on a batch beyond 2**32 elements (the pattern of
tests/test_gpu_large_batch.py): 4 194 308 chains x 1024 doubles, R = 4, through gather and
swap with generated uniforms.  Ladders never interact and every draw is keyed by the GLOBAL
chain index, so the first ladders, the ladders straddling flat index 2**32 and the last
ladders, recomputed as small batches with their ``chain_offset`` (bit-identical to the host
restatement at such sizes: tests/test_gpu_replica_exchange.py), must reproduce the big run's
rows bit for bit."""
import pytest
import torch

from binf_amd import _native
from binf_amd.samplers.rng import DeviceRNG

pytestmark = pytest.mark.gpu

D, R = 1024, 4
EDGE = (1 << 32) // D                    # the chain whose first element has flat index 2**32
C_BIG = EDGE + 4                         # 4 194 308 chains, a whole number of ladders
GIB = float(1 << 30)


def test_gather_and_swap_beyond_2_32_elements(device):
    free, _ = torch.cuda.mem_get_info(device)
    if free < 80 * GIB:
        pytest.skip('needs 80 GiB of free HBM, %.0f free' % (free / GIB))
    assert C_BIG % R == 0 and C_BIG * D > 1 << 32
    rng = DeviceRNG(11, device)
    x = rng.normal((C_BIG, D), device)
    lp_own = rng.normal((C_BIG,), device) - 40.0
    lp_sw = rng.normal((C_BIG,), device) - 40.0
    seed, offset = 99, (1 << 33) + 7
    w = 40 * R
    windows = [(0, w), (EDGE - w, EDGE + 4), (C_BIG - w, C_BIG)]
    ids = torch.arange(C_BIG, dtype=torch.int64, device=device)
    try:
        for parity in (0, 1):
            gathered = _native.replica_gather(x, R, parity)
            for a, b in windows:
                assert torch.equal(_native.replica_gather(x[a:b].clone(), R, parity), gathered[a:b]), (parity, a, b)
            del gathered
            acc = torch.empty(C_BIG, dtype=torch.uint8, device=device)
            att = torch.full((C_BIG,), 5, dtype=torch.int64, device=device)
            nac = torch.full((C_BIG,), 2, dtype=torch.int64, device=device)
            walker = ids.clone()
            out = _native.replica_swap(x, lp_own, lp_sw, R, parity, acc, n_attempted=att, n_accepted=nac,
                                       walker=walker, seed=seed, offset=offset)
            rate = float(acc.double().mean())
            assert 0.2 < rate < 0.8, rate
            for a, b in windows:
                n = b - a
                acc_w = torch.empty(n, dtype=torch.uint8, device=device)
                att_w = torch.full((n,), 5, dtype=torch.int64, device=device)
                nac_w = torch.full((n,), 2, dtype=torch.int64, device=device)
                walker_w = ids[a:b].clone()
                out_w = _native.replica_swap(x[a:b].clone(), lp_own[a:b].clone(), lp_sw[a:b].clone(), R, parity,
                                             acc_w, n_attempted=att_w, n_accepted=nac_w, walker=walker_w,
                                             seed=seed, offset=offset, chain_offset=a)
                assert torch.equal(out_w, out[a:b]), (parity, a, b)
                assert torch.equal(acc_w, acc[a:b]) and torch.equal(att_w, att[a:b]) and torch.equal(nac_w, nac[a:b])
                assert torch.equal(walker_w, walker[a:b])
            # an accepted pair exchanged its rows, every other chain kept its own -- over the whole batch
            moved = (out != x).any(dim=1)
            assert torch.equal(moved, acc.bool())
            del out, moved
    finally:
        del x
        torch.cuda.empty_cache()
