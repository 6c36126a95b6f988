"""CPU tests of the replica exchange: the pairing, exact detailed balance of the restated
swap, the committed GPU cases (every decision outside the device test's margin), ladder
sharding and the ladder helpers, and the double-well mixing run in numpy inside the bounds
the GPU test uses (tests/test_gpu_replica_exchange.py)."""
import itertools

import numpy as np
import pytest

import replica_exchange as RX
from binf_amd.dist import shard_chains, shard_ladders
from binf_amd.samplers.replica import geometric_betas, ladder_precision


@pytest.mark.parametrize('R', range(1, 10))
@pytest.mark.parametrize('n_ladders', [1, 3])
def test_partner_is_a_neighbour_pairing_inside_the_ladder(R, n_ladders):
    C = R * n_ladders
    c = np.arange(C)
    attempted = np.zeros(C, dtype=np.int64)
    for parity in (0, 1):
        p = RX.partner(C, R, parity)
        assert np.array_equal(p[p], c)                              # an involution
        assert np.array_equal(p // R, c // R)                       # confined to its ladder
        low = RX.lower_members(C, R, parity)
        # exactly the slots stated: r >= parity, (r - parity) even, r + 1 < R
        want = np.array([(r >= parity) and ((r - parity) % 2 == 0) and (r + 1 < R) for r in c % R])
        assert np.array_equal(low, want)
        assert np.array_equal(p[low], c[low] + 1) and np.array_equal(p[c[low] + 1], c[low])
        paired = low.copy()
        paired[c[low] + 1] = True
        assert np.array_equal(p[~paired], c[~paired])               # everyone else: itself
        assert not np.any(low & np.roll(low, 1)) or R == 1          # pairs are disjoint
        attempted += low
    # over two consecutive parities every neighbour pair (r, r + 1) is attempted once
    assert np.array_equal(attempted, (c % R + 1 < R).astype(np.int64))


def _flows(lp, sign):
    """pi(a,b) A((a,b)->(b,a)) for all joint states of two replicas over the states of the
    tables lp[0], lp[1] (log-probs of replica 0 / 1); A = min(1, accept_probability(delta))
    -- u is uniform in [0, 1) -- with delta restated here, times ``sign``."""
    n = lp.shape[1]
    pi, flow = np.zeros((n, n)), np.zeros((n, n))
    for a, b in itertools.product(range(n), repeat=2):
        lp_own = np.array([lp[0, a], lp[1, b]])
        lp_sw = np.array([lp[0, b], lp[1, a]])
        delta = sign * RX.pair_delta(lp_own, lp_sw, np.array([0]))[0]
        A = RX.accept_probability(delta)
        A = 0.0 if np.isnan(A) else min(1.0, A)                     # NaN rejects
        with np.errstate(invalid='ignore'):
            pi[a, b] = np.exp(lp[0, a] + lp[1, b])
        flow[a, b] = pi[a, b] * A
    return pi, flow


def _balanced(pi, flow):
    """Every flow (a,b)->(b,a) equals its reverse to 1e-15 of the larger of the two
    stationary weights (a state of weight 0 is entered at the clip's floor e^-308, not at
    0: that is the accept function's documented clip, 1e-134 of the weight)."""
    scale = np.maximum(pi, pi.T)
    return bool(np.all(np.abs(flow - flow.T) <= 1e-15 * scale))


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_exact_detailed_balance_of_the_restated_swap(seed):
    """Two replicas over a 4-point state space, arbitrary log-prob tables with a -inf entry:
    all 16 joint states.  The entries are random multiples of 1/8, so that the sums and
    delta are exact and the only roundings are those of exp and one product: at most
    3.5 ulp = 7.8e-16 between the two sides."""
    rs = np.random.RandomState(seed)
    lp = rs.randint(-40, 9, size=(2, 4)) / 8.0
    lp[rs.randint(2), rs.randint(4)] = -np.inf
    pi, flow = _flows(lp, +1.0)
    assert np.count_nonzero(pi == 0.0) == 4 and np.count_nonzero(flow) >= 6
    assert _balanced(pi, flow)
    # the same check sees a wrong sign of delta
    pi_bad, flow_bad = _flows(lp, -1.0)
    assert not _balanced(pi_bad, flow_bad)


def test_the_committed_gpu_cases_are_decisive():
    """Every random case the GPU test holds the kernel to, bit for bit: no pair's |u - e^delta|
    within 2**-40 -- supplied and generated uniforms, both parities."""
    n_acc = n_rej = 0
    for R in RX.CASE_R:
        for n_ladders in RX.CASE_LADDERS:
            k = RX.case_inputs(R, n_ladders)
            ug = RX.generated_uniforms(k['seed'], k['offset'], k['chain_offset'], k['C'])
            assert ug.shape == (k['C'],) and np.all((ug >= 0.0) & (ug < 1.0))
            for parity in (0, 1):
                for u in (k['u'], ug):
                    assert RX.decisive(k['lp_own'], k['lp_sw'], u, R, parity), (R, n_ladders, parity)
                    _, acc = RX.swap_round(np.zeros((k['C'], 1)), k['lp_own'], k['lp_sw'], u, R, parity)
                    low = RX.lower_members(k['C'], R, parity)
                    n_acc += int(acc[low].sum())
                    n_rej += int(low.sum() - acc[low].sum())
    assert n_acc > 100 and n_rej > 100                              # both branches are exercised


def test_swap_round_bookkeeping():
    R, C = 3, 6
    x = np.arange(C * 2, dtype=np.float64).reshape(C, 2)
    lp_own = np.zeros(C)
    lp_sw = np.array([1.0, 1.0, 0.0, -50.0, -50.0, 0.0])            # ladder 0 accepts, ladder 1 rejects
    u = np.full(C, 0.5)
    att, acc = np.full(C, 10, dtype=np.int64), np.full(C, 3, dtype=np.int64)
    walker = np.arange(C, dtype=np.int64)
    out, flags = RX.swap_round(x, lp_own, lp_sw, u, R, 0, (att, acc), walker)
    assert flags.tolist() == [1, 1, 0, 0, 0, 0]
    assert np.array_equal(out, x[[1, 0, 2, 3, 4, 5]])
    assert att.tolist() == [11, 10, 10, 11, 10, 10] and acc.tolist() == [4, 3, 3, 3, 3, 3]
    assert walker.tolist() == [1, 0, 2, 3, 4, 5]
    # NaN rejects; delta = 0 accepts u < 1
    lp_sw[0] = np.nan
    assert RX.swap_round(x, lp_own, lp_sw, u, R, 0)[1].tolist() == [0] * 6
    assert RX.swap_round(x, lp_own, lp_own, u, R, 1)[1].tolist() == [0, 1, 1, 0, 1, 1]


def test_shard_ladders():
    for n_ladders, R, ws in [(8, 3, 2), (7, 4, 3), (5, 6, 8), (0, 3, 2), (37, 1, 4)]:
        blocks = [shard_ladders(n_ladders, R, r, ws) for r in range(ws)]
        pos = 0
        for r, (start, count) in enumerate(blocks):
            assert start == pos and start % R == 0 and count % R == 0   # tiles; whole ladders
            assert (start // R, count // R) == shard_chains(n_ladders, r, ws)
            pos += count
        assert pos == n_ladders * R
        counts = [b[1] // R for b in blocks]
        assert max(counts) - min(counts) <= 1                           # uneven counts: by one ladder
    assert shard_ladders(7, 4, 0, 3) == (0, 12) and shard_ladders(7, 4, 2, 3) == (20, 8)
    for bad in [(-1, 3, 0, 2), (4, 0, 0, 2), (4, 3, 2, 2), (4, 3, 0, 0), (4, 2.5, 0, 2)]:
        with pytest.raises(ValueError):
            shard_ladders(*bad)


def test_geometric_betas_and_ladder_precision():
    assert geometric_betas(1, 0.1) == [1.0]
    assert geometric_betas(2, 0.25) == [1.0, 0.25]
    b = geometric_betas(5, 1.0 / 16.0)
    assert b == [1.0, 0.5, 0.25, 0.125, 0.0625]
    b = geometric_betas(4, 0.03)
    assert b[0] == 1.0 and b[-1] == 0.03 and np.allclose(np.array(b[1:]) / np.array(b[:-1]), 0.03 ** (1.0 / 3.0), rtol=1e-15)
    for bad in [(0, 0.5), (3, 0.0), (3, 1.5)]:
        with pytest.raises(ValueError):
            geometric_betas(*bad)
    p = ladder_precision([1.0, 0.5, 0.3], 7.0, 2)
    assert p.dtype.is_floating_point and p.element_size() == 8
    assert p.tolist() == [7.0, 3.5, 0.3 * 7.0, 7.0, 3.5, 0.3 * 7.0]
    assert ladder_precision([1.0], 2.0, 0).numel() == 0


@pytest.mark.parametrize('seed', [11, 12, 13])
def test_double_well_mixes_with_swaps_only(seed):
    """The run of the GPU mixing test, in numpy: with swaps the cold slot's fraction at x < 0
    is within 5 sigma = 0.11 of 0.5 after 150 rounds; without them it stays below 0.02."""
    f = RX.double_well_run(seed)
    stuck = RX.double_well_run(seed, swaps=False)
    print('seed %d: %.4f with swaps, %.4f without' % (seed, f, stuck))
    assert abs(5.0 * RX.DW_SIGMA - RX.DW_BOUND) < 1e-3
    assert abs(f - 0.5) <= RX.DW_BOUND
    assert stuck < RX.DW_STUCK
