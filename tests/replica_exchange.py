"""Host restatement (numpy) of the replica exchange of ``csrc/replica.hip`` /
``binf_amd/samplers/replica.py``, written from the contract in ``include/binf_hip.h``:
the pairing, the gather, one swap round with its flags, counters and walker ids, and the
double-well run the mixing tests use.  Nothing here calls into the library.

C = n_ladders * R chains, chain c is slot r = c % R of ladder c // R.  In a round of
``parity`` slot r is the lower member of the pair (r, r + 1) iff r >= parity, (r - parity)
is even and r + 1 < R.  For a pair (i, j = i + 1)

    delta  = (lp_sw[i] + lp_sw[j]) - (lp_own[i] + lp_own[j])      (three roundings)
    accept = u[i] < exp(clip(delta, -308, 709))                   (NaN rejects)

The device evaluates the exponential with its own polynomial (``gauss_common.hpp``), within
an ulp of numpy's; its accept shortcut carries a margin of 2**-40.  A decision is therefore
only pinned where ``|u - e^delta|`` exceeds 2**-40 (relative to max(1, e^delta)):
:func:`decisive` says so, and the committed cases are checked with it on the CPU
(``tests/test_replica_exchange.py``).
"""
import numpy as np

from draw_streams import uniform_stream

MARGIN = 2.0 ** -40


def lower_members(C, R, parity):
    """[C] bool: chain c is the lower member of a pair in this round."""
    assert R >= 1 and C % R == 0 and parity in (0, 1)
    r = np.arange(C, dtype=np.int64) % R
    return (r >= parity) & ((r - parity) % 2 == 0) & (r + 1 < R)


def partner(C, R, parity):
    """[C] int64: the other member of c's pair, c itself for an unpaired chain."""
    p = np.arange(C, dtype=np.int64)
    low = np.nonzero(lower_members(C, R, parity))[0]
    p[low], p[low + 1] = low + 1, low
    return p


def gather(x, R, parity):
    return x[partner(x.shape[0], R, parity)]


def pair_delta(lp_own, lp_sw, i):
    """delta of the pairs whose lower members are i (array of indices)."""
    with np.errstate(invalid='ignore'):
        return (lp_sw[i] + lp_sw[i + 1]) - (lp_own[i] + lp_own[i + 1])


def accept_probability(delta):
    """exp(clip(delta, -308, 709)): what u is compared with (NaN stays NaN)."""
    with np.errstate(invalid='ignore'):
        return np.exp(np.clip(delta, -308.0, 709.0))


def generated_uniforms(seed, offset, chain_offset, C):
    """u == NULL: the pair with lower member i reads element chain_offset + i of the uniform
    stream (seed, offset)."""
    return uniform_stream(seed, offset, chain_offset, C).ref


def swap_round(x, lp_own, lp_sw, u, R, parity, counters=None, walker=None):
    """One round: returns (out [C x D], accepted [C] uint8).  ``counters`` = (n_attempted,
    n_accepted) int64 [C] and ``walker`` int64 [C] are updated IN PLACE (lower member only /
    the two entries of an accepted pair exchanged)."""
    C = x.shape[0]
    low = np.nonzero(lower_members(C, R, parity))[0]
    with np.errstate(invalid='ignore'):
        acc = u[low] < accept_probability(pair_delta(lp_own, lp_sw, low))
    accepted = np.zeros(C, dtype=np.uint8)
    accepted[low[acc]] = 1
    accepted[low[acc] + 1] = 1
    src = np.where(accepted == 1, partner(C, R, parity), np.arange(C, dtype=np.int64))
    out = x[src]
    if counters is not None:
        counters[0][low] += 1
        counters[1][low[acc]] += 1
    if walker is not None:
        walker[:] = walker[src]
    return out, accepted


def decisive(lp_own, lp_sw, u, R, parity):
    """True if every pair's decision is outside the device test's margin: |u - p| > 2**-40 *
    max(1, p), or p is NaN (rejected whatever u is)."""
    C = lp_own.shape[0]
    low = np.nonzero(lower_members(C, R, parity))[0]
    p = accept_probability(pair_delta(lp_own, lp_sw, low))
    with np.errstate(invalid='ignore'):
        ok = np.isnan(p) | (np.abs(u[low] - p) > MARGIN * np.maximum(1.0, p))
    return bool(np.all(ok))


# ---------------------------------------------------------------------------
# The random cases of tests/test_gpu_replica_exchange.py: log-probs that give a mix of
# accepted and rejected pairs, a supplied uniform per chain, and a Philox stream position
# for the generated ones.  One seed per (R, n_ladders); tests/test_replica_exchange.py
# asserts that every one of them is decisive for both parities and both kinds of draw.
# ---------------------------------------------------------------------------
CASE_R = (1, 2, 3, 4, 5)
CASE_LADDERS = (1, 3, 37)
CASE_D = (0, 1, 2, 3, 7, 8, 33, 255, 256, 257, 768, 1025)
PHILOX_SEED = (1 << 40) + 4711


def case_inputs(R, n_ladders):
    C = R * n_ladders
    rs = np.random.RandomState(7000 + 100 * R + n_ladders)
    return dict(C=C, lp_own=rs.standard_normal(C) * 2.0 - 30.0, lp_sw=rs.standard_normal(C) * 2.0 - 30.0,
                u=rs.random_sample(C), seed=PHILOX_SEED + R, offset=(1 << 33) + n_ladders,
                chain_offset=5 * R)


def case_rows(C, D, salt=0):
    """The [C x D] state of a case: distinct values, so a row from the wrong chain shows."""
    return np.random.RandomState(9000 + salt).standard_normal((C, D)) if D else np.zeros((C, 0))


# ---------------------------------------------------------------------------
# The double-well run of the mixing tests, in numpy: HMC (velocity Verlet, the reference's
# hmc.py:113-125) on log p_c(x) = -beta_c a (x^2 - 1)^2, D = 1, with the swap above.
# ---------------------------------------------------------------------------
DW_A = 16.0
DW_BETAS = (1.0, 0.5, 0.25, 0.12, 0.06, 0.03)
DW_LADDERS, DW_DT, DW_STEPS, DW_TRANSITIONS, DW_ROUNDS = 512, 0.07, 8, 2, 150
DW_SIGMA = 0.5 / np.sqrt(DW_LADDERS)
DW_BOUND = 0.11            # 5 sigma = 0.1105 of the cold slot's fraction at x < 0 around 0.5
DW_STUCK = 0.02            # without swaps: all but a few of the 512 cold chains stay at x > 0


def double_well_log_prob(x, beta):
    w = x * x - 1.0
    return -(beta * DW_A) * (w * w)


def double_well_gradient(x, beta):
    return (4.0 * DW_A) * beta * x * (x * x - 1.0)


def double_well_run(seed, swaps=True, rounds=DW_ROUNDS):
    """Fraction of the cold slot's chains at x < 0 after ``rounds`` rounds, every chain
    started at x = +1."""
    rs = np.random.RandomState(seed)
    R = len(DW_BETAS)
    C = DW_LADDERS * R
    beta = np.tile(np.array(DW_BETAS), DW_LADDERS)
    x = np.ones(C)
    for rnd in range(rounds):
        for _ in range(DW_TRANSITIONS):
            p = rs.standard_normal(C)
            e0 = -double_well_log_prob(x, beta) + 0.5 * p * p
            q = x.copy()
            p = p - 0.5 * DW_DT * double_well_gradient(q, beta)
            for _ in range(DW_STEPS - 1):
                q = q + p * DW_DT
                p = p - DW_DT * double_well_gradient(q, beta)
            q = q + p * DW_DT
            p = p - 0.5 * DW_DT * double_well_gradient(q, beta)
            e1 = -double_well_log_prob(q, beta) + 0.5 * p * p
            acc = rs.random_sample(C) < accept_probability(-(e1 - e0))
            x = np.where(acc, q, x)
        if swaps:
            parity = rnd & 1
            xp = x[partner(C, R, parity)]
            out, _ = swap_round(x[:, None], double_well_log_prob(x, beta), double_well_log_prob(xp, beta),
                                rs.random_sample(C), R, parity)
            x = out[:, 0]
    return float(np.mean(x[0::R] < 0.0))
