"""Replica exchange on the device (``csrc/replica.hip``, ``binf_amd/samplers/replica.py``)
against the host restatement ``tests/replica_exchange.py``: the two kernels bit for bit
through the C ABI, refusals, guard zones, shard == whole, the sampler against a loop written
here, checkpoint / resume, stationarity with a derived tolerance, and the double-well run
that only mixes with the swaps."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import replica_exchange as RX
import stationarity as ST
from binf_amd import _native, checkpoint
from binf_amd.example.likelihood import POLYVAL
from binf_amd.example.misc import make_posterior
from binf_amd.pdf import IsotropicGaussian
from binf_amd.samplers.hmc import HMCSampler
from binf_amd.samplers.replica import ReplicaExchangeSampler, geometric_betas, ladder_precision
from binf_amd.samplers.rng import DeviceRNG
from conftest import ROOT

pytestmark = pytest.mark.gpu

SENT = -7.25                       # sentinel of the double buffers
SENT_I = -99


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def ptr(t):
    return None if t is None else t.data_ptr()


def carve(a, device, before=0, after=0, fill=None):
    """``a`` on the device inside a larger sentinel-filled buffer: (view, whole buffer).
    ``before`` elements in front shift a double view off 16-byte alignment when odd."""
    flat = np.ascontiguousarray(a).reshape(-1)
    if fill is None:
        fill = SENT if flat.dtype == np.float64 else SENT_I
    whole = torch.full((before + flat.size + after,), fill, dtype=torch.from_numpy(flat[:0]).dtype,
                       device=device)
    view = whole[before:before + flat.size]
    view.copy_(torch.from_numpy(flat))
    return view, whole


def guards_intact(whole, before, n):
    w = whole.cpu().numpy()
    fill = SENT if w.dtype == np.float64 else (SENT_I if w.dtype != np.uint8 else SENT_I % 256)
    return bool(np.all(w[:before] == fill) and np.all(w[before + n:] == fill))


def call_gather(L, x, out, C, D, R, parity, device):
    return L.binf_replica_gather_f64(ptr(x), ptr(out), C, D, R, parity, _native.stream_handle(device))


def call_swap(L, x, lp_own, lp_sw, u, out, acc, natt, nacc, walker, C, D, R, parity, device,
              seed=0, offset=0, chain_offset=0):
    return L.binf_replica_swap_f64(ptr(x), ptr(lp_own), ptr(lp_sw), ptr(u), ptr(out), ptr(acc), ptr(natt),
                                   ptr(nacc), ptr(walker), C, D, R, parity, seed, offset, chain_offset,
                                   _native.stream_handle(device))


def run_swap(L, device, x, lp_own, lp_sw, u, R, parity, shift_x=0, shift_out=0, gen=None,
             att0=None, acc0=None, walker0=None, guard=0):
    """One swap through the C ABI with every output carved out of a sentinel buffer; returns
    numpy (out, accepted, n_attempted, n_accepted, walker) after checking the guard zones."""
    C, D = x.shape
    xd, _ = carve(x, device, before=shift_x, after=3)
    outd, out_w = carve(np.full((C, D), SENT), device, before=shift_out + 2 * guard, after=guard + 3)
    accd, acc_w = carve(np.full(C, SENT_I % 256, dtype=np.uint8), device, before=guard, after=guard, fill=SENT_I % 256)
    att0 = np.zeros(C, dtype=np.int64) if att0 is None else att0
    acc0 = np.zeros(C, dtype=np.int64) if acc0 is None else acc0
    walker0 = np.arange(C, dtype=np.int64) if walker0 is None else walker0
    attd, att_w = carve(att0, device, before=guard, after=guard)
    nacd, nac_w = carve(acc0, device, before=guard, after=guard)
    wald, wal_w = carve(walker0, device, before=guard, after=guard)
    ud = None if u is None else dev(u, device)
    seed, offset, coff = gen if gen is not None else (0, 0, 0)
    rc = call_swap(L, xd if D else None, dev(lp_own, device), dev(lp_sw, device), ud, outd if D else None,
                   accd, attd, nacd, wald, C, D, R, parity, device, seed, offset, coff)
    assert rc == 0, _native.last_error()
    assert guards_intact(out_w, shift_out + 2 * guard, C * D) and guards_intact(acc_w, guard, C)
    assert guards_intact(att_w, guard, C) and guards_intact(nac_w, guard, C) and guards_intact(wal_w, guard, C)
    return (outd.cpu().numpy().reshape(C, D), accd.cpu().numpy(), attd.cpu().numpy(), nacd.cpu().numpy(),
            wald.cpu().numpy())


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def expect_swap(x, lp_own, lp_sw, u, R, parity, att0, acc0, walker0):
    att, acc, walker = att0.copy(), acc0.copy(), walker0.copy()
    out, flags = RX.swap_round(x, lp_own, lp_sw, u, R, parity, (att, acc), walker)
    return out, flags, att, acc, walker


def check_swap(got, want, what):
    for g, w, name in zip(got, want, ('out', 'accepted', 'n_attempted', 'n_accepted', 'walker')):
        assert same_bits(np.ascontiguousarray(g), np.ascontiguousarray(w)), (what, name)


# ---------------------------------------------------------------------------
# the kernels, bit for bit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('D', RX.CASE_D)
def test_gather_and_swap_bits_against_the_restatement(device, D):
    """R in 1..5, both parities, 1 / 3 / 37 ladders; x and out 16-byte aligned, x at an
    8-byte-only aligned offset of a larger buffer, and both; supplied u == generated u ==
    the restated Philox stream; counters from non-zero values; walker ids permuted."""
    L = _native.lib()
    for R in RX.CASE_R:
        for n_ladders in RX.CASE_LADDERS:
            k = RX.case_inputs(R, n_ladders)
            C = k['C']
            x = RX.case_rows(C, D, salt=R + n_ladders)
            rs = np.random.RandomState(C)
            att0, acc0 = rs.randint(1, 50, size=C).astype(np.int64), rs.randint(1, 50, size=C).astype(np.int64)
            walker0 = rs.permutation(C).astype(np.int64) + 1000
            ug = RX.generated_uniforms(k['seed'], k['offset'], k['chain_offset'], C)
            for parity in (0, 1):
                for shift_x, shift_out in ((0, 0), (1, 0), (1, 1)):
                    what = (R, n_ladders, D, parity, shift_x, shift_out)
                    if D:
                        xd, _ = carve(x, device, before=shift_x, after=3)
                        outd, _ = carve(np.full((C, D), SENT), device, before=shift_out, after=3)
                        assert call_gather(L, xd, outd, C, D, R, parity, device) == 0
                        assert same_bits(outd.cpu().numpy().reshape(C, D), RX.gather(x, R, parity)), what
                    else:
                        assert call_gather(L, None, None, C, D, R, parity, device) == 0
                    want = expect_swap(x, k['lp_own'], k['lp_sw'], k['u'], R, parity, att0, acc0, walker0)
                    got = run_swap(L, device, x, k['lp_own'], k['lp_sw'], k['u'], R, parity, shift_x, shift_out,
                                   att0=att0, acc0=acc0, walker0=walker0)
                    check_swap(got, want, what + ('supplied',))
                    want = expect_swap(x, k['lp_own'], k['lp_sw'], ug, R, parity, att0, acc0, walker0)
                    gen = (k['seed'], k['offset'], k['chain_offset'])
                    got = run_swap(L, device, x, k['lp_own'], k['lp_sw'], None, R, parity, shift_x, shift_out,
                                   gen=gen, att0=att0, acc0=acc0, walker0=walker0)
                    check_swap(got, want, what + ('generated',))
                    if (shift_x, shift_out) == (0, 0):
                        got2 = run_swap(L, device, x, k['lp_own'], k['lp_sw'], ug, R, parity,
                                        att0=att0, acc0=acc0, walker0=walker0)
                        check_swap(got2, got, what + ('supplied == generated',))


def test_generated_uniforms_are_the_device_uniform_stream(device):
    """u == NULL reads element chain_offset + i of the stream DeviceRNG.uniform(C) writes."""
    k = RX.case_inputs(4, 37)
    rng = DeviceRNG(k['seed'], device, chain_offset=k['chain_offset'])
    rng.offset = k['offset']
    want = RX.generated_uniforms(k['seed'], k['offset'], k['chain_offset'], k['C'])
    assert same_bits(rng.uniform(k['C'], device).cpu().numpy(), want)


def test_forced_decisions_and_edge_inputs(device):
    L = _native.lib()
    R, n_ladders, D = 4, 37, 7
    k = RX.case_inputs(R, n_ladders)
    C = k['C']
    x = RX.case_rows(C, D)
    for parity in (0, 1):
        low = RX.lower_members(C, R, parity)
        # u = 0 accepts every finite delta, u = +inf rejects all
        out, acc, att, nacc, _ = run_swap(L, device, x, k['lp_own'], k['lp_sw'], np.zeros(C), R, parity)
        pair = low | np.roll(low, 1)
        assert np.array_equal(acc.astype(bool), pair) and same_bits(out, RX.gather(x, R, parity))
        assert np.array_equal(att, low.astype(np.int64)) and np.array_equal(nacc, low.astype(np.int64))
        out, acc, att, nacc, walker = run_swap(L, device, x, k['lp_own'], k['lp_sw'], np.full(C, np.inf), R, parity)
        assert not acc.any() and same_bits(out, x) and not nacc.any() and np.array_equal(walker, np.arange(C))
        assert np.array_equal(att, low.astype(np.int64))
        zero = np.zeros(C, dtype=np.int64)
        ids = np.arange(C, dtype=np.int64)
        # delta = 0 exactly: accepted by u < 1, rejected by u = 1
        for uval in (0.999, 1.0, 0.0):
            u = np.full(C, uval)
            got = run_swap(L, device, x, k['lp_own'], k['lp_own'], u, R, parity)
            check_swap(got, expect_swap(x, k['lp_own'], k['lp_own'], u, R, parity, zero, zero, ids), ('delta 0', uval))
            assert bool(got[1][low].all()) == (uval < 1.0)
        # delta beyond both clip bounds (+-1000 per chain: +-2000 per pair)
        for shift in (1000.0, -1000.0):
            for uval in (0.5, 0.0, 1e-300):
                u = np.full(C, uval)
                lp_sw = k['lp_own'] + shift
                got = run_swap(L, device, x, k['lp_own'], lp_sw, u, R, parity)
                check_swap(got, expect_swap(x, k['lp_own'], lp_sw, u, R, parity, zero, zero, ids), ('clip', shift, uval))
        # NaN / +inf / -inf in the log-probs of ONE chain: as the restatement says (NaN rejects),
        # and every other pair keeps its bits
        base = expect_swap(x, k['lp_own'], k['lp_sw'], k['u'], R, parity, zero, zero, ids)
        for bad in (np.nan, np.inf, -np.inf):
            for which in ('own', 'sw', 'both'):
                for c in (int(np.nonzero(low)[0][3]), int(np.nonzero(low)[0][5]) + 1):
                    lp_own, lp_sw = k['lp_own'].copy(), k['lp_sw'].copy()
                    if which in ('own', 'both'):
                        lp_own[c] = bad
                    if which in ('sw', 'both'):
                        lp_sw[c] = bad
                    want = expect_swap(x, lp_own, lp_sw, k['u'], R, parity, zero, zero, ids)
                    got = run_swap(L, device, x, lp_own, lp_sw, k['u'], R, parity)
                    check_swap(got, want, (bad, which, c))
                    i = c if low[c] else c - 1
                    others = np.ones(C, dtype=bool)
                    others[[i, i + 1]] = False
                    assert same_bits(got[0][others], base[0][others]) and np.array_equal(got[1][others], base[1][others])
                    if np.isnan(bad) or which == 'both':
                        assert got[1][i] == 0 and got[1][i + 1] == 0          # NaN rejects


def test_refusals_leave_the_outputs_untouched(device):
    L = _native.lib()
    R, n_ladders, D = 3, 4, 5
    C = R * n_ladders
    x = dev(RX.case_rows(C, D), device)
    lp = dev(np.zeros(C), device)
    u = dev(np.full(C, 0.0), device)                                 # would accept everything
    out = torch.full((C, D), SENT, dtype=torch.float64, device=device)
    acc = torch.full((C,), 77, dtype=torch.uint8, device=device)
    att = torch.full((C,), SENT_I, dtype=torch.int64, device=device)
    nac = torch.full((C,), SENT_I, dtype=torch.int64, device=device)
    wal = torch.full((C,), SENT_I, dtype=torch.int64, device=device)
    xbig = torch.zeros(3 * C * D, dtype=torch.float64, device=device)

    def swap(x_=x, lp_own=lp, lp_sw=lp, out_=out, acc_=acc, C_=C, D_=D, R_=R, parity=0, coff=0):
        return call_swap(L, x_, lp_own, lp_sw, u, out_, acc_, att, nac, wal, C_, D_, R_, parity, device, 1, 2, coff)

    def gather(x_=x, out_=out, C_=C, D_=D, R_=R, parity=0):
        return call_gather(L, x_, out_, C_, D_, R_, parity, device)

    E_ARG, E_ALIAS = _native.E_ARG, _native.E_ALIAS
    for fn in (swap, gather):
        assert fn(C_=-3) == E_ARG and fn(D_=-1) == E_ARG
        assert fn(R_=0) == E_ARG and fn(R_=-1) == E_ARG
        assert fn(R_=5) == E_ARG                                     # C % R != 0
        assert fn(parity=2) == E_ARG and fn(parity=-1) == E_ARG
        assert fn(x_=None) == E_ARG and fn(out_=None) == E_ARG
        assert fn(C_=0, R_=0) == E_ARG                               # argument errors come before C == 0
        # any overlap of out with x
        assert fn(x_=xbig[:C * D], out_=xbig[:C * D]) == E_ALIAS
        assert fn(x_=xbig[:C * D], out_=xbig[1:C * D + 1]) == E_ALIAS
        assert fn(x_=xbig[C * D - 1:2 * C * D - 1], out_=xbig[:C * D]) == E_ALIAS
        assert fn(C_=0) == 0                                         # no launch, not an error
    assert swap(coff=-3) == E_ARG and swap(coff=1) == E_ARG and swap(coff=4) == E_ARG
    assert swap(lp_own=None) == E_ARG and swap(lp_sw=None) == E_ARG and swap(acc_=None) == E_ARG
    assert 'replica_swap' in _native.last_error()
    with pytest.raises(ValueError):
        _native.replica_gather(x, 5, 0)
    with pytest.raises(ValueError):
        _native.replica_swap(x, lp, lp, R, 0, acc, u=u, out=x)
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((acc == 77).all())
    for t in (att, nac, wal):
        assert bool((t == SENT_I).all())
    # adjacent buffers are no overlap
    assert swap(x_=xbig[:C * D], out_=xbig[C * D:2 * C * D]) == 0
    assert gather(x_=xbig[:C * D], out_=xbig[C * D:2 * C * D]) == 0


@pytest.mark.parametrize('D', [1, 33, 257])
def test_guard_zones(device, D):
    """out, accepted, the counters and walker carved out of larger sentinel-filled buffers
    (out at an odd offset as well): nothing outside changes."""
    L = _native.lib()
    R, n_ladders = 3, 37
    k = RX.case_inputs(R, n_ladders)
    C = k['C']
    x = RX.case_rows(C, D)
    zero, ids = np.zeros(C, dtype=np.int64), np.arange(C, dtype=np.int64)
    for parity in (0, 1):
        for shift_out in (0, 1):
            got = run_swap(L, device, x, k['lp_own'], k['lp_sw'], k['u'], R, parity, shift_out=shift_out, guard=64)
            check_swap(got, expect_swap(x, k['lp_own'], k['lp_sw'], k['u'], R, parity, zero, zero, ids), (D, parity))
            outd, out_w = carve(np.full((C, D), SENT), device, before=64 + shift_out, after=64)
            assert call_gather(L, dev(x, device), outd, C, D, R, parity, device) == 0
            assert guards_intact(out_w, 64 + shift_out, C * D)
            assert same_bits(outd.cpu().numpy().reshape(C, D), RX.gather(x, R, parity))


def test_a_shard_of_ladders_equals_the_whole(device):
    """8 ladders x R = 3 whole, and as blocks of 3 + 5 ladders with chain_offset: row for
    row, with generated uniforms."""
    L = _native.lib()
    R, D = 3, 33
    C = 8 * R
    rs = np.random.RandomState(21)
    x = rs.standard_normal((C, D))
    lp_own, lp_sw = rs.standard_normal(C) - 20.0, rs.standard_normal(C) - 20.0
    seed, offset = RX.PHILOX_SEED, 12
    ug = RX.generated_uniforms(seed, offset, 0, C)
    zero, ids = np.zeros(C, dtype=np.int64), np.arange(C, dtype=np.int64)
    for parity in (0, 1):
        assert RX.decisive(lp_own, lp_sw, ug, R, parity)
        whole = run_swap(L, device, x, lp_own, lp_sw, None, R, parity, gen=(seed, offset, 0), walker0=ids)
        check_swap(whole, expect_swap(x, lp_own, lp_sw, ug, R, parity, zero, zero, ids), parity)
        assert 0 < whole[1].sum() < 2 * RX.lower_members(C, R, parity).sum()
        for a, b in ((0, 3 * R), (3 * R, C)):
            part = run_swap(L, device, x[a:b], lp_own[a:b], lp_sw[a:b], None, R, parity, gen=(seed, offset, a),
                            walker0=ids[a:b])
            check_swap(part, [w[a:b] for w in whole], (parity, a, b))


# ---------------------------------------------------------------------------
# the sampler
# ---------------------------------------------------------------------------
R_S, LADDERS_S, ROUNDS = 3, 4, 6


def build_inner(kind, device, rng=None, adapt=4):
    C = R_S * LADDERS_S
    rs = np.random.RandomState(31)
    if kind == 'gauss':
        D = 8
        pdf, name = IsotropicGaussian(1.7, 0.2), 'x'
        q0, dt, nsteps = rs.standard_normal((C, D)), 0.25, 4
    else:
        D = 4
        xs = np.linspace(-2, 2, 20)
        ys = POLYVAL(xs, np.array([2.0, -4.0, 1.0, 1.5])) + 0.6 * rs.standard_normal(20)
        tau = ladder_precision(geometric_betas(R_S, 0.2), 2.0, LADDERS_S, device)
        pdf, name = make_posterior(xs, ys, POLYVAL).conditional_factory(precision=tau), 'coefficients'
        q0, dt, nsteps = np.array([2.0, -4.0, 1.0, 1.5]) + 0.3 * rs.standard_normal((C, D)), 0.02, 5
    kw = {} if rng is None else {'rng': rng}
    s = HMCSampler(pdf, dev(q0, device), dt, nsteps, timestep_adaption_limit=adapt, variable_name=name, **kw)
    return s, name, C, D


def draws(C, D, n):
    rs = np.random.RandomState(32)
    return rs.standard_normal((n, C, D)), rs.uniform(size=(n, C)), rs.uniform(size=(n, C))


def restated_round(ref, name, u_swap, rnd, counters, device):
    """The swap of round ``rnd`` restated around the sampler ``ref``: the pdf's own log-probs
    of the state and of the gathered state, the numpy swap, the state handed back."""
    x = ref.state.cpu().numpy()
    parity = rnd & 1
    lp_own = ref.pdf.log_prob(**{name: ref.state}).cpu().numpy().reshape(-1)
    lp_sw = ref.pdf.log_prob(**{name: dev(RX.gather(x, R_S, parity), device)}).cpu().numpy().reshape(-1)
    assert RX.decisive(lp_own, lp_sw, u_swap, R_S, parity)
    out, flags = RX.swap_round(x, lp_own, lp_sw, u_swap, R_S, parity, counters)
    ref.state = dev(out, device)
    return out, flags


@pytest.mark.parametrize('kind', ['gauss', 'poly'])
def test_sampler_equals_a_loop_of_inner_samples_and_restated_swaps(device, kind):
    ref, name, C, D = build_inner(kind, device)
    p0, u_h, u_s = draws(C, D, ROUNDS)
    counters = (np.zeros(C, dtype=np.int64), np.zeros(C, dtype=np.int64))
    inner, _, _, _ = build_inner(kind, device)
    re = ReplicaExchangeSampler(inner, R_S)
    assert re.variable_name == name and re.n_ladders == LADDERS_S
    states, n_swapped = [], 0
    for i in range(ROUNDS):
        ref.sample(p0=dev(p0[i], device), u=dev(u_h[i], device))
        out, flags = restated_round(ref, name, u_s[i], i, counters, device)
        got = re.sample(u=dev(u_s[i], device), inner={'p0': dev(p0[i], device), 'u': dev(u_h[i], device)})
        assert got is inner.state and re.round == i + 1
        assert same_bits(got.cpu().numpy(), out), i
        assert np.array_equal(re.last_swap_accepted.cpu().numpy(), flags.astype(bool))
        assert np.array_equal(re.n_swap_attempted.cpu().numpy(), counters[0])
        assert np.array_equal(re.n_swap_accepted.cpu().numpy(), counters[1])
        # step sizes and acceptance counters of the inner sampler stay with the slot
        assert torch.equal(inner.timestep, ref.timestep) and torch.equal(inner.n_accepted, ref.n_accepted)
        states.append(out)
        n_swapped += int(flags.sum())
    assert n_swapped > 0 and counters[0].sum() == LADDERS_S * ROUNDS
    rate = re.swap_acceptance_rate.cpu().numpy()
    att = counters[0].reshape(LADDERS_S, R_S).sum(0)[:R_S - 1]
    assert np.array_equal(rate, counters[1].reshape(LADDERS_S, R_S).sum(0)[:R_S - 1] / att)
    assert same_bits(re.slot(re.state, 0).cpu().numpy(), states[-1][0::R_S])
    # sample_n(6, thin=2) == 6 x sample()
    inner2, _, _, _ = build_inner(kind, device)
    re2 = ReplicaExchangeSampler(inner2, R_S)
    rec = re2.sample_n(ROUNDS, thin=2, u=dev(u_s, device), inner={'p0': dev(p0, device), 'u': dev(u_h, device)})
    assert rec.shape == (ROUNDS // 2, C, D)
    for j in range(ROUNDS // 2):
        assert same_bits(rec[j].cpu().numpy(), states[2 * j + 1]), j
    assert np.array_equal(re2.n_swap_accepted.cpu().numpy(), counters[1]) and re2.round == ROUNDS
    assert re2.slot(rec, 1).shape == (ROUNDS // 2, LADDERS_S, D)


@pytest.mark.parametrize('kind', ['gauss', 'poly'])
def test_swap_interval_through_the_inner_sample_n(device, kind):
    ref, name, C, D = build_inner(kind, device)
    p0, u_h, u_s = draws(C, D, ROUNDS)
    counters = (np.zeros(C, dtype=np.int64), np.zeros(C, dtype=np.int64))
    inner, _, _, _ = build_inner(kind, device)
    re = ReplicaExchangeSampler(inner, R_S, swap_interval=3)
    for rnd in range(2):
        sl = slice(3 * rnd, 3 * rnd + 3)
        for i in range(sl.start, sl.stop):
            ref.sample(p0=dev(p0[i], device), u=dev(u_h[i], device))
        out, flags = restated_round(ref, name, u_s[rnd], rnd, counters, device)
        got = re.sample(u=dev(u_s[rnd], device), inner={'p0': dev(p0[sl], device), 'u': dev(u_h[sl], device)})
        assert same_bits(got.cpu().numpy(), out), rnd
        assert np.array_equal(re.last_swap_accepted.cpu().numpy(), flags.astype(bool))
        assert torch.equal(inner.timestep, ref.timestep) and torch.equal(inner.n_accepted, ref.n_accepted)
    assert inner.counter == 6 and re.round == 2
    assert np.array_equal(re.n_swap_accepted.cpu().numpy(), counters[1])


def test_checkpoint_resumes_bit_for_bit(device, tmp_path):
    def build():
        inner, _, _, _ = build_inner('poly', device, rng=DeviceRNG(9, device), adapt=7)
        return ReplicaExchangeSampler(inner, R_S, track_walkers=True)

    a = build()
    for _ in range(8):
        a.sample()
    b = build()
    for _ in range(4):
        b.sample()
    path = str(tmp_path / 're.pt')
    checkpoint.save(path, replica=b)
    c = build()
    checkpoint.load(path, replica=c)
    assert c.round == 4 and c.rng.offset == b.rng.offset
    for _ in range(4):
        c.sample()
    assert torch.equal(a.state, c.state) and a.round == c.round == 8
    assert torch.equal(a.n_swap_attempted, c.n_swap_attempted) and torch.equal(a.n_swap_accepted, c.n_swap_accepted)
    assert torch.equal(a.last_swap_accepted, c.last_swap_accepted) and torch.equal(a.walker, c.walker)
    assert torch.equal(a.sampler.n_accepted, c.sampler.n_accepted) and torch.equal(a.sampler.timestep, c.sampler.timestep)
    assert int(a.n_swap_accepted.sum()) > 0 and not torch.equal(a.walker, torch.arange(a.walker.numel(), device=device))
    assert sorted(a.walker.cpu().tolist()) == list(range(a.walker.numel()))          # a permutation
    assert torch.equal(a.walker // R_S, torch.arange(a.walker.numel(), device=device) // R_S)   # inside its ladder


class Harmonic(object):
    """A torch PDF: log p_c(x) = -1/2 k_c sum x^2."""

    def __init__(self, k):
        self.k = k

    def log_prob(self, x):
        return -0.5 * self.k * (x * x).sum(dim=1)

    def gradient(self, x):
        return self.k[:, None] * x


def test_stationarity_with_a_derived_tolerance(device):
    """Started exactly in equilibrium (x = z / sqrt(k_r)), 40 rounds of HMC + swaps must leave
    every slot in ITS distribution: the sample variance over the 512 ladders x 8 = 4096
    independent N(0, 1/k_r) entries of a slot has relative standard deviation sqrt(2/4096);
    5 of them = 11 %."""
    R, n_ladders, D = 4, 512, 8
    C = R * n_ladders
    k = torch.tensor([1.0, 0.5, 0.25, 0.125], dtype=torch.float64, device=device).repeat(n_ladders)
    rng = DeviceRNG(2024, device)
    x0 = rng.normal((C, D), device) / k.sqrt()[:, None]
    inner = HMCSampler(Harmonic(k), x0, 0.3 / k.sqrt(), 8, variable_name='x', rng=rng)
    re = ReplicaExchangeSampler(inner, R)
    for _ in range(40):
        x = re.sample()
    tol = 5.0 * np.sqrt(2.0 / (n_ladders * D))
    assert abs(tol - 0.11) < 1e-3
    for r in range(R):
        var = float(re.slot(x, r).reshape(-1).var())
        want = 1.0 / float(k[r])
        print('slot %d: variance %.4f, expected %.4f (%+.1f %%)' % (r, var, want, 100 * (var / want - 1)))
        assert abs(var / want - 1.0) <= tol, r
        # the same entries pooled, at the exact chi^2 quantiles (level 1e-9 over the four slots)
        pooled = ST.pooled_chi2(re.slot(x, r).cpu().numpy() * np.sqrt(float(k[r])), ST.ALPHA / R, 'slot %d' % r)
        print(ST.describe(pooled))
        assert ST.inside(pooled), r
    att = re.n_swap_attempted.view(n_ladders, R).sum(0).cpu().numpy()
    acc = re.n_swap_accepted.view(n_ladders, R).sum(0).cpu().numpy()
    assert np.array_equal(att, [20 * n_ladders] * (R - 1) + [0]) and np.all(acc[:R - 1] > 0) and acc[R - 1] == 0
    assert float(inner.acceptance_rate.mean()) > 0.5


def _example():
    spec = importlib.util.spec_from_file_location('example_replica_exchange',
                                                  os.path.join(ROOT, 'examples', 'replica_exchange.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_double_well_mixes_with_swaps_only(device):
    """512 ladders x 6 slots of the double well (a = 16), every chain started at x = +1: after
    150 rounds of 2 transitions the cold slot's fraction at x < 0 is within 5 sigma = 0.11 of
    0.5 (sigma = 0.5 / sqrt(512)); the same 300 transitions without swaps leave it below 0.02."""
    pdf_cls = _example().TemperedDoubleWell
    R = len(RX.DW_BETAS)
    C = RX.DW_LADDERS * R
    beta = torch.tensor(RX.DW_BETAS, dtype=torch.float64, device=device).repeat(RX.DW_LADDERS)

    def build(seed):
        x0 = torch.ones((C, 1), dtype=torch.float64, device=device)
        return HMCSampler(pdf_cls(RX.DW_A, beta), x0, RX.DW_DT, RX.DW_STEPS, variable_name='x',
                          rng=DeviceRNG(seed, device))

    re = ReplicaExchangeSampler(build(5), R, swap_interval=RX.DW_TRANSITIONS)
    for _ in range(RX.DW_ROUNDS):
        x = re.sample()
    f = float((re.slot(x, 0) < 0).double().mean())
    plain = build(5)
    for _ in range(RX.DW_ROUNDS * RX.DW_TRANSITIONS):
        y = plain.sample()
    stuck = float((y[0::R] < 0).double().mean())
    print('cold slot at x < 0: %.4f with swaps, %.4f without; swap rates %s'
          % (f, stuck, re.swap_acceptance_rate.cpu().numpy().round(3)))
    assert abs(f - 0.5) <= RX.DW_BOUND
    assert stuck < RX.DW_STUCK
