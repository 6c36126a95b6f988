// hmc_gauss_persist_kernel: the fused Gaussian HMC kernel template, shared by
// hmc_gauss.hip (draws read from HBM) and hmc_gauss_rng.hip (draws generated in
// the kernel).  See hmc_gauss.hip for the mapping and the reference lines.
#pragma once
#include "gauss_common.hpp"
#include "xoshiro.hpp"

namespace binf {

// RNG = 0: the momentum / uniform draws are read from HBM (a.p0, a.u);
// RNG = 1: they are generated in the kernel (xoshiro.hpp), nothing is read;
// RNG = 2: the same draws are only WRITTEN OUT (a.p_dump, a.u_dump) and no
//          trajectory is integrated -- what makes the fused generator testable:
//          sample_n with RNG = 1 must equal sample_n fed with this dump, bit for bit.
enum { GAUSS_RNG_HBM = 0, GAUSS_RNG_FUSED = 1, GAUSS_RNG_DUMP = 2 };

// LW = log2(waves per chain).  LW = 0: a chain is G = 8 << H <= 64 lanes of one
// wave (several chains per wave when G < 64).  LW > 0 (D > 1024): a chain spans
// 2 / 4 / 8 whole waves of the workgroup; the leaf-tree levels above a wave are
// joined through LDS (chain_sum_finish).
// Waves per workgroup: 4 (8 for chains of 8 waves).  With the generator in the
// kernel: 8, so that two workgroups per CU share the 160 KiB of LDS as 2 x (64 KiB
// stash + the 8 KiB layer table) -- still 16 waves per CU, the whole C2 batch resident.
constexpr int gauss_wpb(int LW, int RNG) { return (LW == 3 || RNG != GAUSS_RNG_HBM) ? 8 : 4; }

// Full leapfrog steps per taken back-edge of the step loop.  The bare loop is 4 x GS FP64
// instructions closed by a taken branch: the same arithmetic without memory issues at 0.88
// of the pipe's rate at 4 waves per SIMD, 0.91 unrolled by 4, 0.95 as 19 steps in straight
// line (scripts/fp64bench.hip, profiles/r08_u_fp64bench_unroll.json).  The waves of a SIMD do
// not reach the branch together: at equal priority the oldest runs nearly alone and a
// back-edge costs most in a wave that runs with few others left to cover it (0.65 of the
// rate at one wave per SIMD), which is what the priority rule below shortens.  In the kernel 4 measured best (16 and 19 give half of
// its gain: HISTORY 35).  Regular one-wave chains of the unit Gaussian only; 1 where the
// unrolled form costs a wave per SIMD (the non-unit kernels: 127 -> 132 VGPRs at TMAX 16;
// TMAX 12 EXACT: 80 -> 82; TMAX 4 with the generator: 79 -> 81).  These exceptions rest on
// register counts one or two short of an occupancy step under the compiler of the day:
// profiles/r16_s_gauss_resources.txt (first: r08_u_) is the table of every instantiation to regenerate
// (-Rpass-analysis=kernel-resource-usage) when the compiler or this loop changes.
constexpr int GAUSS_STEP_UNROLL = 4;
constexpr int gauss_step_unroll(int TMAX, bool REGULAR, bool UNIT, bool FMA, int LW, int RNG)
{
    if (!REGULAR || LW != 0 || !UNIT) return 1;
    if ((TMAX == 12 && !FMA) || (TMAX == 4 && RNG == GAUSS_RNG_FUSED)) return 1;
    return GAUSS_STEP_UNROLL;
}

// Wave priority from the transitions a wave has left.  The waves that share a SIMD belong to
// different workgroups, and at equal priority VALU issue goes to the oldest wave first: left
// alone, the four finish at 0.32 / 0.53 / 0.77 / 1.0 of the launch and the youngest runs the
// last fifth with nothing to cover its back-edges, trees and waits (scripts/fp64bench.hip
// priority, profiles/r10_p_fp64bench_priority.json).  So the priority falls as the wave's own
// count of transitions left does: min(3, (n - 1 - s) / GAUSS_PRIO_WINDOW), i.e. 3 until three
// windows before the end, then 2, 1 and, over the last window, 0.  A wave that is ahead crosses
// a threshold first and from there yields to every wave behind it until that one has crossed
// it too, so at each threshold the waves of a SIMD are level to within a window, whatever
// their order of arrival, and they finish together.  It needs no word between waves and no
// slot number, and it is monotone over the launch: there is no wrap across which a leader
// could take the top priority again and run ahead.  (The rotation (slot + s / R) & 3 has one:
// it levels half as well and gains half as much, HISTORY 39.)  Priority changes no value.
// The launch ends at 0, the priority every other kernel runs at, and 0 is restored before the
// final stores; until the last three windows, though, a wave of another kernel on the same
// SIMD is outranked and gets the issue slots this kernel leaves.  Window 4 measured best
// (2, 4, 8 tried).  One chain per wave with draws from
// HBM only (HC = 3): the waves of a longer chain meet at __syncthreads every transition and
// must not be ranked against each other.
constexpr int GAUSS_PRIO_WINDOW = 4;
constexpr bool gauss_wave_priority(int LW, int RNG, int HC)
{
    return LW == 0 && RNG == GAUSS_RNG_HBM && HC == 3;
}

// s_setprio takes an immediate and ignores EXEC: a scalar switch on a wave-uniform value
__device__ __forceinline__ void gauss_set_priority(int prio)
{
    switch (prio & 3) {
    case 0: __builtin_amdgcn_s_setprio(0); break;
    case 1: __builtin_amdgcn_s_setprio(1); break;
    case 2: __builtin_amdgcn_s_setprio(2); break;
    default: __builtin_amdgcn_s_setprio(3); break;
    }
}

// The rare path of a FASTSUM kernel: the accept decision of one transition from numpy's sums.
// The trajectory is a function of the start state and the drawn momentum alone, so running it
// again yields the end state the lane already holds in q: this runs it on copies, one group
// of GS elements at a time -- the start state from where a rejection restores it (`qs_lds`, the
// LDS stash, or else `qs`, the record read back), the momentum read again from `pc` with
// plain loads -- sums all four energies in numpy's order as the first transition of a launch
// does, and decides by metropolis_accept.  It writes nothing and leaves q, the prefetched
// momentum and the fused sums as they are; the caller drains its loads (s_waitcnt 0).
// GAUSS_REDO_GS elements at a time: its copies are live beside all of q and the prefetched
// group, and at 8 they cost the TMAX = 16 kernels the fourth wave per SIMD (112 -> 154 VGPRs;
// 4: 122, 2: 114).  The order of the additions inside a lane's accumulator does not depend on it.
// WIDE (below): the lanes of the calling kernel own other elements than numpy's accumulators
// do, so this path keeps numpy's ownership for its own reads -- `qs` and `pc` are the lane's
// bases in numpy's layout, and the stash, which a WIDE kernel keeps in element order (slot
// 2 (e / 128) + (e & 1) of lane (e % 128) / 2 is double number e of the wave's stash), is
// read at the lane's numpy elements 128 (lane / 8) + 8 t + lane % 8.  Bank conflicts there
// do not matter.
constexpr int GAUSS_REDO_GS = 2;
template <int TMAX, int GS, bool UNIT, bool FMA, bool WIDE = false>
__device__ inline bool gauss_exact_accept(const GaussNArgs &a, const double *qs, const double (*qs_lds)[64],
                                          int lane, const double *pc, double dt, double hdt, double c_lp,
                                          double u)
{
    LaneSum s0 = {0.0, 0.0}, spb = {0.0, 0.0}, sqa = {0.0, 0.0}, spa = {0.0, 0.0};
    const int e0 = 128 * (lane >> 3) + (lane & 7);                // WIDE: the lane's first numpy element
#pragma unroll 1
    for (int g = 0; g < TMAX / GS; ++g) {
        double qq[GS], pp[GS];
#pragma unroll
        for (int i = 0; i < GS; ++i) {
            const int t = g * GS + i;
            if (WIDE) qq[i] = qs_lds ? (&qs_lds[0][0])[e0 + 8 * t] : qs[8 * t];
            else qq[i] = qs_lds ? qs_lds[t][lane] : qs[8 * t];
            pp[i] = pc[8 * t];
        }
#pragma unroll
        for (int i = 0; i < GS; ++i) {
            const int t = g * GS + i;
            const double d = UNIT ? qq[i] : qq[i] - a.x0;
            lane_sum_add<true>(s0, d * d, t, TMAX);
            lane_sum_add<true>(spb, pp[i] * pp[i], t, TMAX);      // hmc.py:148
        }
#pragma unroll
        for (int i = 0; i < GS; ++i)                              // hmc.py:116
            pp[i] = kick<FMA>(pp[i], hdt, gauss_grad<UNIT>(qq[i], a.k, a.x0));
#pragma unroll 1
        for (int l = 0; l < a.nsteps - 1; ++l) {                  // hmc.py:118-120
#pragma unroll
            for (int i = 0; i < GS; ++i) {
                qq[i] = drift<FMA>(qq[i], pp[i], dt);
                pp[i] = kick<FMA>(pp[i], dt, gauss_grad<UNIT>(qq[i], a.k, a.x0));
            }
        }
#pragma unroll
        for (int i = 0; i < GS; ++i) {                            // hmc.py:122-123, 150
            const int t = g * GS + i;
            qq[i] = drift<FMA>(qq[i], pp[i], dt);
            pp[i] = kick<FMA>(pp[i], hdt, gauss_grad<UNIT>(qq[i], a.k, a.x0));
            const double d = UNIT ? qq[i] : qq[i] - a.x0;
            lane_sum_add<true>(sqa, d * d, t, TMAX);
            lane_sum_add<true>(spa, pp[i] * pp[i], t, TMAX);
        }
    }
    const double r = chain_sums_shared(sqa.r, spa.r, spb.r, s0.r, true);
    const double Eb = -(c_lp * lane_value_f64<12>(r)) + 0.5 * lane_value_f64<8>(r);
    const double Ea = -(c_lp * lane_value_f64<0>(r)) + 0.5 * lane_value_f64<4>(r);
    return metropolis_accept<true>(u, -(Ea - Eb));                // hmc.py:151
}

// UDT ("uniform dt"): every chain integrates with the kernel argument `timestep` and no
// adaption runs in the launch (the host picks it: gauss_uniform_dt).  The step size then
// lives in a scalar register pair instead of a vector pair per lane; same arithmetic, same
// bits, ~3 % shorter launches at the C2 shape (profiles/r04_u_ab.txt).
// HC >= 0: the tree height of a regular one-wave chain, fixed at compile time (the host
// dispatches it, hmc_gauss.hip): the energy trees are unrolled straight-line code
// (chain_sum_finish_fixed), the one of the drawn momentum finishes inside the last
// group's trajectory and the two end-of-trajectory trees go up together.  HC = -1:
// the height is the runtime a.H.
// HC = 3 (one chain per wave: D = 768, 1024): the three sums of a transition go up ONE
// shared tree on the tail (chain_sums_shared) and the finished sums are wave-uniform
// scalars.  The acceptance draw stays a per-lane value on purpose: with a scalar accept
// flag the rejection restore becomes a real branch, and the register allocator then
// copies all of q on the accepted path to meet the registers the restore loads into
// (16 v_mov_b64 per transition; in FMA mode 27 more VGPRs and the fourth wave).
//
// FASTSUM (the HC = 3 kernels with draws from HBM, launched when no energy is recorded:
// hmc_gauss.hip): the energies feed one bit, u < exp(-(Ea - Eb)), and that bit needs numpy's
// rounding of the three sums only when u lies within rounding distance of the threshold.  The
// running sums are acc = fma(x, x, acc), one instruction per element where lane_sum_add makes
// two (48 of a lane's 1488 per transition at TMAX = 16, 1455 with the decision's own); they go up the same shared tree, the
// carried sum of the current state is the fused one, and accept_decide (gauss_common.hpp)
// decides from them with a derived bound on their distance from numpy's.  A transition it
// cannot decide (order 1e-11 of them; every transition of a chain that holds an inf or a NaN)
// is decided by gauss_exact_accept below, from numpy's sums: states, flags and counts are
// bit for bit those of the kernel without FASTSUM.
// Not built where it costs a wave per SIMD: the unit kernels of TMAX = 12 (D = 768).  The exact
// decision's copies and sums are live beside the whole state on the tail.  At TMAX = 16 that is
// 2 or 3 VGPRs over the step loop's peak (C2: 112 -> 114) or under it (non-unit: 126 -> 124); at
// TMAX = 12 it is the peak, 84 / 88 -> 90 / 96 VGPRs and still 5 waves in the non-unit kernels,
// 79 .. 87 -> 106 .. 126 and 4 waves instead of 5 or 6 in the unit ones:
// profiles/r13_f_gauss_resources.txt, regenerated as r14_a_ with the table of gauss_step_unroll.
//
// ONESUM (a FASTSUM kernel of the unit Gaussian with the batch-wide step, UNIT && UDT; launched
// inside gauss_onesum_domain, hmc_gauss.hip): leapfrog on H = q^2 / 2 + p^2 / 2 conserves
// p^2 + (1 - dt^2 / 4) q^2, so dH = (dt^2 / 8) (sum q'^2 - sum q^2) and the end momentum feeds
// nothing.  The trajectory of a group ends with its last drift -- no final half kick (2
// instructions per element), no sum of p'^2 (1) -- and two sums climb the shared tree
// (chain_sums_shared2), three on the first transition.  The exponent is x~ = -(c_dh (Sqa~ -
// Sq_state~)), delta = f_dh (2 Eb~ + |x~|) with Eb~ from the carried sum and the drawn momentum's
// (which also sends an overflowing momentum to the exact decision); f_dh and the conditions
// are derived above gauss_onesum_factor (gauss_common.hpp).  The decision (accept_decide), the
// undecided path (gauss_exact_accept, which integrates its own final half kick in numpy's order)
// and the carried sum are FASTSUM's.  At TMAX = 16: 1455 -> 1389 VALU instructions per wave and
// transition (981 -> 924 in the listing), 114 -> 123 VGPRs in EXACT mode and 112 -> 113 in FMA
// mode, 4 waves per SIMD, no scratch, the counted waits unchanged (vmcnt(9) at the top,
// vmcnt(15..8) in the second group): profiles/r14_a_gauss_resources.txt, r14_a_pmc_persist.json.
//
// WIDE (an ONESUM kernel; launched in EXACT mode when q0, p0, the record and q_out are 16-byte
// aligned, hmc_gauss.hip): numpy's ownership -- lane (leaf g, accumulator j) holds 128 g + 8 t + j
// -- exists so that a lane's running sum is numpy's j-th accumulator, and every 8-byte access of
// a wave touches eight separate 64-byte half lines.  The steady path's sums are fused ones under
// a bound that counts roundings by depth alone, so their order is free: lane l owns 128 r + 2 l
// + b and every q0 / p0 load, record and q_out store, stash access and rejection restore is
// one 16-byte access per (lane, r), a wave instruction covering 1 KiB contiguous.  Only
// gauss_exact_accept still sums as numpy does, and it reads by numpy's ownership.  Measured:
// VMEM instructions per wave and transition 17.5 + 17.3 -> 9.3 + 9.1, VALU 1389 -> 1391, HBM bytes
// unchanged, 123 VGPRs, 4 waves per SIMD, no scratch; +1.3 % on the headline in two calls with
// disjoint ranges, nothing in FMA mode (which keeps numpy's ownership) and +0.5 % with
// overlapping ranges at thin = 64: profiles/r15_a_bench_headline.json, r15_a_pmc_persist.json.
//
// STREAM (a compile-time property of the WIDE kernel, gauss_stream_policy; no kernel argument,
// nothing read from the environment): the cache policy of its two HBM streams.  The launch's
// traffic shape alone -- two 4 KiB load groups and one 8 KiB store group per wave and transition,
// 4 waves per SIMD, 32 MiB between a wave's rows -- moves 5.05 TB/s at FMA-mode pacing and 5.26
// with no work at all, 0.80 and 0.84 of what a copy moves (scripts/streambench.hip,
// profiles/r16_s_streambench.json): the cap of the FMA-mode kernel is the shape's own.  The
// `nt` bit on its loads and stores together lifts it by 3 to 4 %; on either alone, and sc1 or
// sc0 sc1 on either or both, nothing; contiguous slabs of chains per XCD cost 2 %, wave skew up
// to 40 transitions and one 8 KiB load burst change nothing.  So the record stores and the
// momentum loads (p0; not q0, not q_out, which the next launch reads) are non-temporal:
// __builtin_nontemporal_store / _load of the 16-byte vector, `global_*_dwordx4 ... nt` in the
// listing, which differs from the kernel's without them in that bit of 12 loads and 8 stores
// alone -- pins, sched_barriers and counted waits as they were, 123 VGPRs, 4 waves per SIMD,
// no scratch (profiles/r16_s_gauss_resources.txt).  A hint changes no value, but two reads
// depend on what a hinted store left: the rejection restore reads back what the same lane
// stored one transition earlier, and gauss_exact_accept reads that record through other lanes
// of the wave, both with plain loads.  An `nt` store keeps its line in the XCD's L2 like a
// plain one and a wave's memory instructions reach it in order, so both see the stored bytes
// (tests/test_gpu_gauss_stream.py: nearly every transition rejecting, a record buffer written
// by two launches).  Measured: +2.6 % on the headline, eight rounds, ranges apart by 1.6 %
// (stores alone +1.6 %, loads alone +1.1 %); VALU instructions and HBM bytes per launch
// unchanged; thin = 64 +0.4 %: profiles/r16_s_bench_headline.json, r16_s_pmc_persist.json.
// The microbenchmark's other gain, the stores spread behind the next transition's first loads
// (+2 to 3 %), would change the steady path's counted waits and is not taken here (HISTORY 45).
constexpr int GAUSS_STREAM_NT_RECORD = 1;            // record stores: global_store_dwordx4 ... nt
constexpr int GAUSS_STREAM_NT_P0 = 2;                // momentum loads: global_load_dwordx4 ... nt
constexpr int GAUSS_STREAM_WIDE = GAUSS_STREAM_NT_RECORD | GAUSS_STREAM_NT_P0;
constexpr int gauss_stream_policy(bool WIDE) { return WIDE ? GAUSS_STREAM_WIDE : 0; }

constexpr bool gauss_fastsum_built(int TMAX, int HC, bool UNIT) { return HC == 3 && (TMAX == 16 || !UNIT); }

// 16 bytes per lane: two neighbouring doubles as one global_load / global_store_dwordx4 or one
// ds_read / ds_write_b128.  The address must be 16-byte aligned.  NT: the non-temporal form
// (the `nt` bit of the instruction on gfx950), global memory only.
typedef double gauss_d2 __attribute__((ext_vector_type(2)));
template <bool NT = false>
__device__ __forceinline__ void gauss_ld2(double &x, double &y, const double *p)
{
    const gauss_d2 v = NT ? __builtin_nontemporal_load(reinterpret_cast<const gauss_d2 *>(p))
                          : *reinterpret_cast<const gauss_d2 *>(p);
    x = v.x;
    y = v.y;
}
template <bool NT = false>
__device__ __forceinline__ void gauss_st2(double *p, double x, double y)
{
    const gauss_d2 v = {x, y};
    if (NT) __builtin_nontemporal_store(v, reinterpret_cast<gauss_d2 *>(p));
    else *reinterpret_cast<gauss_d2 *>(p) = v;
}

template <int TMAX, bool REGULAR, bool UNIT, bool FMA, int LW, int RNG = GAUSS_RNG_HBM, bool UDT = false,
          int HC = -1, bool FASTSUM = false, bool ONESUM = false, bool WIDE = false>
__global__ void __launch_bounds__(64 * gauss_wpb(LW, RNG))
hmc_gauss_persist_kernel(const GaussNArgs a)
{
    static_assert(!WIDE || (ONESUM && TMAX == 16 && HC == 3 && REGULAR && LW == 0),
                  "16-byte ownership: the two-sum kernel of one 1024-element chain per wave");
    static_assert(HC < 0 || (REGULAR && LW == 0), "compile-time tree height: regular one-wave chains only");
    constexpr bool FIXED = HC >= 0;
    constexpr int HF = FIXED ? HC : 0;
    constexpr bool SHARED = HC == 3;
    static_assert(!FASTSUM || (SHARED && RNG == GAUSS_RNG_HBM), "fused sums: the shared-tree kernels, draws from HBM");
    static_assert(!ONESUM || (FASTSUM && UNIT && UDT), "two sums: the unit Gaussian, one step size for the batch");
    // the drawn momentum's tree inside the last group's trajectory: with UNIT it frees
    // registers (116 -> 109 VGPRs at TMAX = 16); without, it costs 2 and, on the per-lane-dt
    // variant, the fourth wave (127 -> 129), so there it stays on the tail, beside the other two.
    // Not with the shared tree, where it joins the other two sums for 10 instructions.
    constexpr bool EARLY = FIXED && UNIT && !SHARED;
    constexpr int WPB = gauss_wpb(LW, RNG);          // waves per workgroup
    constexpr int WPC = 1 << LW;                     // waves per chain
    __shared__ double xch[WPB];
    __shared__ double ubc[WPB];                      // the chain's acceptance draw, wave to wave
    constexpr int GS = (TMAX % 8 == 0) ? 8 : ((TMAX % 4 == 0) ? 4 : TMAX);   // measured: 8 beats 4 and 16
    constexpr int NG = TMAX / GS;
    constexpr int USTEP = gauss_step_unroll(TMAX, REGULAR, UNIT, FMA, LW, RNG);
    constexpr bool PRIO = gauss_wave_priority(LW, RNG, HC);
    constexpr bool NT_REC = (gauss_stream_policy(WIDE) & GAUSS_STREAM_NT_RECORD) != 0;
    constexpr bool NT_P0 = (gauss_stream_policy(WIDE) & GAUSS_STREAM_NT_P0) != 0;
    // WIDE: written and read 16 bytes per lane, a wave's part in element order (below)
    alignas(WIDE ? 16 : 8) __shared__ double stash[RNG == GAUSS_RNG_DUMP ? 1 : WPB][RNG == GAUSS_RNG_DUMP ? 1 : TMAX][64];
    __shared__ double zx[RNG == GAUSS_RNG_HBM ? 1 : XZIG_C + 1];
    if (RNG != GAUSS_RNG_HBM) {
        xzig_load_table(zx, threadIdx.x, WPB * 64);
        __syncthreads();
    }

    const int lane = threadIdx.x & 63;
    const int wib = threadIdx.x >> 6;
    const int64_t wave = (int64_t)blockIdx.x * WPB + wib;
    const int H = FIXED ? HC : a.H;
    const int lg = (LW > 0) ? 6 : 3 + H;             // log2(lanes of a chain in this wave)
    const int slot = lane & ((1 << lg) - 1);
    const int j = slot & 7;
    const int wchain = wib & (WPC - 1);              // wave index inside the chain
    const int grp = (LW > 0) ? ((wchain << 3) | (lane >> 3)) : (slot >> 3);
    const bool writer = (LW > 0) ? (wchain == 0 && lane == 0) : (slot == 0);

    int off, n, leafdepth, canonical;
    if (REGULAR) {
        n = 8 * TMAX;
        off = grp * n;
        leafdepth = H;
        canonical = 1;
    } else {
        const Leaf L = pairwise_leaf(a.D, H, grp);
        off = L.off;
        n = L.len;
        leafdepth = L.depth;
        canonical = L.canonical;
    }
    const int T = (n >= 8) ? (n >> 3) : 0;
    const int rem = (n >= 8) ? (n & 7) : n;

    const int64_t raw = (LW > 0) ? (int64_t)blockIdx.x * (WPB / WPC) + (wib >> LW)
                                 : (wave << (6 - lg)) + (lane >> lg);
    const bool cvalid = raw < a.C;
    const int64_t chain = cvalid ? raw : a.C - 1;
    const int64_t CD = a.C * (int64_t)a.D;
    // WIDE: lane l owns elements 128 r + 2 l + b, r = 0..7, b = 0..1, held in q[2 r + b] -- one
    // 16-byte access per (lane, r), and one wave instruction covers 1 KiB, eight whole 128-byte
    // lines, where numpy's ownership touches eight separate 64-byte halves with 8 bytes per
    // lane: 8 loads and 8 stores per lane and transition instead of 16 and 16.  Group g of the
    // momentum ring holds r = 4 g .. 4 g + 3.  The fused sums run over the lane's 16 slots in
    // slot order and climb the same tree: their bound counts roundings by depth alone
    // (gauss_common.hpp), whichever elements a lane holds.  numpy's order is kept where it is
    // needed, in gauss_exact_accept, which reads by numpy's ownership (base_np).
    const int64_t base_np = chain * (int64_t)a.D + off + j;
    // The lane's WIDE base points at its row r = WR0 in the middle of the chain: the eight rows
    // then lie at -4 .. +3 KiB, inside the signed 13-bit offset of a global instruction, and
    // no access needs an address of its own.
    constexpr int WR0 = TMAX / 4;
    const int64_t base = WIDE ? chain * (int64_t)a.D + 2 * lane + 128 * WR0 : base_np;

    double dt = (UDT || !a.dt_chain) ? a.timestep : a.dt_chain[chain];
    double uu = 0.0;
    if (RNG == GAUSS_RNG_HBM) uu = a.u[chain];
    // the lane's random stream: identified by (GLOBAL chain, leaf, accumulator),
    // i.e. by WHICH elements the lane owns, not by where it runs (nor by which
    // rank's shard the chain sits in: chain_offset); the redundant groups of a
    // ragged tree share the stream of the leaf they recompute
    // Transition s of a launch draws from stream position rng_offset + s, exactly what
    // a single-transition launch at that position draws: sample_n(n) and n sample()
    // calls see the same chains (as on the long-chain path, hmc_gauss_big.hip).
    Xo128 gen = {0u, 0u, 0u, 0u};
    uint64_t gen_stream = 0;
    if (RNG != GAUSS_RNG_HBM) {
        const int cgrp = grp & ~((1 << (H - leafdepth)) - 1);
        gen_stream = (uint64_t)(chain + a.chain_offset) * (uint64_t)(8 << H) + (uint64_t)(cgrp * 8 + j);
    }
    __builtin_amdgcn_sched_barrier(0);

    // q lives in registers for the whole launch; the momentum is needed one
    // element group at a time, so it streams through a 2-deep register ring
    // (pa / pb): while group g runs its trajectory, group g+1's draw (or group
    // 0 of the next transition) is in flight.
    double q[TMAX], pa[GS], pb[GS];
    // issue order = arrival order: the first group's state and momentum first,
    // so its trajectory can start while the rest of the state is in flight
    if constexpr (WIDE) {
#pragma unroll
        for (int r = 0; r < GS / 2; ++r) gauss_ld2(q[2 * r], q[2 * r + 1], a.q0 + base + 128 * (r - WR0));
#pragma unroll
        for (int r = 0; r < GS / 2; ++r) gauss_ld2<NT_P0>(pa[2 * r], pa[2 * r + 1], a.p0 + base + 128 * (r - WR0));
#pragma unroll
        for (int r = GS / 2; r < TMAX / 2; ++r) gauss_ld2(q[2 * r], q[2 * r + 1], a.q0 + base + 128 * (r - WR0));
    } else {
#pragma unroll
        for (int t = 0; t < GS; ++t) {
            const bool m = REGULAR || (8 * t + j < n);
            q[t] = (m && RNG != GAUSS_RNG_DUMP) ? a.q0[base + 8 * t] : 0.0;
        }
        if (RNG == GAUSS_RNG_HBM) {
#pragma unroll
            for (int i = 0; i < GS; ++i) {
                const bool m = REGULAR || (8 * i + j < n);
                pa[i] = m ? a.p0[base + 8 * i] : 0.0;
            }
        }
#pragma unroll
        for (int t = GS; t < TMAX; ++t) {
            const bool m = REGULAR || (8 * t + j < n);
            q[t] = (m && RNG != GAUSS_RNG_DUMP) ? a.q0[base + 8 * t] : 0.0;
        }
    }

    const double c_lp = SHARED ? a.c_lp : -0.5 * a.k;         // SHARED: a scalar operand
    // np.sum((q - x0)**2) of the CURRENT state, carried across transitions
    // (for the start state it is summed group by group inside the first
    // transition, so that the first trajectories need not wait for all of q0)
    LaneSum s0 = {0.0, 0.0};
    double Sq_state = 0.0;
    int64_t nacc = 0;

    // Where a rejected chain gets its old state back from.  When EVERY state is recorded
    // (thin == 1) the state before transition s is what this very lane wrote to the
    // record of transition s - 1 (q0 for s = 0): it is read back from there on the rare
    // rejection, and the per-transition copy of the state to LDS (16 ds_write_b64 per lane)
    // is not made at all; a single transition (n == 1) reads q0 again.  Regular trees only
    // (every lane owns what it reads back).
    const bool stash_lds = !(REGULAR && ((a.samples && a.thin == 1) || a.n == 1));
    // the record: every thin-th state goes to the next slot (a running count, no division
    // per transition); `prev` is where the read-back restore finds the state before the
    // current transition (q0, then the slot last written)
    double *rec = a.samples;
    const double *prev = a.q0;
    int rec_wait = a.thin;

    for (int s = 0; s < a.n; ++s) {
        if (PRIO) {
            const int left = (a.n - 1 - s) / GAUSS_PRIO_WINDOW;
            gauss_set_priority(left < 3 ? left : 3);
        }
        const double hdt = (UDT && SHARED) ? a.half_timestep : 0.5 * dt;
        if (RNG != GAUSS_RNG_HBM) gen = xo_seed(gen_stream, a.rng_seed, a.rng_offset + (uint64_t)s);
        // state before the transition -> LDS (read back only on rejection)
        if (RNG != GAUSS_RNG_DUMP && stash_lds) {
            if constexpr (WIDE) {
#pragma unroll
                for (int r = 0; r < TMAX / 2; ++r)
                    gauss_st2(&stash[wib][0][0] + 128 * r + 2 * lane, q[2 * r], q[2 * r + 1]);
            } else {
#pragma unroll
                for (int t = 0; t < TMAX; ++t) stash[wib][t][lane] = q[t];
            }
        }

        // Prefetches are issued UNCONDITIONALLY (on the last transition they
        // re-read this transition's data and are ignored): a load under a
        // branch makes the compiler's vmcnt bookkeeping assume it may not have
        // been issued, and the next counted wait then also waits for it.
        const bool more = s + 1 < a.n;
        const double *pc = a.p0 + (int64_t)s * CD + base;
        const double *pn = more ? pc + CD : pc;
        double un = 0.0;
        if (RNG == GAUSS_RNG_HBM) un = a.u[(int64_t)(more ? s + 1 : s) * a.C + chain];

        LaneSum spb = {0.0, 0.0}, sqa = {0.0, 0.0}, spa = {0.0, 0.0};   // ONESUM: spa stays unused
        double Spb = 0.0;                                     // EARLY: summed in the last group
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            double(&cur)[GS] = (RNG == GAUSS_RNG_HBM && (g & 1)) ? pb : pa;
            double(&nxt)[GS] = (RNG == GAUSS_RNG_HBM && (g & 1)) ? pa : pb;
            if (RNG != GAUSS_RNG_HBM) {
                // this group's momentum draw, np.random.normal (hmc.py:146)
                unsigned want = 0;
#pragma unroll
                for (int i = 0; i < GS; ++i)
                    if (REGULAR || (8 * (g * GS + i) + j < n)) want |= 1u << i;
                xzig_normals<GS>(cur, want, gen, zx);
                if (RNG == GAUSS_RNG_DUMP) {
                    if (cvalid && canonical) {
                        double *go = a.p_dump + (int64_t)s * CD + base;
#pragma unroll
                        for (int i = 0; i < GS; ++i)
                            if (want & (1u << i)) go[8 * (g * GS + i)] = cur[i];
                    }
                    continue;
                }
            } else if (WIDE) {
                const double *pg = (g + 1 < NG) ? pc + 128 * ((g + 1) * (GS / 2)) : pn;
#pragma unroll
                for (int r = 0; r < GS / 2; ++r) gauss_ld2<NT_P0>(nxt[2 * r], nxt[2 * r + 1], pg + 128 * (r - WR0));
            } else if (g + 1 < NG) {
#pragma unroll
                for (int i = 0; i < GS; ++i) {
                    const int t = (g + 1) * GS + i;
                    const bool m = REGULAR || (8 * t + j < n);
                    nxt[i] = m ? pc[8 * t] : 0.0;
                }
            } else {
#pragma unroll
                for (int i = 0; i < GS; ++i) {
                    const bool m = REGULAR || (8 * i + j < n);
                    nxt[i] = m ? pn[8 * i] : 0.0;
                }
            }
            (void)nxt;
            // pin this group's values to this point: without it the compiler
            // forms the p*p / q*q products of every group early and keeps
            // them alive until the group's turn
#pragma unroll
            for (int i = 0; i < GS; ++i)
                asm volatile("" : "+v"(cur[i]), "+v"(q[g * GS + i]));
            if (s == 0) {
#pragma unroll
                for (int i = 0; i < GS; ++i) {
                    const int t = g * GS + i;
                    const double d = UNIT ? q[t] : q[t] - a.x0;
                    if (FASTSUM) lane_sum_fused(s0, d, t);
                    else lane_sum_add<REGULAR>(s0, d * d, t, T);
                }
                if (FIXED && !SHARED && g == NG - 1) {
                    double v[1] = {s0.r};
                    chain_sum_finish_fixed<HF, 1>(v, lane);
                    Sq_state = v[0];
                }
            }
#pragma unroll
            for (int i = 0; i < GS; ++i) {                    // hmc.py:148
                if (FASTSUM) lane_sum_fused(spb, cur[i], g * GS + i);
                else lane_sum_add<REGULAR>(spb, cur[i] * cur[i], g * GS + i, T);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (EARLY && g == NG - 1) {
                // the drawn momentum's sum is complete: its tree goes up here, beside the
                // half kick below, instead of on the transition's tail
                double v[1] = {spb.r};
                chain_sum_finish_fixed<HF, 1>(v, lane);
                Spb = v[0];
            }
#pragma unroll
            for (int i = 0; i < GS; ++i) {                    // hmc.py:116
                const int t = g * GS + i;
                cur[i] = kick<FMA>(cur[i], hdt, gauss_grad<UNIT>(q[t], a.k, a.x0));
            }
            if (EARLY && g == NG - 1) asm volatile("" : "+v"(Spb));
            if (USTEP == 1) {
                // the bare loop, spelled out (not the blocked form at USTEP = 1) so that these
                // instantiations compile to exactly the code they had before the unrolled form
                for (int l = 0; l < a.nsteps - 1; ++l) {      // hmc.py:118-120
#pragma unroll
                    for (int i = 0; i < GS; ++i) {
                        const int t = g * GS + i;
                        q[t] = drift<FMA>(q[t], cur[i], dt);
                        cur[i] = kick<FMA>(cur[i], dt, gauss_grad<UNIT>(q[t], a.k, a.x0));
                    }
                }
            } else {
                const auto step = [&]() {
#pragma unroll
                    for (int i = 0; i < GS; ++i) {
                        const int t = g * GS + i;
                        q[t] = drift<FMA>(q[t], cur[i], dt);
                        cur[i] = kick<FMA>(cur[i], dt, gauss_grad<UNIT>(q[t], a.k, a.x0));
                    }
                };
                static_assert((USTEP & (USTEP - 1)) == 0, "the remainder below goes by the bits of its count");
                const int nl = a.nsteps > 1 ? a.nsteps - 1 : 0;   // hmc.py:118-120
                // USTEP steps per back-edge, then the remaining steps in straight line, one
                // block per bit of their count: L = 20 takes 3 back-edges per group, not 18
#pragma unroll 1
                for (int m = nl / USTEP; m > 0; --m) {
#pragma unroll
                    for (int k = 0; k < USTEP; ++k) step();
                }
#pragma unroll
                for (int b = USTEP >> 1; b > 0; b >>= 1) {
                    if (nl & b) {
#pragma unroll
                        for (int k = 0; k < b; ++k) step();
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < GS; ++i) {                    // hmc.py:122-123
                const int t = g * GS + i;
                q[t] = drift<FMA>(q[t], cur[i], dt);
                // ONESUM: the end momentum feeds nothing, the trajectory ends with the drift
                if (!ONESUM) cur[i] = kick<FMA>(cur[i], hdt, gauss_grad<UNIT>(q[t], a.k, a.x0));
            }
#pragma unroll
            for (int i = 0; i < GS; ++i) {                    // hmc.py:150
                const int t = g * GS + i;
                const double d = UNIT ? q[t] : q[t] - a.x0;
                if (ONESUM) {
                    lane_sum_fused(sqa, d, t);
                } else if (FASTSUM) {
                    lane_sum_fused(sqa, d, t);
                    lane_sum_fused(spa, cur[i], t);
                } else {
                    lane_sum_add<REGULAR>(sqa, d * d, t, T);
                    lane_sum_add<REGULAR>(spa, cur[i] * cur[i], t, T);
                }
            }
            // ... and pin the running sums here: otherwise the group's last
            // half kick and its squares are sunk below the NEXT group's step
            // loop and its momenta stay live through it
            if (ONESUM)
                asm volatile("" : "+v"(sqa.r), "+v"(spb.r));
            else if (EARLY && g == NG - 1)
                asm volatile("" : "+v"(sqa.r), "+v"(spa.r));
            else
                asm volatile("" : "+v"(sqa.r), "+v"(spa.r), "+v"(spb.r));
            __builtin_amdgcn_sched_barrier(0);
        }
        if (RNG != GAUSS_RNG_HBM) {
            // the acceptance draw, np.random.uniform (hmc.py:151): every lane
            // advances its stream, the chain uses the one of its first lane
            const double ud = xo_uniform53(gen);
            if (LW == 0) {
                uu = shfl_f64(ud, lane & ~((1 << lg) - 1));
            } else {
                // the first lane of the chain's first wave draws for all its waves
                if (wchain == 0 && lane == 0) ubc[wib] = ud;
                __syncthreads();
                uu = ubc[wib & ~(WPC - 1)];
                __syncthreads();
            }
            if (RNG == GAUSS_RNG_DUMP) {
                if (cvalid && writer) a.u_dump[(int64_t)s * a.C + chain] = uu;
                continue;
            }
        }
        if (RNG == GAUSS_RNG_HBM && (NG & 1)) {
            // odd group count: the next transition's group 0 landed in pb
#pragma unroll
            for (int i = 0; i < GS; ++i) pa[i] = pb[i];
        }
        double Sqa, Spa = 0.0;
        if (ONESUM) {
            // lanes 0 / 4 / 8: Sqa, Spb and, on the first transition, the start state's
            const double r = chain_sums_shared2(sqa.r, spb.r, s0.r, s == 0);
            Sqa = lane_value_f64<0>(r);
            Spb = lane_value_f64<4>(r);
            if (s == 0) Sq_state = lane_value_f64<8>(r);
        } else if (SHARED) {
            // lanes 0 / 4 / 8 / 12: Sqa, Spa, Spb and, on the first transition, the start state's
            const double r = chain_sums_shared(sqa.r, spa.r, spb.r, s0.r, s == 0);
            Sqa = lane_value_f64<0>(r);
            Spa = lane_value_f64<4>(r);
            Spb = lane_value_f64<8>(r);
            if (s == 0) Sq_state = lane_value_f64<12>(r);
        } else if (FIXED) {
            if (EARLY) {
                double v[2] = {sqa.r, spa.r};                 // one tree, two chains per level
                chain_sum_finish_fixed<HF, 2>(v, lane);
                Sqa = v[0];
                Spa = v[1];
            } else {
                double v[3] = {spb.r, sqa.r, spa.r};
                chain_sum_finish_fixed<HF, 3>(v, lane);
                Spb = v[0];
                Sqa = v[1];
                Spa = v[2];
            }
        } else {
            if (s == 0)
                Sq_state = chain_sum_finish<REGULAR, LW>(s0, T, rem, lane, H, leafdepth, xch, wib);
            Spb = chain_sum_finish<REGULAR, LW>(spb, T, rem, lane, H, leafdepth, xch, wib);
            Sqa = chain_sum_finish<REGULAR, LW>(sqa, T, rem, lane, H, leafdepth, xch, wib);
            Spa = chain_sum_finish<REGULAR, LW>(spa, T, rem, lane, H, leafdepth, xch, wib);
        }
        const double Eb = -(c_lp * Sq_state) + 0.5 * Spb;
        const double Ea = -(c_lp * Sqa) + 0.5 * Spa;          // ONESUM: not used

        // The bounds of metropolis_accept and the scalar constants above: in the SHARED
        // kernels only.  Elsewhere the bounds' registers cost occupancy (the regular TMAX
        // 1 / 2 / 4 kernels with a per-lane step go from 98 to 102 SGPRs and from 8 to 7
        // waves per SIMD, the regular 2-wave non-unit ones from 127 to 130 VGPRs and from 4
        // to 3), where the kernels as they are lose none.
        bool acc;
        if (FASTSUM) {
            // Eb, Ea: of the fused sums.  delta: accept_decide's derivation; it needs k > 0.
            // ONESUM: the exponent from the two sums of squares of the state and delta from
            // gauss_onesum_factor's derivation (gauss_common.hpp); Ea <= Eb + |dH|.
            const double xt = ONESUM ? -(a.c_dh * (Sqa - Sq_state)) : -(Ea - Eb);
            const double delta = ONESUM ? a.f_dh * ((Eb + Eb) + __builtin_fabs(xt)) : 0x1p-46 * (Eb + Ea);
            const int dec = accept_decide(uu, xt, delta);
            acc = dec == GAUSS_ACCEPT;
            // One chain per wave: the same for every lane, and a branch the wave does not
            // enter.  Its loads are drained inside it, as the rejection restore's are below:
            // the counted waits after the join then count what the steady path issued.
            if (__builtin_amdgcn_ballot_w64(dec == GAUSS_UNDECIDED || !(c_lp < 0.0)) != 0) {
                // numpy's order needs numpy's ownership: base_np, not the lane's own base
                acc = gauss_exact_accept<TMAX, GAUSS_REDO_GS, UNIT, FMA, WIDE>(
                    a, prev + base_np, stash_lds ? stash[wib] : nullptr, lane, pc + (base_np - base), dt, hdt,
                    c_lp, uu);
                __builtin_amdgcn_s_waitcnt(0);                // vmcnt(0) expcnt(0) lgkmcnt(0)
            }
        } else {
            acc = metropolis_accept<SHARED>(uu, -(Ea - Eb));  // hmc.py:151
        }

        if (!UDT && s < a.n_adapt)                            // hmc.py:188-191
            dt = acc ? dt * a.uprate : dt * a.downrate;
        if (cvalid && writer) {
            const int64_t o = (int64_t)s * a.C + chain;
            if (a.accepted) a.accepted[o] = acc ? 1 : 0;
            if (!ONESUM) {                                    // launched without energy buffers
                if (a.e_before) a.e_before[o] = Eb;
                if (a.e_after) a.e_after[o] = Ea;
            }
        }
        if (acc) {
            Sq_state = Sqa;
            nacc += 1;
        } else {
            // the rare path: the old state back, and a wait for exactly these reads
            // here.  Without it the waits of the record stores below would count these
            // reads on every path, and the accepted one (which issued none) would wait
            // on the momentum prefetches in flight instead.
            if (WIDE && stash_lds) {
#pragma unroll
                for (int r = 0; r < TMAX / 2; ++r)
                    gauss_ld2(q[2 * r], q[2 * r + 1], &stash[wib][0][0] + 128 * r + 2 * lane);
            } else if (WIDE) {
#pragma unroll
                for (int r = 0; r < TMAX / 2; ++r) gauss_ld2(q[2 * r], q[2 * r + 1], prev + base + 128 * (r - WR0));
            } else if (stash_lds) {
#pragma unroll
                for (int t = 0; t < TMAX; ++t) q[t] = stash[wib][t][lane];
            } else {
#pragma unroll
                for (int t = 0; t < TMAX; ++t) q[t] = prev[base + 8 * t];
            }
            __builtin_amdgcn_s_waitcnt(0);                    // vmcnt(0) expcnt(0) lgkmcnt(0)
        }
        if (a.samples && --rec_wait == 0) {
            rec_wait = a.thin;
            if (cvalid && canonical) {
                double *go = rec + base;
                if constexpr (WIDE) {
#pragma unroll
                    for (int r = 0; r < TMAX / 2; ++r) gauss_st2<NT_REC>(go + 128 * (r - WR0), q[2 * r], q[2 * r + 1]);
                } else {
#pragma unroll
                    for (int t = 0; t < TMAX; ++t)
                        if (REGULAR || (8 * t + j < n)) go[8 * t] = q[t];
                }
            }
            prev = rec;
            rec += CD;
        }
        if (RNG == GAUSS_RNG_HBM) uu = un;
    }
    if (RNG == GAUSS_RNG_DUMP) return;
    if (PRIO) __builtin_amdgcn_s_setprio(0);

    if (cvalid && writer) {
        if (a.n_accepted) a.n_accepted[chain] += nacc;
        if (!UDT && a.n_adapt > 0 && a.dt_chain) a.dt_chain[chain] = dt;
    }
    if (cvalid && canonical) {
        double *go = a.q_out + base;
        if constexpr (WIDE) {
#pragma unroll
            for (int r = 0; r < TMAX / 2; ++r) gauss_st2(go + 128 * (r - WR0), q[2 * r], q[2 * r + 1]);
        } else {
#pragma unroll
            for (int t = 0; t < TMAX; ++t)
                if (REGULAR || (8 * t + j < n)) go[8 * t] = q[t];
        }
    }
}


}  // namespace binf
