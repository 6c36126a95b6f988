// Pair-distance model, force scheme "sym" (32 .. 256 beads).  Included by pairdist.hip
// alone, after pairdist_force.hpp.
#pragma once
#include "pairdist_force.hpp"

namespace binf {

// ---------------------------------------------------------------------------
// 32 <= n_beads <= 256: every UNORDERED pair once, its target distance in a register.
//
// The all-pairs loops (pairdist_onesided.hpp) give each lane the pairs (i, j = ...) of ITS bead and
// read y[j][i] from memory for each: one CU streams the whole [n x n] target
// matrix (512 KiB at n = 256) per force evaluation, and that stream -- not the
// arithmetic -- is what a workgroup waits for (scripts/pairforce_probe.hip: 30 us
// per evaluation with the loads, 10 us without, at any number of chains).  Here
// one workgroup owns a chain and computes each pair {i, j} ONCE:
//
//  * beads in NBLK = ceil(n / 64) blocks of 64; the unordered block pairs go to
//    NBLK^2 waves (n = 256: 16 waves, a 1024-thread workgroup): waves 0..NBLK-1 the
//    diagonal blocks (b, b), the others the off-diagonal pairs (bi < bj), two
//    waves each (the halves h = 0, 1 of the partner range);
//  * lane l of a wave is ROW bead i = 64 bi + l for all of its 32 steps; at step
//    k its partner is COLUMN bead j = 64 bj + (l + off + k) mod 64 (off = 32 h,
//    or 1 on the diagonal, where step 31 -- partner l + 32 -- is done by lanes
//    0-31 only).  At every step the 64 lanes hold 64 different partners;
//  * the 32 target distances of a lane never change: they are loaded ONCE per
//    launch (tile rows through LDS, coalesced) and stay in 64 VGPRs -- the fused
//    leapfrog reads the target matrix once per trajectory instead of L + 1 times;
//  * one pair weight serves both beads: w (x_i - x_j) is added to the lane's own
//    sum F (row bead) and subtracted from a second sum R that belongs to the
//    partner bead; since the partner advances by one column per step, R
//    is passed to the neighbouring lane after every step (wave_rol:1), so it
//    stays with its bead.  Half the arithmetic of the one-sided loops;
//  * a bead's 8 partial sums (partner block b' = 0..3: the diagonal wave's F and
//    R for b' = b, else the two half-waves' sums) are added in that order by the
//    bead's owner thread (threads 0-255) -- a fixed order that depends on n
//    only, so results are bit-identical for any number of chains, and the fused
//    leapfrog is bit-identical to the per-step tier (both use this scheme for
//    n <= 256; the one-sided kernels serve larger n).
// ---------------------------------------------------------------------------
constexpr int SYM_MAX_BEADS = 256;
constexpr int SYM_MIN_BEADS = 32;        // fewer: most of the 32 steps would be masked (one-sided loops)
constexpr int SYM_STEPS = 32;
constexpr int SYM_ROWS = 8;              // rows of a wave's 64 x 64 target tile staged at a time

// NBLK = ceil(n / 64) blocks of 64 beads -> NBLK^2 waves (NBLK diagonal blocks one wave
// each, NBLK (NBLK - 1) / 2 off-diagonal pairs two waves each): a 64- / 256- / 576- /
// 1024-thread workgroup.  A wave computes the same partial sums whatever NBLK is, a
// bead's partials are added in slot order, and the slots of blocks that do not exist
// would hold +0.0 and come last -- so choosing NBLK from n (small workgroups for few
// beads: 16 / 4 chains per CU at a time instead of 1) does not change a bit.
template <int NBLK>
struct SymShared {
    double sx[NBLK][3][128];             // positions [block][axis][slot]; slots 64-127 repeat 0-63
                                         // (a block's three axes within one ds_read2 offset range)
    union {
        double part[2 * NBLK][3][64 * NBLK];     // partial forces [partner block * 2 + k][axis][bead]
        double ytile[NBLK * NBLK][SYM_ROWS][64]; // launch prologue only
    } u;
};

struct SymRole {
    int bi, bj, h, off;
    bool diag;
};

template <int NBLK>
__device__ inline SymRole sym_role()
{
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    SymRole r;
    if (wave < NBLK) {
        r.bi = wave; r.bj = wave; r.h = 0; r.off = 1; r.diag = true;
    } else {
        int rem = (wave - NBLK) >> 1;              // pairs in the order (0,1) (0,2) .. (1,2) ..
        r.h = (wave - NBLK) & 1;
        r.bi = 0;
        while (rem >= NBLK - 1 - r.bi) { rem -= NBLK - 1 - r.bi; ++r.bi; }
        r.bj = r.bi + 1 + rem;
        r.off = 32 * r.h;
        r.diag = false;
    }
    return r;
}

// The lane's 32 target distances y[k] = ymat[64 bi + l][64 bj + (l + off + k) mod 64]
// (0 where a bead does not exist), and the bit mask of its pairs that do exist.
template <int NBLK, bool PK>
__device__ inline void sym_load_targets(double (&y)[SYM_STEPS], unsigned &live, SymShared<NBLK> &sh,
                                        const double *ymat, const double *ypk, int n,
                                        const SymRole &ro)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if constexpr (PK) {
        // packed by sym_pack_targets_kernel: step k of wave w, lane l at ypk[(32 w + k) 64 + l]
        // -- 32 independent coalesced loads, no exchange through LDS
        const double *src = ypk + (int64_t)wave * SYM_STEPS * 64 + lane;
#pragma unroll
        for (int k = 0; k < SYM_STEPS; ++k) y[k] = src[k * 64];
    } else {
    // The tile goes through a scratch area of the wave's own, SYM_ROWS rows at a
    // time (lane = column on the way in: coalesced 512-byte rows; lane = row on the
    // way out), the next rows' loads in flight meanwhile.  No other wave touches the
    // scratch: LDS serves a wave's instructions in order, so wave-level fences (no
    // s_barrier) are all the synchronisation the exchange needs.
    const int col = 64 * ro.bj + lane;
    double nxt[SYM_ROWS];
    auto fetch = [&](int r0) {
#pragma unroll
        for (int r = 0; r < SYM_ROWS; ++r) {
            const int row = 64 * ro.bi + r0 + r;
            nxt[r] = (row < n && col < n) ? ymat[(int64_t)row * n + col] : 0.0;
        }
    };
    fetch(0);
    for (int r0 = 0; r0 < 64; r0 += SYM_ROWS) {
#pragma unroll
        for (int r = 0; r < SYM_ROWS; ++r) sh.u.ytile[wave][r][lane] = nxt[r];
        if (r0 + SYM_ROWS < 64) fetch(r0 + SYM_ROWS);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (lane >= r0 && lane < r0 + SYM_ROWS) {
            const double *rowp = sh.u.ytile[wave][lane - r0];
#pragma unroll
            for (int k = 0; k < SYM_STEPS; ++k) y[k] = rowp[(lane + ro.off + k) & 63];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    __syncthreads();                     // the scratch shares its LDS with the partial sums
    }
    live = 0;
    const int i = 64 * ro.bi + lane;
#pragma unroll
    for (int k = 0; k < SYM_STEPS; ++k) {
        const int j = 64 * ro.bj + ((lane + ro.off + k) & 63);
        const bool ok = i < n && j < n && !(ro.diag && k == SYM_STEPS - 1 && lane >= 32);
        live |= ok ? (1u << k) : 0u;
    }
}

// The targets in the order the waves of the sym kernels hold them: a function of
// (ymat, n) alone, written once per model and read by every launch after that
// (256 beads: 256 KiB instead of a 512 KiB matrix walked tile by tile through LDS).
template <int NBLK>
__global__ void __launch_bounds__(1024) sym_pack_targets_kernel(const double *ymat, double *ypk, int n)
{
    const SymRole ro = sym_role<NBLK>();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = 64 * ro.bi + lane;
    for (int k = 0; k < SYM_STEPS; ++k) {
        const int j = 64 * ro.bj + ((lane + ro.off + k) & 63);
        ypk[((int64_t)wave * SYM_STEPS + k) * 64 + lane] =
            (i < n && j < n) ? ymat[(int64_t)i * n + j] : 0.0;
    }
}

// One force evaluation: this wave's partial sums to sh.u.part.  Positions must be
// in sh.sx (both copies); the caller synchronises before reading the partials.
// FULL: n == 64 NBLK, every pair exists except the diagonal waves' last half step.
template <bool FULL, int NBLK>
__device__ inline void sym_partials(const double (&y)[SYM_STEPS], unsigned live, SymShared<NBLK> &sh,
                                    int n, const SymRole &ro)
{
    const int lane = threadIdx.x & 63;
    double F0 = 0.0, F1 = 0.0, F2 = 0.0, R0 = 0.0, R1 = 0.0, R2 = 0.0;
    if (64 * ro.bi < n && 64 * ro.bj < n) {            // wave-uniform
        const double x0 = sh.sx[ro.bi][0][lane], x1 = sh.sx[ro.bi][1][lane],
                     x2 = sh.sx[ro.bi][2][lane];
        const double *pj0 = &sh.sx[ro.bj][0][lane + ro.off];
        const double *pj1 = &sh.sx[ro.bj][1][lane + ro.off];
        const double *pj2 = &sh.sx[ro.bj][2][lane + ro.off];
#pragma unroll
        for (int k = 0; k < SYM_STEPS; ++k) {
            const double d0 = x0 - pj0[k], d1 = x1 - pj1[k], d2 = x2 - pj2[k];
            // pair_weight() with the squared distance and both bookings contracted to
            // FMAs (24 instead of 29 VALU instructions per pair; the force is held to
            // 1e-10 of numpy's, not to its bits, in either arithmetic mode)
            const double s2 = __builtin_fma(d2, d2, __builtin_fma(d1, d1, d0 * d0));
            double r = __builtin_amdgcn_rsq(s2);
            r = r * __builtin_fma(-0.5 * s2 * r, r, 1.5);
            double w = __builtin_fma(-y[k], r, 1.0);
            if (FULL) {
                if (k == SYM_STEPS - 1) w = (ro.diag && lane >= 32) ? 0.0 : w;
            } else {
                w = ((live >> k) & 1u) ? w : 0.0;      // also discards the NaN of a 0-distance ghost
            }
            F0 = __builtin_fma(w, d0, F0); F1 = __builtin_fma(w, d1, F1); F2 = __builtin_fma(w, d2, F2);
            R0 = wave_rol1(__builtin_fma(-w, d0, R0));  // the partner's share is -w d; then R moves on
            R1 = wave_rol1(__builtin_fma(-w, d1, R1));
            R2 = wave_rol1(__builtin_fma(-w, d2, R2));
        }
    }
    const int slotF = ro.diag ? 2 * ro.bi : 2 * ro.bj + ro.h;
    const int slotR = ro.diag ? 2 * ro.bi + 1 : 2 * ro.bi + ro.h;
    const int bF = 64 * ro.bi + lane;
    const int bR = 64 * ro.bj + ((lane + ro.off + SYM_STEPS) & 63);
    sh.u.part[slotF][0][bF] = F0; sh.u.part[slotF][1][bF] = F1; sh.u.part[slotF][2][bF] = F2;
    sh.u.part[slotR][0][bR] = R0; sh.u.part[slotR][1][bR] = R1; sh.u.part[slotR][2][bR] = R2;
}

// Owner thread t (< 64 NBLK) of bead t: the bead's force, partials added in slot order.
template <int NBLK>
__device__ inline void sym_reduce(const SymShared<NBLK> &sh, int t, double (&f)[3])
{
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        double v = sh.u.part[0][ax][t];
#pragma unroll
        for (int sl = 1; sl < 2 * NBLK; ++sl) v = v + sh.u.part[sl][ax][t];
        f[ax] = v;
    }
}

template <int NBLK>
__device__ inline void sym_publish(SymShared<NBLK> &sh, int t, const double (&q)[3])
{
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        sh.sx[t >> 6][ax][t & 63] = q[ax];
        sh.sx[t >> 6][ax][(t & 63) + 64] = q[ax];
    }
}

// A workgroup loads its target distances once and then walks chains blockIdx.x,
// blockIdx.x + gridDim.x, ...: the launchers start as many workgroups as the chip
// holds at a time (126 VGPRs: 16 waves per CU), so with more chains than that the
// target load is paid once per workgroup, not once per chain.
// __launch_bounds__(1024) whatever NBLK: it is what keeps the kernel within 128 VGPRs.
template <bool FULL, int NBLK, bool PK>
__global__ void __launch_bounds__(1024)
pairdist_grad_sym_kernel(const double *x, const double *ymat, const double *ypk, double tau,
                         const double *tau_chain, double *out, int32_t n_beads, int64_t n_chains)
{
    __shared__ SymShared<NBLK> sh;
    const int n = n_beads, t = threadIdx.x;
    const SymRole ro = sym_role<NBLK>();
    double y[SYM_STEPS];
    unsigned live;
    sym_load_targets<NBLK, PK>(y, live, sh, ymat, ypk, n, ro);
    for (int64_t c = blockIdx.x; c < n_chains; c += gridDim.x) {
        const double *xc = x + c * 3 * (int64_t)n;
        if (t < 64 * NBLK) {
            double q[3];
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) q[ax] = (t < n) ? xc[3 * t + ax] : 0.0;
            sym_publish<NBLK>(sh, t, q);
        }
        __syncthreads();
        sym_partials<FULL, NBLK>(y, live, sh, n, ro);
        __syncthreads();
        if (t < n) {
            double f[3];
            sym_reduce<NBLK>(sh, t, f);
            store_scaled_force(out + c * 3 * (int64_t)n + 3 * t, tau_chain ? tau_chain[c] : tau, f[0], f[1], f[2]);
        }
    }
}

// The whole _leapfrog() (binf/samplers/hmc.py:92-125) in one launch with the
// scheme above: owner threads keep q and p of their bead in registers.
template <bool FMA, bool FULL, int NBLK, bool PK>
__global__ void __launch_bounds__(1024) pairdist_leapfrog_sym_kernel(const PairLeapArgs a)
{
    __shared__ SymShared<NBLK> sh;
    const int n = a.n_beads, t = threadIdx.x;
    const SymRole ro = sym_role<NBLK>();
    const bool owner = t < n;
    double y[SYM_STEPS];
    unsigned live;
    sym_load_targets<NBLK, PK>(y, live, sh, a.ymat, a.ypk, n, ro);
    for (int64_t c = blockIdx.x; c < a.n_chains; c += gridDim.x) {
        const PairChain ch = pair_chain(a, c);
        double q[3] = {0.0, 0.0, 0.0}, p[3] = {0.0, 0.0, 0.0};
        if (owner) {
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) { q[ax] = ch.qs[3 * t + ax]; p[ax] = ch.pc[3 * t + ax]; }
        }
        if (t < 64 * NBLK) sym_publish<NBLK>(sh, t, q);
        __syncthreads();
        // nsteps + 1 force evaluations: half kick, (nsteps - 1) x [drift, kick], drift, half kick
        for (int e = 0; e <= a.nsteps; ++e) {
            sym_partials<FULL, NBLK>(y, live, sh, n, ro);
            __syncthreads();
            if (owner) {
                double f[3];
                sym_reduce<NBLK>(sh, t, f);
                const double step = (e == 0 || e == a.nsteps) ? ch.hdt : ch.dt;
#pragma unroll
                for (int ax = 0; ax < 3; ++ax)
                    pair_kick<FMA>(a, f[ax], q[ax], p[ax], ch.tau, step, ch.dt, e < a.nsteps);
                if (e < a.nsteps) sym_publish<NBLK>(sh, t, q);
            }
            __syncthreads();
        }
        if (owner) {
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) { ch.qc[3 * t + ax] = q[ax]; ch.pc[3 * t + ax] = p[ax]; }
        }
    }
}

}  // namespace binf
