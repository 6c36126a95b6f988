// Pair-distance model, force schemes "ring" (257 .. 1024 beads, a workgroup per chain) and
// "tiles" (257 .. 8192 beads, a wave per tile): both walk the same tiles of the same packed
// targets (ring_phase, ring_chunk).  Included by pairdist.hip alone, after pairdist_force.hpp.
#pragma once
#include "pairdist_force.hpp"

namespace binf {

// ---------------------------------------------------------------------------
// 256 < n_beads <= 1024: every UNORDERED pair once as well -- the "ring" scheme.
//
// The sym scheme (pairdist_sym.hpp) keeps a bead's 2 NBLK partial sums in LDS and a wave's 32 target
// distances in registers for the whole launch; neither scales past 256 beads (512
// beads: 196 KB of partial sums, 128 targets per lane).  Here a workgroup of NBLK =
// ceil(n / 64) waves owns a chain, wave b = the 64 ROW beads of block b, and the block
// pairs are walked in PHASES that every wave takes together:
//
//   phase 0       the diagonal tile (b, b): 31.5 steps, partner l + 1 + m (as above)
//   phase s >= 1  the tile (b, (b + s) mod NBLK): 64 steps, partner column l + m;
//                 s runs to NBLK / 2.  For an even NBLK the last phase pairs antipodal
//                 blocks, which see each other from both sides: the lower block takes
//                 the column offsets 0..31, the upper one 1..32 (32 steps each) -- an
//                 exact cover of the tile.
//
//  * In every phase each COLUMN block is visited by exactly one wave.  A lane adds
//    w (x_i - x_j) to its row bead's sum F (a register for the whole evaluation) and
//    subtracts it from the partner's sum R, which moves on by one lane per step
//    (wave_rol1) and so stays with its bead; at the end of a phase R goes to ONE LDS
//    slot per bead, and after a barrier the bead's owner adds it to a second register
//    G.  The force is F + G: F summed in step order, G in phase order -- a fixed order
//    that depends on n only, so results are bit-identical for any number of chains and
//    the fused leapfrog is bit-identical to the per-step tier.  Half the arithmetic of
//    the one-sided loops, one barrier per phase (5 at 512 beads, 9 at 1024).
//  * The targets cannot stay in registers: they are read again for every force
//    evaluation, 8 steps ahead of their use, from the packed array (ring_pack_targets_
//    kernel: step t of wave b, lane l at ypk[(b T + t) 64 + l] -- coalesced, 1 MiB at
//    512 beads, shared by all chains and resident in L2).
// ---------------------------------------------------------------------------
constexpr int RING_MAX_BEADS = 1024;     // a workgroup (<= 16 waves) per chain
constexpr int TILES_MAX_BEADS = 8192;    // a wave per tile: any number of blocks (packed targets: 256 MiB here)
constexpr int RING_CHUNK = 8;            // steps whose targets are in flight / in use at a time
                                         // (4: -2 %, 16: -8 % at 512 .. 1024 beads, same-box A/B)

__host__ __device__ inline int ring_steps(int nblk)      // steps a wave walks per force evaluation
{
    return (nblk & 1) ? 32 + 64 * (nblk / 2) : 64 * (nblk / 2);
}

struct RingPhase {
    int bj, off, steps;
};

__host__ __device__ inline RingPhase ring_phase(int nblk, int bi, int s)
{
    RingPhase ph;
    if (s == 0) {
        ph.bj = bi; ph.off = 1; ph.steps = 32;
    } else {
        const bool half = !(nblk & 1) && s == nblk / 2;
        ph.bj = bi + s; if (ph.bj >= nblk) ph.bj -= nblk;
        ph.off = (half && bi >= nblk / 2) ? 1 : 0;
        ph.steps = half ? 32 : 64;
    }
    return ph;
}

template <int NBT>
struct RingShared {
    double sx[NBT][3][128];              // positions [block][axis][slot]; slots 64-127 repeat 0-63
    double racc[2][NBT][3][64];          // a phase's column-side sums [buffer][block][axis][bead]
};

// The targets in the order the waves of the ring kernels read them.
__global__ void __launch_bounds__(256) ring_pack_targets_kernel(const double *ymat, double *ypk, int n, int nblk)
{
    const int bi = blockIdx.x, lane = threadIdx.x & 63;
    const int total = ring_steps(nblk);
    const int i = 64 * bi + lane;
    for (int t = threadIdx.x >> 6; t < total; t += blockDim.x >> 6) {
        const int s = t < 32 ? 0 : 1 + (t - 32) / 64;
        const int m = t < 32 ? t : (t - 32) % 64;
        const RingPhase ph = ring_phase(nblk, bi, s);
        const int j = 64 * ph.bj + ((lane + ph.off + m) & 63);
        ypk[((int64_t)bi * total + t) * 64 + lane] = (i < n && j < n) ? ymat[(int64_t)i * n + j] : 0.0;
    }
}

// RING_CHUNK steps of a phase.  MASK: some of this tile's pairs do not exist (the last half
// step of a diagonal tile; beads beyond n when n is not a multiple of 64 and the row or the
// column block is the last one) -- bit k of `live` says whether the pair of step m0 + k does.
template <bool MASK>
__device__ inline void ring_chunk(const double (&y)[RING_CHUNK], const double *pj0, const double *pj1,
                                  const double *pj2, int m0, double x0, double x1, double x2,
                                  unsigned live,
                                  double &F0, double &F1, double &F2, double &R0, double &R1, double &R2)
{
#pragma unroll
    for (int k = 0; k < RING_CHUNK; ++k) {
        const int m = m0 + k;
        const double d0 = x0 - pj0[m], d1 = x1 - pj1[m], d2 = x2 - pj2[m];
        const double s2 = __builtin_fma(d2, d2, __builtin_fma(d1, d1, d0 * d0));
        double r = __builtin_amdgcn_rsq(s2);
        r = r * __builtin_fma(-0.5 * s2 * r, r, 1.5);
        double w = __builtin_fma(-y[k], r, 1.0);
        if (MASK) w = ((live >> k) & 1u) ? w : 0.0;     // also discards the NaN of a 0-distance ghost pair
        F0 = __builtin_fma(w, d0, F0); F1 = __builtin_fma(w, d1, F1); F2 = __builtin_fma(w, d2, F2);
        R0 = wave_rol1(__builtin_fma(-w, d0, R0));
        R1 = wave_rol1(__builtin_fma(-w, d1, R1));
        R2 = wave_rol1(__builtin_fma(-w, d2, R2));
    }
}

// One force evaluation of the chain whose positions are in sh.sx (both copies): the force on
// this thread's bead (wave = block, lane = bead in the block) in f.  Every wave of the
// workgroup must call it; it ends behind the last phase's barrier, so the caller may
// overwrite sh.sx at once (and must synchronise before the next evaluation).
template <bool FULL, int NBT>
__device__ inline void ring_force(RingShared<NBT> &sh, const double *ypk, int n, int nblk, int &buf,
                                  double (&f)[3])
{
    const int bi = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int total = ring_steps(nblk);
    const double *yp = ypk + (int64_t)bi * total * 64 + lane;
    const double x0 = sh.sx[bi][0][lane], x1 = sh.sx[bi][1][lane], x2 = sh.sx[bi][2][lane];
    const bool row_ok = 64 * bi + lane < n;
    double F0 = 0.0, F1 = 0.0, F2 = 0.0, G0 = 0.0, G1 = 0.0, G2 = 0.0;
    double y[RING_CHUNK], yn[RING_CHUNK];
#pragma unroll
    for (int k = 0; k < RING_CHUNK; ++k) y[k] = yp[k * 64];
    int t = 0;
    const int nph = nblk / 2;
    for (int s = 0; s <= nph; ++s) {
        const RingPhase ph = ring_phase(nblk, bi, s);
        const double *pj0 = &sh.sx[ph.bj][0][lane + ph.off];
        const double *pj1 = &sh.sx[ph.bj][1][lane + ph.off];
        const double *pj2 = &sh.sx[ph.bj][2][lane + ph.off];
        // which of the lane's pairs exist in this tile: bit m <-> step m (wave-uniform test)
        const bool mask = s == 0 || (!FULL && (bi == nblk - 1 || ph.bj == nblk - 1));
        unsigned long long live = ~0ull;
        if (mask) {
            const int col_lim = n - 64 * ph.bj;                               // columns that exist
            const unsigned long long cols = col_lim >= 64 ? ~0ull : ((1ull << col_lim) - 1ull);
            const int rot = (lane + ph.off) & 63;                             // bit m <- column (rot + m) mod 64
            live = rot ? ((cols >> rot) | (cols << (64 - rot))) : cols;
            if (!row_ok) live = 0ull;
            if (s == 0 && lane >= 32) live &= ~(1ull << 31);                  // partner l + 32: lanes 0-31 only
        }
        double P0 = 0.0, P1 = 0.0, P2 = 0.0, R0 = 0.0, R1 = 0.0, R2 = 0.0;   // this TILE's row / column sums
        for (int m0 = 0; m0 < ph.steps; m0 += RING_CHUNK) {
            const bool more = t + RING_CHUNK < total;                         // wave-uniform
            if (more) {
#pragma unroll
                for (int k = 0; k < RING_CHUNK; ++k) yn[k] = yp[(int64_t)(t + RING_CHUNK + k) * 64];
            }
            if (mask) ring_chunk<true>(y, pj0, pj1, pj2, m0, x0, x1, x2, (unsigned)(live >> m0), P0, P1, P2, R0, R1, R2);
            else      ring_chunk<false>(y, pj0, pj1, pj2, m0, x0, x1, x2, 0u, P0, P1, P2, R0, R1, R2);
            if (more) {
#pragma unroll
                for (int k = 0; k < RING_CHUNK; ++k) y[k] = yn[k];
            }
            t += RING_CHUNK;
        }
        // a bead's force is the sum of its tiles' partial sums in phase order (row side F, column
        // side G) -- the same numbers whether one workgroup walks the phases (here) or every tile
        // is a wave of its own (pairdist_tiles_kernel below)
        F0 = s == 0 ? P0 : F0 + P0; F1 = s == 0 ? P1 : F1 + P1; F2 = s == 0 ? P2 : F2 + P2;
        // the column-side sums of this phase to their beads' slots; one wave per column block
        const int col = (lane + ph.off + ph.steps) & 63;
        sh.racc[buf][ph.bj][0][col] = R0; sh.racc[buf][ph.bj][1][col] = R1; sh.racc[buf][ph.bj][2][col] = R2;
        __syncthreads();
        G0 = G0 + sh.racc[buf][bi][0][lane]; G1 = G1 + sh.racc[buf][bi][1][lane]; G2 = G2 + sh.racc[buf][bi][2][lane];
        buf ^= 1;
    }
    f[0] = F0 + G0; f[1] = F1 + G1; f[2] = F2 + G2;
}

template <int NBT>
__device__ inline void ring_publish(RingShared<NBT> &sh, int t, const double (&q)[3])
{
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        sh.sx[t >> 6][ax][t & 63] = q[ax];
        sh.sx[t >> 6][ax][(t & 63) + 64] = q[ax];
    }
}

// One force evaluation per chain (the per-step tier's gradient): 64 NBLK threads per
// workgroup, a workgroup walks chains blockIdx.x, blockIdx.x + gridDim.x, ...
template <bool FULL, int NBT>
__global__ void __launch_bounds__(1024)
pairdist_grad_ring_kernel(const double *x, const double *ypk, double tau, const double *tau_chain,
                          double *out, int32_t n_beads, int32_t nblk, int64_t n_chains)
{
    __shared__ RingShared<NBT> sh;
    const int n = n_beads, t = threadIdx.x;
    int buf = 0;
    for (int64_t c = blockIdx.x; c < n_chains; c += gridDim.x) {
        const double *xc = x + c * 3 * (int64_t)n;
        double q[3];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) q[ax] = (t < n) ? xc[3 * t + ax] : 0.0;
        ring_publish<NBT>(sh, t, q);
        __syncthreads();
        double f[3];
        ring_force<FULL, NBT>(sh, ypk, n, nblk, buf, f);
        if (t < n) store_scaled_force(out + c * 3 * (int64_t)n + 3 * t, tau_chain ? tau_chain[c] : tau, f[0], f[1], f[2]);
    }
}

// The whole _leapfrog() (binf/samplers/hmc.py:92-125) in one launch with the ring scheme:
// every thread keeps q and p of its bead in registers.
template <bool FMA, bool FULL, int NBT>
__global__ void __launch_bounds__(1024) pairdist_leapfrog_ring_kernel(const PairLeapArgs a, int32_t nblk)
{
    __shared__ RingShared<NBT> sh;
    const int n = a.n_beads, t = threadIdx.x;
    const bool owner = t < n;
    int buf = 0;
    for (int64_t c = blockIdx.x; c < a.n_chains; c += gridDim.x) {
        const PairChain ch = pair_chain(a, c);
        double q[3] = {0.0, 0.0, 0.0}, p[3] = {0.0, 0.0, 0.0};
        if (owner) {
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) { q[ax] = ch.qs[3 * t + ax]; p[ax] = ch.pc[3 * t + ax]; }
        }
        ring_publish<NBT>(sh, t, q);
        __syncthreads();
        // nsteps + 1 force evaluations: half kick, (nsteps - 1) x [drift, kick], drift, half kick
        for (int e = 0; e <= a.nsteps; ++e) {
            double f[3];
            ring_force<FULL, NBT>(sh, a.ypk, n, nblk, buf, f);
            if (owner) {
                const double step = (e == 0 || e == a.nsteps) ? ch.hdt : ch.dt;
#pragma unroll
                for (int ax = 0; ax < 3; ++ax)
                    pair_kick<FMA>(a, f[ax], q[ax], p[ax], ch.tau, step, ch.dt, e < a.nsteps);
                if (e < a.nsteps) ring_publish<NBT>(sh, t, q);
            }
            __syncthreads();
        }
        if (owner) {
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) { ch.qc[3 * t + ax] = q[ax]; ch.pc[3 * t + ax] = p[ax]; }
        }
    }
}

// ---------------------------------------------------------------------------
// The same tiles with FEW chains: a workgroup per chain (above) leaves the chip idle
// when there are fewer chains than CUs -- 32 replicas of a 1000-bead model use an eighth
// of it.  Here every tile (row block b, phase s) is a wave of its own, whatever chain it
// belongs to: the tile's row-side and column-side sums go to a workspace
// (part[chain][tile][side][axis][bead in block]) and a second launch adds a bead's
// partial sums in the ring kernels' order -- the same bits -- and scales, kicks or drifts.
// ---------------------------------------------------------------------------
constexpr int TILE_WAVES = 4;            // tiles per workgroup

__host__ __device__ inline int ring_tiles(int nblk) { return nblk * (nblk / 2 + 1); }

template <bool FULL>
__global__ void __launch_bounds__(64 * TILE_WAVES)
pairdist_tiles_kernel(const double *x, const double *ypk, double *part, int32_t n, int32_t nblk)
{
    __shared__ double sxw[TILE_WAVES][3][128];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int nph = nblk / 2, ntiles = ring_tiles(nblk);
    const int tile = blockIdx.x * TILE_WAVES + wave;
    if (tile >= ntiles) return;                      // no workgroup barrier below
    const int bi = tile / (nph + 1), s = tile - bi * (nph + 1);
    const int64_t c = blockIdx.y;
    const double *xc = x + c * 3 * (int64_t)n;
    const RingPhase ph = ring_phase(nblk, bi, s);
    const int i = 64 * bi + lane, jb = 64 * ph.bj + lane;
    const bool row_ok = i < n;
    double x0 = 0.0, x1 = 0.0, x2 = 0.0;
    if (row_ok) { x0 = xc[3 * i]; x1 = xc[3 * i + 1]; x2 = xc[3 * i + 2]; }
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        const double v = jb < n ? xc[3 * jb + ax] : 0.0;
        sxw[wave][ax][lane] = v;
        sxw[wave][ax][lane + 64] = v;
    }
    // the wave's own scratch: LDS serves a wave's instructions in order, wave-level fences do
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const double *pj0 = &sxw[wave][0][lane + ph.off];
    const double *pj1 = &sxw[wave][1][lane + ph.off];
    const double *pj2 = &sxw[wave][2][lane + ph.off];
    const bool mask = s == 0 || (!FULL && (bi == nblk - 1 || ph.bj == nblk - 1));
    unsigned long long live = ~0ull;
    if (mask) {
        const int col_lim = n - 64 * ph.bj;
        const unsigned long long cols = col_lim >= 64 ? ~0ull : ((1ull << col_lim) - 1ull);
        const int rot = (lane + ph.off) & 63;
        live = rot ? ((cols >> rot) | (cols << (64 - rot))) : cols;
        if (!row_ok) live = 0ull;
        if (s == 0 && lane >= 32) live &= ~(1ull << 31);
    }
    const int t0 = s == 0 ? 0 : 32 + 64 * (s - 1);
    const double *yp = ypk + ((int64_t)bi * ring_steps(nblk) + t0) * 64 + lane;
    double y[RING_CHUNK], yn[RING_CHUNK];
#pragma unroll
    for (int k = 0; k < RING_CHUNK; ++k) y[k] = yp[k * 64];
    double P0 = 0.0, P1 = 0.0, P2 = 0.0, R0 = 0.0, R1 = 0.0, R2 = 0.0;
    for (int m0 = 0; m0 < ph.steps; m0 += RING_CHUNK) {
        const bool more = m0 + RING_CHUNK < ph.steps;
        if (more) {
#pragma unroll
            for (int k = 0; k < RING_CHUNK; ++k) yn[k] = yp[(int64_t)(m0 + RING_CHUNK + k) * 64];
        }
        if (mask) ring_chunk<true>(y, pj0, pj1, pj2, m0, x0, x1, x2, (unsigned)(live >> m0), P0, P1, P2, R0, R1, R2);
        else      ring_chunk<false>(y, pj0, pj1, pj2, m0, x0, x1, x2, 0u, P0, P1, P2, R0, R1, R2);
        if (more) {
#pragma unroll
            for (int k = 0; k < RING_CHUNK; ++k) y[k] = yn[k];
        }
    }
    double *o = part + ((c * ntiles + tile) * 2) * 3 * 64;
    const int col = (lane + ph.off + ph.steps) & 63;
    o[0 * 64 + lane] = P0; o[1 * 64 + lane] = P1; o[2 * 64 + lane] = P2;
    o[3 * 64 + col] = R0; o[4 * 64 + col] = R1; o[5 * 64 + col] = R2;
}

// A bead's force from the tiles' partial sums, in the ring kernels' order.  The loads of four
// tiles (three axes each) are issued before their sums are added one after the other: a loop
// that waits for every load cost 59 us per force evaluation at 8 chains of 4096 beads.
__device__ inline void tiles_force(const double *part, int64_t c, int bead, int nblk, double (&f)[3])
{
    constexpr int UN = 4;
    const int nph = nblk / 2, ntiles = ring_tiles(nblk);
    const int b = bead >> 6, l = bead & 63;
    const double *pc = part + c * ntiles * 2 * 3 * 64 + l;
    double F[3] = {0.0, 0.0, 0.0}, G[3] = {0.0, 0.0, 0.0};
    // row side: the tiles (b, s), s = 0 .. nph
    for (int s0 = 0; s0 <= nph; s0 += UN) {
        double v[UN][3];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int s = (s0 + u <= nph) ? s0 + u : nph;            // clamped: loaded, not added
            const double *pt = pc + ((int64_t)(b * (nph + 1) + s) * 2) * 192;
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) v[u][ax] = pt[ax * 64];
        }
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            if (s0 + u > nph) break;
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) F[ax] = (s0 + u == 0) ? v[u][ax] : F[ax] + v[u][ax];
        }
    }
    // column side: at phase s the block's partner is row block (b - s) mod NBLK
    for (int s0 = 0; s0 <= nph; s0 += UN) {
        double v[UN][3];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int s = (s0 + u <= nph) ? s0 + u : nph;
            int bi = b - s; if (bi < 0) bi += nblk;
            const double *pt = pc + ((int64_t)(bi * (nph + 1) + s) * 2 + 1) * 192;
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) v[u][ax] = pt[ax * 64];
        }
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            if (s0 + u > nph) break;
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) G[ax] = G[ax] + v[u][ax];
        }
    }
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) f[ax] = F[ax] + G[ax];
}

__global__ void __launch_bounds__(256)
pairdist_tiles_grad_kernel(const double *part, double tau, const double *tau_chain, double *out,
                           int32_t n, int32_t nblk)
{
    const int bead = blockIdx.x * 256 + threadIdx.x;
    const int64_t c = blockIdx.y;
    if (bead >= n) return;
    double f[3];
    tiles_force(part, c, bead, nblk, f);
    store_scaled_force(out + c * 3 * (int64_t)n + 3 * bead, tau_chain ? tau_chain[c] : tau, f[0], f[1], f[2]);
}

// Force evaluation e of a trajectory: the kick (and, before the last one, the drift) of
// pairdist_leapfrog_ring_kernel's owner threads, on q and p in memory.
template <bool FMA>
__global__ void __launch_bounds__(256)
pairdist_tiles_update_kernel(const double *part, const PairLeapArgs a, const double *q_in, int32_t nblk, int32_t e)
{
    const int n = a.n_beads;
    const int bead = blockIdx.x * 256 + threadIdx.x;
    const int64_t c = blockIdx.y;
    if (bead >= n) return;
    double f[3];
    tiles_force(part, c, bead, nblk, f);
    const double tau = a.tau_chain ? a.tau_chain[c] : a.tau;
    const double dt = a.dt_chain ? a.dt_chain[c] : a.timestep;
    const double step = (e == 0 || e == a.nsteps) ? 0.5 * dt : dt;
    const int64_t o = c * 3 * (int64_t)n + 3 * bead;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        double q = q_in[o + ax], p = a.p[o + ax];
        pair_kick<FMA>(a, f[ax], q, p, tau, step, dt, e < a.nsteps);
        a.p[o + ax] = p;
        a.q[o + ax] = q;
    }
}

}  // namespace binf
