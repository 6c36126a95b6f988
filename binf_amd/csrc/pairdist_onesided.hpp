// Pair-distance model, force scheme "one-sided": all-pairs loops, every lane the pairs of
// ITS bead, the chain's coordinates staged in LDS, target distances read from a symmetric
// [n x n] matrix.  The only scheme for fewer than 32 beads and for unpacked targets above
// 256 beads.  Included by pairdist.hip alone, after pairdist_force.hpp.
#pragma once
#include "pairdist_force.hpp"

namespace binf {

// Restraint force on bead i summed by FOUR adjacent lanes: lane quarter qt adds
// the pairs j in [qt*ceil(n/4), (qt+1)*ceil(n/4)) in ascending order, the four
// partial sums are joined as (f0 + f1) + (f2 + f3) by xor-shuffles 1 and 2 (all
// four lanes end up with the total).  With one lane per bead a 256-bead chain
// is one wave per SIMD and the loop is latency-bound; four lanes per bead give
// the scheduler four waves per SIMD.  sx: LDS copy of the chain's coordinates.
// Must be called by all lanes of the wave (shuffles).
__device__ inline void quartered_force(const double *sx, const double *ymat, int n, int i,
                                       bool valid, int qt, double x0, double x1, double x2,
                                       double &f0, double &f1, double &f2)
{
    const int per = (n + 3) >> 2;
    const int jb = qt * per;
    int je = jb + per;
    if (je > n) je = n;
    f0 = 0.0; f1 = 0.0; f2 = 0.0;
    if (valid) {
        for (int j = jb; j < je; ++j) {
            if (j == i) continue;
            const double d0 = x0 - sx[3 * j];
            const double d1 = x1 - sx[3 * j + 1];
            const double d2 = x2 - sx[3 * j + 2];
            const double w = pair_weight(d0, d1, d2, ymat[(int64_t)j * n + i]);
            f0 += w * d0;
            f1 += w * d1;
            f2 += w * d2;
        }
    }
    f0 = f0 + __shfl_xor(f0, 1, 64); f0 = f0 + __shfl_xor(f0, 2, 64);
    f1 = f1 + __shfl_xor(f1, 1, 64); f1 = f1 + __shfl_xor(f1, 2, 64);
    f2 = f2 + __shfl_xor(f2, 1, 64); f2 = f2 + __shfl_xor(f2, 2, 64);
}

// The same sum by ONE lane: four quarter accumulators advanced in lock-step
// (four independent chains of FMAs for the scheduler), joined in the same
// order -- bit-identical to quartered_force, so which variant a launch uses is
// a pure performance choice (many chains: one lane per bead; few: four).
__device__ inline void quartered_force_1lane(const double *sx, const double *ymat, int n, int i,
                                             double x0, double x1, double x2,
                                             double &f0, double &f1, double &f2)
{
    const int per = (n + 3) >> 2;
    double g[4][3];
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) { g[qt][0] = 0.0; g[qt][1] = 0.0; g[qt][2] = 0.0; }
    for (int jj = 0; jj < per; ++jj) {
#pragma unroll
        for (int qt = 0; qt < 4; ++qt) {
            const int j = qt * per + jj;
            if (j < n && j != i) {
                const double d0 = x0 - sx[3 * j];
                const double d1 = x1 - sx[3 * j + 1];
                const double d2 = x2 - sx[3 * j + 2];
                const double w = pair_weight(d0, d1, d2, ymat[(int64_t)j * n + i]);
                g[qt][0] += w * d0;
                g[qt][1] += w * d1;
                g[qt][2] += w * d2;
            }
        }
    }
    f0 = (g[0][0] + g[1][0]) + (g[2][0] + g[3][0]);
    f1 = (g[0][1] + g[1][1]) + (g[2][1] + g[3][1]);
    f2 = (g[0][2] + g[1][2]) + (g[2][2] + g[3][2]);
}

// n_beads <= 1024, a workgroup of 256 LANES threads per chain.  LANES = 1: one lane per bead;
// LANES = 4: thread = (bead tile slot, quarter)
template <int LANES>
__global__ void __launch_bounds__(256 * LANES)
pairdist_grad_lanes_kernel(const double *x, const double *ymat, double tau,
                           const double *tau_chain, double *out, int32_t n_beads)
{
    extern __shared__ double sx[];
    const int n = n_beads;
    const int64_t c = blockIdx.x;
    const double *xc = x + c * 3 * (int64_t)n;
    const double t = tau_chain ? tau_chain[c] : tau;
    for (int k = threadIdx.x; k < 3 * n; k += 256 * LANES) sx[k] = xc[k];
    __syncthreads();
    if constexpr (LANES == 1) {
        for (int i = threadIdx.x; i < n; i += 256) {
            double f0, f1, f2;
            quartered_force_1lane(sx, ymat, n, i, sx[3 * i], sx[3 * i + 1], sx[3 * i + 2], f0, f1, f2);
            store_scaled_force(out + c * 3 * (int64_t)n + 3 * i, t, f0, f1, f2);
        }
    } else {
        const int qt = threadIdx.x & 3;
        for (int i0 = 0; i0 < n; i0 += 256) {
            const int i = i0 + (threadIdx.x >> 2);
            const bool iv = i < n;
            const double x0 = iv ? sx[3 * i] : 0.0, x1 = iv ? sx[3 * i + 1] : 0.0,
                         x2 = iv ? sx[3 * i + 2] : 0.0;
            double f0, f1, f2;
            quartered_force(sx, ymat, n, i, iv, qt, x0, x1, x2, f0, f1, f2);
            if (iv && qt == 0) store_scaled_force(out + c * 3 * (int64_t)n + 3 * i, t, f0, f1, f2);
        }
    }
}

// n_beads > 1024: one lane per bead, coordinates staged tile by tile.
// out[c, 3i + a] = tau_c * sum_{j != i} (d_ij - y[j][i]) * (x_i - x_j)[a] / d_ij
// ymat: symmetric [n x n] target distances (diagonal ignored).
template <int TILE>
__global__ void __launch_bounds__(256)
pairdist_grad_kernel(const double *x, const double *ymat, double tau,
                     const double *tau_chain, double *out, int32_t n_beads)
{
    __shared__ double sx[TILE][3];
    const int64_t c = blockIdx.x;
    const double *xc = x + c * 3 * (int64_t)n_beads;
    const double t = tau_chain ? tau_chain[c] : tau;
    for (int i0 = 0; i0 < n_beads; i0 += 256) {
        const int i = i0 + threadIdx.x;
        const bool iv = i < n_beads;
        double xi0 = 0, xi1 = 0, xi2 = 0;
        if (iv) { xi0 = xc[3 * i]; xi1 = xc[3 * i + 1]; xi2 = xc[3 * i + 2]; }
        double f0 = 0.0, f1 = 0.0, f2 = 0.0;
        for (int j0 = 0; j0 < n_beads; j0 += TILE) {
            __syncthreads();
            for (int k = threadIdx.x; k < TILE * 3; k += 256) {
                const int idx = 3 * j0 + k;
                (&sx[0][0])[k] = (idx < 3 * n_beads) ? xc[idx] : 0.0;
            }
            __syncthreads();
            const int jn = (n_beads - j0 < TILE) ? n_beads - j0 : TILE;
            if (iv) {
                for (int jj = 0; jj < jn; ++jj) {
                    const int j = j0 + jj;
                    if (j == i) continue;
                    const double a = xi0 - sx[jj][0];
                    const double b = xi1 - sx[jj][1];
                    const double e = xi2 - sx[jj][2];
                    const double w = pair_weight(a, b, e, ymat[(int64_t)j * n_beads + i]);
                    f0 += w * a;
                    f1 += w * b;
                    f2 += w * e;
                }
            }
        }
        if (iv) store_scaled_force(out + c * 3 * (int64_t)n_beads + 3 * i, t, f0, f1, f2);
    }
}

// ---------------------------------------------------------------------------
// Fused leapfrog for the restraint posterior: the whole _leapfrog() of
// binf/samplers/hmc.py:92-125 in one launch, one 1024-thread workgroup per chain.
// Four adjacent lanes share a bead (slot, slot + 256, ...; position and momentum
// in registers, identical in the four lanes); every bead position is mirrored in
// LDS for the all-pairs force loop.  The force is evaluated exactly like
// pairdist_grad_lanes_kernel (quartered_force) and the gradient is assembled like the
// Posterior does (pair_grad1, pairdist_force.hpp), so the result is bit-identical to the
// per-step generic tier.
// ---------------------------------------------------------------------------
template <int NB, bool FMA, int LANES>
__global__ void __launch_bounds__(256 * LANES) pairdist_leapfrog_kernel(const PairLeapArgs a)
{
    extern __shared__ double sx[];               // [n_beads][3]
    const int n = a.n_beads;
    const int64_t c = blockIdx.x;
    // (not pair_chain(): through it the one-lane instantiations take two more SGPRs)
    double *qc = a.q + c * 3 * (int64_t)n;
    const double *qs = (a.q_from ? a.q_from : a.q) + c * 3 * (int64_t)n;
    double *pc = a.p + c * 3 * (int64_t)n;
    const double tau = a.tau_chain ? a.tau_chain[c] : a.tau;
    const double dt = a.dt_chain ? a.dt_chain[c] : a.timestep;
    const double hdt = 0.5 * dt;
    const int qt = (LANES == 4) ? (threadIdx.x & 3) : 0;              // quarter of the j-range
    const int slot = (LANES == 4) ? (threadIdx.x >> 2) : threadIdx.x;  // bead inside a tile of 256

    // the four lanes of a bead hold identical copies of its position / momentum.  Four
    // tiles of beads with four lanes each (769 .. 1024 beads, a 1024-thread workgroup:
    // 128 VGPRs) do not fit q AND p in registers -- 28 bytes per lane went to scratch --
    // so there the momentum lives in LDS behind the positions: every lane of a bead
    // writes the same value to the same slot and reads it back itself.
    constexpr bool PLDS = (NB == 4 && LANES == 4);
    double *sp = sx + 3 * n;                     // [n_beads][3], PLDS only
    double q[NB][3], p[PLDS ? 1 : NB][3];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int i = slot + 256 * b;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            q[b][ax] = (i < n) ? qs[3 * i + ax] : 0.0;
            const double pv = (i < n) ? pc[3 * i + ax] : 0.0;
            if (PLDS) { if (i < n) sp[3 * i + ax] = pv; }
            else p[b][ax] = pv;
        }
    }
    auto get_p = [&](int b, int ax) -> double {
        const int i = slot + 256 * b;
        return PLDS ? ((i < n) ? sp[3 * i + ax] : 0.0) : p[PLDS ? 0 : b][ax];
    };
    auto set_p = [&](int b, int ax, double v) {
        const int i = slot + 256 * b;
        if (PLDS) { if (i < n) sp[3 * i + ax] = v; }
        else p[PLDS ? 0 : b][ax] = v;
    };
    auto publish = [&]() {
        __syncthreads();
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const int i = slot + 256 * b;
            if (i < n && qt == 0) {
                sx[3 * i] = q[b][0];
                sx[3 * i + 1] = q[b][1];
                sx[3 * i + 2] = q[b][2];
            }
        }
        __syncthreads();
    };
    // p -= step * gradient(q)
    auto kick = [&](double step) {
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const int i = slot + 256 * b;
            double f[3];
            if (LANES == 4) {
                quartered_force(sx, a.ymat, n, i, i < n, qt, q[b][0], q[b][1], q[b][2],
                                f[0], f[1], f[2]);
            } else {
                f[0] = f[1] = f[2] = 0.0;
                if (i < n)
                    quartered_force_1lane(sx, a.ymat, n, i, q[b][0], q[b][1], q[b][2],
                                          f[0], f[1], f[2]);
            }
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                const double g = pair_grad1(a, f[ax], q[b][ax], tau);
                const double pv = get_p(b, ax);
                set_p(b, ax, pair_kick1<FMA>(g, pv, step));
            }
        }
    };
    auto drift = [&]() {
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int ax = 0; ax < 3; ++ax)
            {
                const double pv = get_p(b, ax);
                q[b][ax] = pair_drift1<FMA>(q[b][ax], pv, dt);
            }
    };

    publish();
    kick(hdt);                                        // hmc.py:116
    for (int s = 0; s < a.nsteps - 1; ++s) {             // hmc.py:118-120
        drift();
        publish();
        kick(dt);
    }
    drift();                                             // hmc.py:122-123
    publish();
    kick(hdt);

#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int i = slot + 256 * b;
        if (i < n && qt == 0) {
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                qc[3 * i + ax] = q[b][ax];
                pc[3 * i + ax] = get_p(b, ax);
            }
        }
    }
}

}  // namespace binf
