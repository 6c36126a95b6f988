// Dense HMC metric: the triangular matrix-vector twins of the leapfrog kernels and the two
// kernels of the windowed covariance warm-up -- streaming pooled co-moments per group, and the
// pooled covariance with its Cholesky factor.  Build-defined: the reference integrates with
// the identity mass only (binf/samplers/hmc.py:92-125).  gfx950, wave64.
//
// A metric M^-1 = L L^T (L lower triangular, [G x D x D] row-major, chain c reads L[c % G])
// is carried through the WHITENED momentum r ~ N(0, I), as the diagonal metric is
// (metric.hip): the draw, energy, accept and adaption kernels serve unchanged, kick and drift
// become
//     kick    t_i = sum_{j = i .. D-1} L[j][i] g_j      p_i <- p_i - d t_i
//     drift   v_i = sum_{j = 0 .. i}   L[i][j] p_j      q_i <- q_i + v_i d
// with d = dt_chain[c] or timestep (0.5 * d first for a half kick).
//
// The arithmetic is stated in include/binf_hip.h and restated in numpy by
// tests/dense_metric_ref.py: every dot product is ONE sequential chain in ascending j, the
// first term the rounded product alone, every later term t + L g with two roundings (EXACT)
// or fma(L, g, t) (FMA).  Products that are rounded separately rule the matrix pipe out; the
// kernels are VALU code.  No loop has a trip count that depends on data.
//
// The piece (LF_KICK / LF_DRIFT / LF_KICK_DRIFT) and the argument check are those of the
// element-wise kernel (leapfrog_ew.hpp); the launcher adds its D limit.
#include "leapfrog_ew.hpp"
#include "diag_core.hpp"

namespace binf {

// ---------------------------------------------------------------------------
// leapfrog pieces
//
// A workgroup of 256 threads owns CW whole chains of ONE group (chains g + m G, CW
// consecutive m), so that every element of L it loads serves CW chains.  A thread is a
// dimension i of an i-tile of NI = 64, 128 or 256 dimensions (the smallest that covers D, 256
// beyond) and one of S = 256 / NI chain slots; it carries R = CW / S chains in registers.
// The g row (kick) and the p row (drift; after a kick_drift's kick: the NEW p row, complete
// before the drift starts) of the CW chains are staged in LDS, CW * D <= DM_ROW doubles, and
// read as broadcasts.
//
//   kick   L[j][i], j = i .. D-1, is read from global memory: a wave reads 64 consecutive
//          columns of row j, coalesced.  Elements above the diagonal are never loaded: the 64
//          rows that cross the wave's own diagonal elements run under a per-lane predicate,
//          the rows below them without one, their loads issued eight rows ahead.
//   drift  L[i][j], j = 0 .. i, is the transposed access: the workgroup copies the
//          [NI x TJ] tile of rows i0 .. i0 + NI - 1 and columns j0 .. j0 + TJ - 1 into LDS
//          with row-contiguous loads (below and on the diagonal only) and a thread reads its
//          own row of it.  The tile's row stride is TJ + 1 doubles: odd, so the 32 lanes of a
//          ds_read_b64 group sit on 32 different bank pairs (TJ alone, a power of two, would
//          be a TJ-way conflict); the row reads of the p row are broadcasts and never
//          conflict.  TJ = DM_TILE / NI: 32, 16 or 8.
// ---------------------------------------------------------------------------
constexpr int DM_THREADS = 256;
constexpr int DM_ROW = 2048;        // doubles of a staged row set: CW * D <= DM_ROW
constexpr int DM_TILE = 2048;       // NI * TJ
constexpr int DM_R = 4;             // chains a thread carries at most
constexpr int DM_MAX_D = 1024;

struct DenseArgs {
    double *q;
    double *p;
    const double *g;
    const double *chol;
    const double *dt_chain;
    double timestep;
    int64_t G, Cg, nblk, nwork;     // groups, chains per group, chain blocks per group, G * nblk
    int32_t D, CW, R, ni_shift, tj_shift, half;
};

template <int KIND, bool FMA>
__global__ void __launch_bounds__(DM_THREADS) dense_leapfrog_kernel(const DenseArgs a)
{
    __shared__ double grow[DM_ROW];                       // gradient rows   [CW][D]
    __shared__ double prow[DM_ROW];                       // momentum rows   [CW][D]
    __shared__ double tile[DM_TILE + DM_THREADS];         // [NI][TJ + 1]
    const int tid = threadIdx.x;
    const int D = a.D, NI = 1 << a.ni_shift, TJ = 1 << a.tj_shift, TS = TJ + 1;
    const int il = tid & (NI - 1), slot = tid >> a.ni_shift;
    const int wbase = il & ~63;                           // first dimension of this wave in the tile

    for (int64_t w = blockIdx.x; w < a.nwork; w += gridDim.x) {
        const int64_t g = w / a.nblk;
        const int64_t m0 = (w - g * a.nblk) * a.CW;
        const double *L = a.chol + g * (int64_t)D * D;

        // stage the rows of the CW chains (zeros for chains beyond the group's last)
        for (int idx = tid; idx < a.CW * D; idx += DM_THREADS) {
            const int k = idx / D, j = idx - k * D;
            const int64_t m = m0 + k;
            double v = 0.0;
            if (m < a.Cg) {
                const int64_t e = (g + m * a.G) * D + j;
                v = KIND == LF_DRIFT ? a.p[e] : a.g[e];
            }
            if (KIND == LF_DRIFT) prow[idx] = v;
            else                  grow[idx] = v;
        }
        bool live[DM_R];
        int64_t base[DM_R];                               // first element of the chain's row
        double d[DM_R];
        int rowk[DM_R];                                   // the chain's staged row (an unused r repeats the
                                                          // slot's first: summed and dropped, so that the
                                                          // loops below unroll without exits)
#pragma unroll
        for (int r = 0; r < DM_R; ++r) {
            const int64_t m = m0 + slot * a.R + r;
            live[r] = r < a.R && m < a.Cg;
            rowk[r] = (slot * a.R + (r < a.R ? r : 0)) * D;
            const int64_t c = live[r] ? g + m * a.G : 0;
            base[r] = c * D;
            d[r] = live[r] ? (a.dt_chain ? a.dt_chain[c] : a.timestep) : 0.0;
            if (KIND == LF_KICK && a.half) d[r] = 0.5 * d[r];     // "0.5 * timestep" first
        }
        __syncthreads();

        if (KIND != LF_DRIFT) {
            for (int i0 = 0; i0 < D; i0 += NI) {
                const int i = i0 + il;
                const bool mine = i < D;
                const int ic = mine ? i : 0;              // a lane beyond D walks column 0 and is dropped
                double t[DM_R] = {0.0, 0.0, 0.0, 0.0};
                // the wave walks the rows from its first column's diagonal element down: the 64
                // rows that cross its lanes' diagonal elements under a per-lane predicate ...
                const int jw = i0 + wbase, jd = jw + 64 < D ? jw + 64 : D;
                for (int j0 = jw; j0 < jd; j0 += 4) {
                    double l[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int j = j0 + u;
                        // every lane loads (no branch around a load): where the row lies above the
                        // lane's diagonal element, or beyond D, that element or the last row instead
                        int jr = j > ic ? j : ic;
                        jr = jr < D ? jr : D - 1;
                        l[u] = L[(int64_t)jr * D + ic];
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int j = j0 + u;
                        if (j < jd) {
#pragma unroll
                            for (int r = 0; r < DM_R; ++r) {
                                const double gj = grow[rowk[r] + j];
                                const double prod = l[u] * gj;
                                const double next = FMA ? __builtin_fma(l[u], gj, t[r]) : t[r] + prod;
                                t[r] = j > i ? next : (j == i ? prod : t[r]);
                            }
                        }
                    }
                }
                // ... the rows below them for every lane alike, eight loads ahead of their use
                // (a row beyond D is clamped to the last one and not used)
                auto rows8 = [&](double (&l)[8], int j0) {
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int j = j0 + u < D ? j0 + u : D - 1;
                        l[u] = L[(int64_t)j * D + ic];
                    }
                };
                double ahead[8];
                if (jd < D) rows8(ahead, jd);
                for (int j0 = jd; j0 < D; j0 += 8) {
                    double l[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) l[u] = ahead[u];
                    if (j0 + 8 < D) rows8(ahead, j0 + 8);
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int j = j0 + u;
                        if (j < D) {
#pragma unroll
                            for (int r = 0; r < DM_R; ++r) {
                                const double gj = grow[rowk[r] + j];
                                t[r] = FMA ? __builtin_fma(l[u], gj, t[r]) : t[r] + l[u] * gj;
                            }
                        }
                    }
                }
#pragma unroll
                for (int r = 0; r < DM_R; ++r) {
                    if (!mine || r >= a.R) continue;
                    double pn = 0.0;
                    if (live[r]) {
                        const double p0 = a.p[base[r] + i];
                        pn = FMA ? __builtin_fma(-d[r], t[r], p0) : p0 - d[r] * t[r];
                        a.p[base[r] + i] = pn;
                    }
                    if (KIND == LF_KICK_DRIFT) prow[(slot * a.R + r) * D + i] = pn;
                }
            }
            if (KIND == LF_KICK_DRIFT) __syncthreads();   // the new p rows are complete
        }

        if (KIND != LF_KICK) {
            for (int i0 = 0; i0 < D; i0 += NI) {
                const int i = i0 + il;
                const bool mine = i < D;
                const int jend = i0 + NI < D ? i0 + NI : D;       // columns 0 .. jend - 1 feed this tile
                double v[DM_R] = {0.0, 0.0, 0.0, 0.0};
                for (int j0 = 0; j0 < jend; j0 += TJ) {
                    for (int idx = tid; idx < NI * TJ; idx += DM_THREADS) {
                        const int rr = idx >> a.tj_shift, jj = idx & (TJ - 1);
                        // rows beyond D repeat the last one, columns beyond the diagonal the diagonal
                        // element: loaded without a branch, never used, nothing above the diagonal read
                        const int ti = i0 + rr < D ? i0 + rr : D - 1;
                        const int tj = j0 + jj < ti ? j0 + jj : ti;
                        tile[rr * TS + jj] = L[(int64_t)ti * D + tj];
                    }
                    __syncthreads();
                    if (j0 > 0 && j0 + TJ - 1 <= i0 + wbase && i0 + wbase < D) {
                        // the whole tile lies on or below the diagonal for every lane of this wave:
                        // no predicate (a lane beyond D sums stale tile rows and is dropped)
#pragma unroll 8
                        for (int jj = 0; jj < TJ; ++jj) {
                            const double l = tile[il * TS + jj];
#pragma unroll
                            for (int r = 0; r < DM_R; ++r) {
                                    const double pj = prow[rowk[r] + j0 + jj];
                                v[r] = FMA ? __builtin_fma(l, pj, v[r]) : v[r] + l * pj;
                            }
                        }
                    } else if (mine) {
                        for (int jj = 0; jj < TJ; ++jj) {
                            const int j = j0 + jj;
                            if (j > i) break;
                            const double l = tile[il * TS + jj];
#pragma unroll
                            for (int r = 0; r < DM_R; ++r) {
                                    const double pj = prow[rowk[r] + j];
                                const double prod = l * pj;
                                const double next = FMA ? __builtin_fma(l, pj, v[r]) : v[r] + prod;
                                v[r] = j == 0 ? prod : next;
                            }
                        }
                    }
                    __syncthreads();
                }
#pragma unroll
                for (int r = 0; r < DM_R; ++r) {
                    if (!mine || !live[r]) continue;
                    const double q0 = a.q[base[r] + i];
                    a.q[base[r] + i] = FMA ? __builtin_fma(v[r], d[r], q0) : q0 + v[r] * d[r];
                }
            }
        }
        __syncthreads();                                  // the staged rows are free again
    }
}

template <int KIND>
static int32_t dense_launch(double *q, double *p, const double *g, const double *chol, int64_t G,
                            double timestep, const double *dt_chain, int32_t half, int64_t C, int64_t D,
                            int32_t mode, void *stream, const char *what)
{
    int32_t rc = leapfrog_check_sizes(G, C, D, mode, what);
    if (rc != 0 || C == 0 || D == 0) return rc;
    if (D > DM_MAX_D)
        return fail(BINF_E_UNSUPPORTED, "%s: D = %lld beyond %d (a workgroup holds a chain's row in LDS)", what,
                    (long long)D, DM_MAX_D);
    rc = leapfrog_check<KIND>(q, p, g, chol, G, D * D, "factor", dt_chain, C, D, what);
    if (rc != 0) return rc;
    DenseArgs a;
    a.q = q; a.p = p; a.g = g; a.chol = chol; a.dt_chain = dt_chain; a.timestep = timestep;
    a.G = G; a.Cg = C / G; a.D = (int32_t)D; a.half = half ? 1 : 0;
    a.ni_shift = D <= 64 ? 6 : (D <= 128 ? 7 : 8);
    a.tj_shift = 11 - a.ni_shift;                        // NI * TJ == DM_TILE
    const int S = DM_THREADS >> a.ni_shift;
    int cw = S * DM_R;
    if (cw > DM_ROW / (int)D) cw = DM_ROW / (int)D;      // >= 2: D <= 1024; a multiple of S: S > 1 only for D <= 128
    a.CW = cw;
    a.R = cw / S;
    a.nblk = (a.Cg + cw - 1) / cw;
    a.nwork = G * a.nblk;
    const int64_t blocks = a.nwork < (1 << 20) ? a.nwork : (1 << 20);     // work-stride beyond
    const dim3 grid((unsigned)blocks);
    hipStream_t st = (hipStream_t)stream;
    if (mode == BINF_MODE_FMA) dense_leapfrog_kernel<KIND, true><<<grid, DM_THREADS, 0, st>>>(a);
    else                       dense_leapfrog_kernel<KIND, false><<<grid, DM_THREADS, 0, st>>>(a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what);
    return 0;
}

// ---------------------------------------------------------------------------
// streaming pooled co-moments: k0, s1 [G x D], s2 [G x D x D] (lower triangle)
//
// One kernel serves both sums.  A workgroup owns one group g and 64 entries -- an 8 x 8 tile
// (i, j) of s2 at or below the diagonal, or 64 dimensions of s1 -- lanes along the entries,
// wave w the chain block b0 + w of the group (64 consecutive chains of the group, sequential
// from 0.0); wave 0 then adds the block sums in block order to its running total.  The order
// is the diagnostics': a function of C / G only.  With `first` the shift k0[g] is read from
// x[chain g] and the launch for s1 (which runs second) stores it.
// ---------------------------------------------------------------------------
constexpr int CM_WAVES = 8;

struct ComomentArgs {
    const double *x;
    double *k0, *s1, *s2;
    int64_t C, D, G, Cg, nt;        // nt: 8-wide tiles along a dimension (pairs), 64-wide (sums)
    int32_t first;
};

template <bool PAIRS>
__global__ void __launch_bounds__(64 * CM_WAVES) comoments_kernel(const ComomentArgs a)
{
    __shared__ double sm[CM_WAVES][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t per = PAIRS ? a.nt * (a.nt + 1) / 2 : a.nt;
    const int64_t g = (int64_t)blockIdx.x / per;
    int64_t t = (int64_t)blockIdx.x - g * per;
    int64_t i, j;
    if (PAIRS) {
        // tile t of the lower triangle, row by row: (ti, tj), tj <= ti
        int64_t ti = 0;
        while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;                // at most nt steps: sizes only
        const int64_t tj = t - ti * (ti + 1) / 2;
        i = ti * 8 + (lane >> 3);
        j = tj * 8 + (lane & 7);
    } else {
        i = t * 64 + lane;
        j = 0;
    }
    const bool valid = i < a.D && (!PAIRS || j <= i);
    const int64_t nb = (a.Cg + DIAG_CHAIN_BLOCK - 1) / DIAG_CHAIN_BLOCK;
    const double *k0 = a.first ? a.x + g * a.D : a.k0 + g * a.D;   // first: the group's first chain
    double ki = 0.0, kj = 0.0;
    if (valid) {
        ki = k0[i];
        if (PAIRS) kj = k0[j];
    }
    double tot = 0.0;
    for (int64_t b0 = 0; b0 < nb; b0 += CM_WAVES) {
        const int64_t b = b0 + w;
        double s = 0.0;
        if (valid && b < nb) {
            const int64_t left = a.Cg - b * DIAG_CHAIN_BLOCK;
            const int cnt = left < DIAG_CHAIN_BLOCK ? (int)left : DIAG_CHAIN_BLOCK;
            const double *row = a.x + (g + b * DIAG_CHAIN_BLOCK * a.G) * a.D;
            const int64_t stride = a.G * a.D;
#pragma unroll 8
            for (int q = 0; q < cnt; ++q) {
                const double di = row[q * stride + i] - ki;
                if (PAIRS) {
                    const double dj = row[q * stride + j] - kj;
                    s = s + di * dj;
                } else {
                    s = s + di;
                }
            }
        }
        sm[w][lane] = s;
        __syncthreads();
        if (w == 0)
            for (int u = 0; u < CM_WAVES && b0 + u < nb; ++u) tot = tot + sm[u][lane];
        __syncthreads();
    }
    if (w != 0 || !valid) return;
    if (PAIRS) {
        double *o = a.s2 + (g * a.D + i) * a.D + j;
        *o = (a.first ? 0.0 : *o) + tot;
    } else {
        double *o = a.s1 + g * a.D + i;
        *o = (a.first ? 0.0 : *o) + tot;
        if (a.first) a.k0[g * a.D + i] = ki;
    }
}

// ---------------------------------------------------------------------------
// pooled covariance -> lower Cholesky factor: one workgroup per group
//
// The covariance goes into work[g] (lower triangle; +0.0 above) and is factorised in place,
// right-looking: at step k the column below the pivot is divided by sqrt(pivot) (and kept in
// LDS), then every entry (i, j), k < j <= i, loses L_ik * L_jk -- for one entry the
// subtractions come in ascending k, each product rounded first: the bits of the
// column-by-column statement in the header.  D steps of two barriers, whatever the data; a
// pivot that is not a positive finite number or an entry that is not finite raises the
// group's flag, and the group's chol is then left as it was.
// ---------------------------------------------------------------------------
constexpr int CF_THREADS = 1024;

struct FactorArgs {
    const double *s1, *s2;
    double *chol, *work;
    int32_t *status;
    double N;
    int32_t D, regularise;
};

__global__ void __launch_bounds__(CF_THREADS) factor_kernel(const FactorArgs a)
{
    __shared__ double col[DM_MAX_D];
    __shared__ int bad_any;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, NW = CF_THREADS / 64;
    const int D = a.D;
    const int64_t g = blockIdx.x;
    const double *s1 = a.s1 + g * D, *s2 = a.s2 + g * (int64_t)D * D;
    double *A = a.work + g * (int64_t)D * D, *out = a.chol + g * (int64_t)D * D;
    const double N = a.N;
    const double shrink = N / (N + 5.0), floor_ = 1e-3 * (5.0 / (N + 5.0));     // Stan's shrinkage
    if (tid == 0) bad_any = 0;
    for (int i = wv; i < D; i += NW) {
        const double si = s1[i];
        for (int j = lane; j < D; j += 64) {
            double c = 0.0;
            if (j <= i) {
                c = (s2[(int64_t)i * D + j] - (si * s1[j]) / N) / (N - 1.0);
                if (a.regularise) {
                    c = shrink * c;
                    if (j == i) c = c + floor_;
                }
            }
            A[(int64_t)i * D + j] = c;
        }
    }
    __syncthreads();
    int bad = 0;
    for (int k = 0; k < D; ++k) {
        const double piv = A[(int64_t)k * D + k];
        if (!(piv > 0.0 && piv <= 1.7976931348623157e308)) bad = 1;
        const double lkk = sqrt(piv);
        for (int i = k + 1 + tid; i < D; i += CF_THREADS) {
            const double v = A[(int64_t)i * D + k] / lkk;
            A[(int64_t)i * D + k] = v;
            col[i] = v;
        }
        __syncthreads();
        if (tid == 0) A[(int64_t)k * D + k] = lkk;        // nobody reads the pivot again
        for (int i = k + 1 + wv; i < D; i += NW) {
            const double lik = col[i];
            for (int j = k + 1 + lane; j <= i; j += 64) {
                const int64_t e = (int64_t)i * D + j;
                A[e] = A[e] - lik * col[j];
            }
        }
        __syncthreads();
    }
    for (int i = wv; i < D; i += NW)
        for (int j = lane; j <= i; j += 64) {
            const double v = A[(int64_t)i * D + j];
            if (!(v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308)) bad = 1;
        }
    if (bad) bad_any = 1;                                 // every writer stores the same value
    __syncthreads();
    const int failed = bad_any;
    if (tid == 0 && a.status) a.status[g] = failed;
    if (failed) return;
    for (int i = wv; i < D; i += NW)
        for (int j = lane; j < D; j += 64) out[(int64_t)i * D + j] = A[(int64_t)i * D + j];     // +0.0 above
}

}  // namespace binf

using namespace binf;

extern "C" int32_t binf_leapfrog_kick_dense_f64(double *p, const double *grad, const double *chol,
                                                int64_t G, double timestep, const double *dt_chain,
                                                int32_t half, int64_t C, int64_t D, int32_t mode,
                                                void *stream)
{
    return dense_launch<LF_KICK>(nullptr, p, grad, chol, G, timestep, dt_chain, half, C, D, mode, stream,
                                 "leapfrog_kick_dense");
}

extern "C" int32_t binf_leapfrog_drift_dense_f64(double *q, const double *p, const double *chol,
                                                 int64_t G, double timestep, const double *dt_chain,
                                                 int64_t C, int64_t D, int32_t mode, void *stream)
{
    return dense_launch<LF_DRIFT>(q, const_cast<double *>(p), nullptr, chol, G, timestep, dt_chain, 0, C, D,
                                  mode, stream, "leapfrog_drift_dense");
}

extern "C" int32_t binf_leapfrog_kick_drift_dense_f64(double *q, double *p, const double *grad,
                                                      const double *chol, int64_t G, double timestep,
                                                      const double *dt_chain, int64_t C, int64_t D,
                                                      int32_t mode, void *stream)
{
    return dense_launch<LF_KICK_DRIFT>(q, p, grad, chol, G, timestep, dt_chain, 0, C, D, mode, stream,
                                       "leapfrog_kick_drift_dense");
}

extern "C" int32_t binf_metric_comoments_f64(const double *x, double *k0, double *s1, double *s2,
                                             int32_t first, int64_t C, int64_t D, int64_t G, void *stream)
{
    const char *what = "metric_comoments";
    if (C < 0 || D < 0) return fail(BINF_E_ARG, "%s: negative size", what);
    if (G < 1) return fail(BINF_E_ARG, "%s: G >= 1 required, got %lld", what, (long long)G);
    if (C % G != 0)
        return fail(BINF_E_ARG, "%s: C = %lld is not a multiple of G = %lld", what, (long long)C, (long long)G);
    if (C == 0 || D == 0) return 0;
    if (D > DM_MAX_D) return fail(BINF_E_UNSUPPORTED, "%s: D = %lld beyond %d", what, (long long)D, DM_MAX_D);
    if (C > 0x7fffffffffffffffLL / D) return fail(BINF_E_ARG, "%s: C*D overflows", what);
    if (G > 0x7fffffffffffffffLL / (D * D)) return fail(BINF_E_ARG, "%s: G*D*D overflows", what);
    if (!x || !k0 || !s1 || !s2) return fail(BINF_E_ARG, "%s: null buffer", what);
    const void *buf[4] = {x, k0, s1, s2};
    const int64_t len[4] = {C * D, G * D, G * D, G * D * D};
    for (int o = 0; o < 4; ++o)
        for (int q = o + 1; q < 4; ++q)
            if (overlap_f64(buf[o], len[o], buf[q], len[q]))
                return fail(BINF_E_ALIAS, "%s: x, k0, s1 and s2 must not overlap", what);
    ComomentArgs a;
    a.x = x; a.k0 = k0; a.s1 = s1; a.s2 = s2; a.C = C; a.D = D; a.G = G; a.Cg = C / G; a.first = first ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    a.nt = (D + 7) / 8;
    const int64_t pairs = G * (a.nt * (a.nt + 1) / 2), sums = G * ((D + 63) / 64);
    if (pairs > 0x7fffffffLL) return fail(BINF_E_UNSUPPORTED, "%s: G * D * D too large for one launch", what);
    // the pairs first: with `first` they read the shift from x, the sums' launch stores it
    comoments_kernel<true><<<dim3((unsigned)pairs), 64 * CM_WAVES, 0, st>>>(a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what);
    a.nt = (D + 63) / 64;
    comoments_kernel<false><<<dim3((unsigned)sums), 64 * CM_WAVES, 0, st>>>(a);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what);
    return 0;
}

extern "C" int32_t binf_metric_factor_f64(const double *s1, const double *s2, int64_t n, int64_t C,
                                          int64_t D, int64_t G, int32_t regularise, double *chol,
                                          double *work, int32_t *status, void *stream)
{
    const char *what = "metric_factor";
    if (C < 0 || D < 0) return fail(BINF_E_ARG, "%s: negative size", what);
    if (n < 1) return fail(BINF_E_ARG, "%s: n >= 1 draws required, got %lld", what, (long long)n);
    if (G < 1) return fail(BINF_E_ARG, "%s: G >= 1 required, got %lld", what, (long long)G);
    if (C % G != 0)
        return fail(BINF_E_ARG, "%s: C = %lld is not a multiple of G = %lld", what, (long long)C, (long long)G);
    if (C == 0 || D == 0) return 0;
    if (D > DM_MAX_D)
        return fail(BINF_E_UNSUPPORTED, "%s: D = %lld beyond %d (one workgroup factorises a group)", what,
                    (long long)D, DM_MAX_D);
    if (G > 0x7fffffffLL) return fail(BINF_E_UNSUPPORTED, "%s: G too large for one launch", what);
    if (!s1 || !s2 || !chol || !work) return fail(BINF_E_ARG, "%s: null buffer", what);
    if (n > ((int64_t)1 << 53) / (C / G))
        return fail(BINF_E_UNSUPPORTED, "%s: n * C / G beyond 2^53", what);
    if (n * (C / G) < 2)
        return fail(BINF_E_ARG, "%s: N = n * C / G >= 2 draws required, got %lld", what, (long long)(n * (C / G)));
    const int64_t nv = G * D, nm = G * D * D;
    if (overlap_f64(chol, nm, s1, nv) || overlap_f64(chol, nm, s2, nm) || overlap_f64(work, nm, s1, nv) ||
        overlap_f64(work, nm, s2, nm) || overlap_f64(chol, nm, work, nm))
        return fail(BINF_E_ALIAS, "%s: chol and work must overlap neither the moments nor each other", what);
    if (status && (overlap_f64(status, (G + 1) / 2, chol, nm) || overlap_f64(status, (G + 1) / 2, work, nm)))
        return fail(BINF_E_ALIAS, "%s: status overlaps a buffer that is written", what);
    FactorArgs a;
    a.s1 = s1; a.s2 = s2; a.chol = chol; a.work = work; a.status = status;
    a.N = (double)(n * (C / G)); a.D = (int32_t)D; a.regularise = regularise ? 1 : 0;
    factor_kernel<<<dim3((unsigned)G), CF_THREADS, 0, (hipStream_t)stream>>>(a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what);
    return 0;
}
