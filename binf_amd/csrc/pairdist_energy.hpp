// Pair-distance model, energy side (bit-identical to numpy: correctly rounded sqrt, np.sum's
// pairwise order):
//   pairdist_forward_kernel     the distances themselves;
//   pairdist_chi2_rows_kernel   chi^2 of one or two chains per workgroup, distances formed on
//                               the fly, with the per-chain two-entry memo of rowsum.hpp;
//   pairdist_chi2_chunk_kernel  chi^2 with few chains: every 8192-pair chunk a workgroup, the
//   pairdist_chi2_join_kernel   chunk sums joined in order by a second launch;
//   pairdist_energy_kernel      HMCSampler's E = 0.5 sum p^2 - log_prob for likelihood + one
//                               isotropic Gaussian prior in one launch (memo check included).
// Included by pairdist.hip alone.
#pragma once
#include "rowsum.hpp"

namespace binf {

// Correctly rounded sqrt of a squared distance.  The compiler's expansion of sqrt(double)
// is rsq + one coupled Goldschmidt step + two residual corrections, wrapped in a scaling
// of inputs below 2^-767 and a pass-through of 0 / inf (18 instructions, 8 of them that
// wrapping).  For an argument in [2^-767, inf) the wrapping does nothing: the same
// iteration without it gives the same bits; any other argument takes the library path.
__device__ inline double sqrt_rn(double s)
{
    const uint32_t hi = (uint32_t)__double2hiint(s);
    const bool plain = hi - 0x10000000u < 0x7ff00000u - 0x10000000u;
    const double r = __builtin_amdgcn_rsq(s);
    double g = s * r;
    double h = r * 0.5;
    const double e = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, e, g);
    h = __builtin_fma(h, e, h);
    double d = __builtin_fma(-g, g, s);
    g = __builtin_fma(d, h, g);
    d = __builtin_fma(-g, g, s);
    g = __builtin_fma(d, h, g);
    if (__builtin_expect(!plain, 0)) g = sqrt(s);
    return g;
}

// d[c, p] for p-th pair (I[p], J[p]); coordinates x[c, 3*bead + axis]
__global__ void __launch_bounds__(256)
pairdist_forward_kernel(const double *x, const int32_t *I, const int32_t *J,
                        double *out, int64_t n_beads, int64_t n_pairs)
{
    const int64_t c = blockIdx.y;
    const double *xc = x + c * 3 * n_beads;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n_pairs;
         p += (int64_t)gridDim.x * 256) {
        const int i = I[p], j = J[p];
        const double a = xc[3 * i] - xc[3 * j];
        const double b = xc[3 * i + 1] - xc[3 * j + 1];
        const double e = xc[3 * i + 2] - xc[3 * j + 2];
        // np.sum(diff**2, axis=1): sequential over the 3 components
        const double s = (a * a + b * b) + e * e;
        out[c * n_pairs + p] = sqrt_rn(s);
    }
}

// chi^2 of the restraints without the [C x n_pairs] distances ever reaching HBM:
// element p of the row reduction is (d_p - y_p)^2 with d_p computed on the fly,
// exactly as pairdist_forward_kernel + the error model's (mock - ys)**2 do.
struct PairArgs {
    const double *x;
    const int32_t *I;
    const int32_t *J;
    const double *ys;
    int64_t n_beads;
};

struct PairResid {
    const double *xc;
    const int32_t *I;
    const int32_t *J;
    const double *ys;
    __device__ inline double operator()(int p) const
    {
        const int i = I[p], j = J[p];
        const double a = xc[3 * i] - xc[3 * j];
        const double b = xc[3 * i + 1] - xc[3 * j + 1];
        const double e = xc[3 * i + 2] - xc[3 * j + 2];
        const double s = (a * a + b * b) + e * e;
        const double d = sqrt_rn(s) - ys[p];
        return d * d;
    }
};

struct PairResidMake {
    __device__ static inline PairResid make(const PairArgs &a, int64_t row)
    {
        PairResid f;
        f.xc = a.x + row * 3 * a.n_beads;
        f.I = a.I;
        f.J = a.J;
        f.ys = a.ys;
        return f;
    }
};

// ---- chi^2 of ROWS chains per workgroup: the pair list (I, J, y) is the same for every
// chain, so one pass over it serves ROWS chains -- the index / target loads and their
// address arithmetic are paid once, and each lane has 8 x ROWS independent square roots
// in flight.  With one chain per workgroup the list is streamed from L2 once per chain
// (16 bytes per pair and chain: 1 GB per evaluation at 2048 chains of 256 beads), which
// is what bounded the one-row kernel there.  Same tree, same order as
// row_reduce_block_kernel: the results are bit-identical to the one-row path.
// LDS: coordinates interleaved [3*bead + axis][row], so one bead's ROWS values of an axis
// are one 16- or 32-byte read.
template <int ROWS>
struct PairResidRows {
    const double *xl;
    const int32_t *I;
    const int32_t *J;
    const double *ys;
    __device__ inline void operator()(int p, double (&v)[ROWS]) const
    {
        const int i = 3 * ROWS * I[p], j = 3 * ROWS * J[p];
        const double y = ys[p];
        double xi[3][ROWS], xj[3][ROWS];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax)
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
                xi[ax][r] = xl[i + ax * ROWS + r];
                xj[ax][r] = xl[j + ax * ROWS + r];
            }
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const double a = xi[0][r] - xj[0][r];
            const double b = xi[1][r] - xj[1][r];
            const double e = xi[2][r] - xj[2][r];
            const double s = (a * a + b * b) + e * e;
            const double d = sqrt_rn(s) - y;
            v[r] = d * d;
        }
    }
};

// leaf_sum_f (rowsum.hpp) for ROWS rows at once; U element values per row in flight
template <int ROWS, int U, class F>
__device__ inline void leaf_sum_rows(const F &f, int off, int n, int lane, bool active,
                                     double (&res)[ROWS])
{
    const int j = lane & 7;
    const int T = (n >= 8) ? (n >> 3) : 0;
    const int rem = (n >= 8) ? (n & 7) : n;
    double r[ROWS];
#pragma unroll
    for (int q = 0; q < ROWS; ++q) r[q] = 0.0;
    if (active && T > 0) {
        int t = 0;
        for (; t + U <= T; t += U) {
            double v[U][ROWS];
#pragma unroll
            for (int u = 0; u < U; ++u) f(off + 8 * (t + u) + j, v[u]);
#pragma unroll
            for (int q = 0; q < ROWS; ++q) r[q] = (t == 0) ? v[0][q] : r[q] + v[0][q];
#pragma unroll
            for (int u = 1; u < U; ++u)
#pragma unroll
                for (int q = 0; q < ROWS; ++q) r[q] = r[q] + v[u][q];
        }
        for (; t < T; ++t) {
            double v[ROWS];
            f(off + 8 * t + j, v);
#pragma unroll
            for (int q = 0; q < ROWS; ++q) r[q] = (t == 0) ? v[q] : r[q] + v[q];
        }
    }
#pragma unroll
    for (int q = 0; q < ROWS; ++q) {
        const double s8 = sum8_f64(r[q]);
        res[q] = (T > 0) ? s8 : -0.0;
    }
    if (__any(rem != 0)) {
        double tail[ROWS];
#pragma unroll
        for (int q = 0; q < ROWS; ++q) tail[q] = 0.0;
        if (active && j < rem) f(off + 8 * T + j, tail);
        const int leafbase = lane & ~7;
#pragma unroll
        for (int i = 0; i < 7; ++i)
#pragma unroll
            for (int q = 0; q < ROWS; ++q) {
                const double v = shfl_f64(tail[q], leafbase + i);
                const double s = res[q] + v;
                res[q] = (i < rem) ? s : res[q];
            }
    }
}

// One np.sum-order reduction of D elements for ROWS rows by the whole workgroup;
// f(i, v[ROWS]) = element i of every row.  THREADS / 8 lane groups sum leaves: with 16
// waves a round covers two 64-leaf chunks at once, with 4 waves a chunk takes two passes.
// The leaf sums of a round go to LDS, ONE barrier, and wave 0 alone walks the round's trees
// with lane exchanges (lane = path) and adds the chunk sums to the running total in chunk
// order -- a tree through LDS costs two barriers per level, 14 per chunk, which at one
// 1024-thread workgroup per CU was a third of the kernel.  The LDS buffers alternate
// between rounds (`round` runs on through consecutive calls), so the barrier of round r + 1
// is all that separates wave 0's reads of round r from the writes of round r + 2.
// The totals come back in THREAD 0 only.
struct BlockSumScratch {
    double S[2][2][128];     // [round parity][row][slot]   (ROWS <= 2)
    int dep[2][128];
};

template <int ROWS, int U, int THREADS, class F>
__device__ inline void block_sum_rows(const F &f, int D, int H, BlockSumScratch &sc, int &round,
                                      double (&total)[ROWS])
{
    static_assert(ROWS <= 2, "BlockSumScratch holds two rows");
    constexpr int GROUPS = THREADS / 8;
    const int npaths = 1 << H;                                   // <= 128
    const int lane = threadIdx.x & 63;
    const int group = threadIdx.x >> 3;
    const int nchunks = D <= 0 ? 1 : (D + NPY_BUFSIZE - 1) / NPY_BUFSIZE;
    const int R = GROUPS >= npaths ? GROUPS / npaths : 1;        // chunks per round
    const int passes = GROUPS >= npaths ? 1 : (npaths + GROUPS - 1) / GROUPS;   // passes per chunk
#pragma unroll
    for (int q = 0; q < ROWS; ++q) total[q] = 0.0;
    for (int c0 = 0; c0 < nchunks; c0 += R, ++round) {
        const int b = round & 1;
        for (int ps = 0; ps < passes; ++ps) {
            const int item = ps * GROUPS + group;                // (chunk of the round, path)
            const int cr = item >> H, path = item & (npaths - 1);
            const int chunk = c0 + cr;
            const bool act = cr < R && chunk < nchunks && item < R * npaths;
            const int cbase = act ? chunk * NPY_BUFSIZE : 0;
            const int n = (D - cbase < NPY_BUFSIZE) ? D - cbase : NPY_BUFSIZE;
            const Leaf L = pairwise_leaf(n, H, act ? path : 0);
            double s[ROWS];
            leaf_sum_rows<ROWS, U>(f, cbase + L.off, L.len, lane, act, s);
            if (act && (lane & 7) == 0) {
#pragma unroll
                for (int q = 0; q < ROWS; ++q) sc.S[b][q][item] = s[q];
                sc.dep[b][item] = L.depth;
            }
        }
        __syncthreads();
        if (threadIdx.x < 64) {
            for (int cr = 0; cr < R && c0 + cr < nchunks; ++cr) {
                const int base = cr << H;
                const bool two = npaths > 64;                    // H = 7: paths p and p + 64 per lane
                const int p0 = base + (lane & (npaths - 1)), p1 = base + ((lane + 64) & (npaths - 1));
                const int d0 = sc.dep[b][p0], d1 = sc.dep[b][p1];
#pragma unroll
                for (int q = 0; q < ROWS; ++q) {
                    double v0 = sc.S[b][q][p0], v1 = sc.S[b][q][p1];
                    for (int l = 0; l < H && l < 6; ++l) {
                        const double o0 = shfl_f64(v0, lane ^ (1 << l));
                        v0 = (d0 >= H - l) ? v0 + o0 : v0;
                        if (two) {
                            const double o1 = shfl_f64(v1, lane ^ (1 << l));
                            v1 = (d1 >= H - l) ? v1 + o1 : v1;
                        }
                    }
                    if (two) v0 = (d0 >= 1) ? v0 + v1 : v0;      // level 6 joins paths p and p + 64
                    total[q] = total[q] + v0;                    // lane 0: path 0, the chunk's sum
                }
            }
        }
    }
}

template <int ROWS, int U, int THREADS>
__global__ void __launch_bounds__(THREADS)
pairdist_chi2_rows_kernel(const PairArgs a, const RowGeom g, double *out)
{
    __shared__ BlockSumScratch sc;
    int round = 0;
    extern __shared__ double row_lds[];
    const int64_t row0 = (int64_t)blockIdx.x * ROWS;
    int64_t rows[ROWS];                          // the last workgroup repeats the last chain
#pragma unroll
    for (int q = 0; q < ROWS; ++q) rows[q] = (row0 + q < g.C) ? row0 + q : g.C - 1;
    if (g.skip) {                                // workgroup-uniform
        bool all_skip = true;
#pragma unroll
        for (int q = 0; q < ROWS; ++q) all_skip = all_skip && g.skip[rows[q]] != 0;
        if (all_skip) {
            if (threadIdx.x < ROWS && row0 + threadIdx.x < g.C) {
                const int64_t row = row0 + threadIdx.x;
                out[row] = row_result(g, row, *row_memo_slot(g, row));
            }
            return;
        }
    }
    const int n3 = 3 * (int)a.n_beads;
#pragma unroll
    for (int q = 0; q < ROWS; ++q) {
        const double *xc = a.x + rows[q] * n3;
        for (int k = threadIdx.x; k < n3; k += THREADS) row_lds[k * ROWS + q] = xc[k];
    }
    __syncthreads();
    PairResidRows<ROWS> f;
    f.xl = row_lds; f.I = a.I; f.J = a.J; f.ys = a.ys;
    double total[ROWS];
    block_sum_rows<ROWS, U, THREADS>(f, g.D, g.H, sc, round, total);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < ROWS; ++q) {
            if (row0 + q >= g.C) break;
            if (g.memo_sum) *row_memo_slot(g, row0 + q) = total[q];
            out[row0 + q] = row_result(g, row0 + q, total[q]);
        }
    }
}

// ---- chi^2 with FEW chains: a workgroup per chain walks the whole pair list (0.3 ms at 1024
// beads, 1.2 ms at 2048, whatever the number of chains up to the number of CUs).  np.sum works
// in chunks of 8192 elements whose sums it adds one after the other, so the chunks are
// independent: here every (chunk, chain) is a workgroup, the chunk sums go to a workspace and a
// second launch adds them in order -- the same bits -- and applies the epilogue.  The
// coordinates are read through the caches (no LDS copy: any number of beads).
struct PairResidChunk {
    const double *xc;
    const int32_t *I;
    const int32_t *J;
    const double *ys;
    int64_t base;
    __device__ inline void operator()(int p, double (&v)[1]) const
    {
        const int64_t P = base + p;
        const int i = I[P], j = J[P];
        const double a = xc[3 * i] - xc[3 * j];
        const double b = xc[3 * i + 1] - xc[3 * j + 1];
        const double e = xc[3 * i + 2] - xc[3 * j + 2];
        const double s = (a * a + b * b) + e * e;
        const double d = sqrt_rn(s) - ys[P];
        v[0] = d * d;
    }
};

template <int U>
__global__ void __launch_bounds__(256)
pairdist_chi2_chunk_kernel(const PairArgs a, const RowGeom g, double *partial, int32_t nchunks)
{
    __shared__ BlockSumScratch sc;
    const int64_t c = blockIdx.y;
    const int k = blockIdx.x;
    if (g.skip && g.skip[c]) return;             // the memo holds this chain's sum (workgroup-uniform)
    int round = 0;
    PairResidChunk f;
    f.xc = a.x + c * 3 * a.n_beads; f.I = a.I; f.J = a.J; f.ys = a.ys;
    f.base = (int64_t)k * NPY_BUFSIZE;
    const int64_t left = (int64_t)g.D - f.base;
    const int len = left < NPY_BUFSIZE ? (int)left : NPY_BUFSIZE;
    double total[1];
    block_sum_rows<1, U, 256>(f, len, g.H, sc, round, total);    // 0.0 + this chunk's sum
    if (threadIdx.x == 0) partial[c * nchunks + k] = total[0];
}

// chunk sums in order, the memo, the epilogue; chi2_out (or null) receives the bare sums
__global__ void __launch_bounds__(256)
pairdist_chi2_join_kernel(const RowGeom g, const double *partial, int32_t nchunks, double *out, double *chi2_out)
{
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= g.C) return;
    double total;
    if (g.skip && g.skip[row]) {
        total = *row_memo_slot(g, row);
    } else {
        total = 0.0;                             // the reduction's identity
        const double *pr = partial + row * nchunks;
        int k = 0;
        for (; k + 8 <= nchunks; k += 8) {       // eight loads in flight, added in order
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = pr[k + u];
#pragma unroll
            for (int u = 0; u < 8; ++u) total = total + v[u];
        }
        for (; k < nchunks; ++k) total = total + pr[k];
        if (g.memo_sum) *row_memo_slot(g, row) = total;
    }
    if (chi2_out) chi2_out[row] = total;
    if (out) out[row] = row_result(g, row, total);
}

// ---- the energy of HMCSampler.sample() (hmc.py:143,148,150) for the restraint posterior in
// ONE launch:  E = 0.5 np.sum(p**2) - log_prob,  log_prob = the Posterior's sum of its
// components in their order (binf/pdf/posteriors.py:147-151): the restraint likelihood
// (-0.5 chi^2 tau + N/2 log tau) and at most one isotropic Gaussian prior
// ((-0.5 k) np.sum((x - x0)**2)).  The per-step tier spends six launches on it (prior row
// sum, memo check, chi^2, term sum, kinetic row sum with the subtraction as its epilogue);
// a workgroup has the chain's coordinates in LDS anyway, so the two short row sums, the
// memo check and the few scalar operations ride along.  Every sum in numpy's order and
// every scalar operation as the per-step tier does it: the same bits.
struct PairEnergyArgs {
    const double *x;         // [C][3n]
    const double *p;         // [C][3n]
    const int32_t *I;
    const int32_t *J;
    const double *ys;
    double *memo_x;          // [2][C][3n] or null (no memo)
    uint8_t *memo_state;     // [2][C]
    double *energy;          // [C]
    double *log_prob;        // [C] or null
    double prior_scale;      // -0.5 k
    double prior_x0;
    int32_t has_prior;
    int32_t n_terms;         // the Posterior's components in its order (<= 4):
    int32_t term_kind[4];    //   0 the prior, 1 the likelihood, 2 / 3 a constant of the move
    const double *extra[2];  // constants per chain [C], or null: extra_scalar
    double extra_scalar[2];
    int32_t n_beads;
    int32_t H_d;             // tree height of a 3n-element sum
    const double *chi2_in;   // [C] or null: the restraints' chi^2 already summed (few chains: by chunks)
};

template <int ROWS>
struct ShiftSqRows {         // (x - x0)**2 from the interleaved LDS copy
    const double *xl;
    double x0;
    __device__ inline void operator()(int i, double (&v)[ROWS]) const
    {
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const double d = xl[i * ROWS + r] - x0;
            v[r] = d * d;
        }
    }
};

template <int ROWS>
struct SqRows {              // p**2 from HBM
    const double *row[ROWS];
    __device__ inline void operator()(int i, double (&v)[ROWS]) const
    {
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const double x = row[r][i];
            v[r] = x * x;
        }
    }
};

template <int ROWS, int U, int THREADS>
__global__ void __launch_bounds__(THREADS)
pairdist_energy_kernel(const PairEnergyArgs a, const RowGeom g)
{
    __shared__ BlockSumScratch sc;
    __shared__ int differs[ROWS][2];
    int round = 0;
    extern __shared__ double row_lds[];
    const int64_t row0 = (int64_t)blockIdx.x * ROWS;
    int64_t rows[ROWS];                          // the last workgroup repeats the last chain
#pragma unroll
    for (int q = 0; q < ROWS; ++q) rows[q] = (row0 + q < g.C) ? row0 + q : g.C - 1;
    const int n3 = 3 * a.n_beads;
    const bool given = a.chi2_in != nullptr;     // then the memo was served by the launches before this one
    const bool memo = a.memo_x != nullptr && !given;
    if (threadIdx.x < 2 * ROWS) differs[threadIdx.x >> 1][threadIdx.x & 1] = 0;
    __syncthreads();
    // coordinates to LDS; on the way, compared BIT FOR BIT with the memo's two entries
    // (row_memo_check_kernel, rowsum.hpp)
#pragma unroll
    for (int q = 0; q < ROWS; ++q) {
        const double *xc = a.x + rows[q] * n3;
        const double *m0 = memo ? a.memo_x + rows[q] * n3 : xc;
        const double *m1 = memo ? a.memo_x + (g.C + rows[q]) * n3 : xc;
        bool d0 = false, d1 = false;
        for (int k = threadIdx.x; k < n3; k += THREADS) {
            const double v = xc[k];
            row_lds[k * ROWS + q] = v;
            if (memo) {
                const long long bits = __double_as_longlong(v);
                d0 = d0 || bits != __double_as_longlong(m0[k]);
                d1 = d1 || bits != __double_as_longlong(m1[k]);
            }
        }
        if (d0) differs[q][0] = 1;
        if (d1) differs[q][1] = 1;
    }
    __syncthreads();
    bool hit[ROWS], all_hit = memo;
    int way[ROWS];
#pragma unroll
    for (int q = 0; q < ROWS; ++q) {
        const bool h0 = memo && !differs[q][0], h1 = memo && !differs[q][1];
        hit[q] = h0 || h1;
        way[q] = hit[q] ? (h0 ? 0 : 1) : (memo ? 1 - (a.memo_state[g.C + rows[q]] & 1) : 0);
        all_hit = all_hit && hit[q];
    }
    if (memo) {
#pragma unroll
        for (int q = 0; q < ROWS; ++q) {
            if (hit[q] || row0 + q >= g.C) continue;         // uniform
            double *m = a.memo_x + ((int64_t)way[q] * g.C + rows[q]) * n3;
            for (int k = threadIdx.x; k < n3; k += THREADS) m[k] = row_lds[k * ROWS + q];
        }
    }
    double chi2[ROWS];
    if (given) {
#pragma unroll
        for (int q = 0; q < ROWS; ++q) chi2[q] = a.chi2_in[rows[q]];
    } else if (!all_hit) {                       // uniform
        PairResidRows<ROWS> f;
        f.xl = row_lds; f.I = a.I; f.J = a.J; f.ys = a.ys;
        block_sum_rows<ROWS, U, THREADS>(f, g.D, g.H, sc, round, chi2);
    } else {
#pragma unroll
        for (int q = 0; q < ROWS; ++q) chi2[q] = g.memo_sum[(int64_t)way[q] * g.C + rows[q]];
    }
    double prior[ROWS], kin[ROWS];
#pragma unroll
    for (int q = 0; q < ROWS; ++q) prior[q] = 0.0;
    if (a.has_prior) {
        ShiftSqRows<ROWS> fp;
        fp.xl = row_lds; fp.x0 = a.prior_x0;
        block_sum_rows<ROWS, U, THREADS>(fp, n3, a.H_d, sc, round, prior);
    }
    SqRows<ROWS> fk;
#pragma unroll
    for (int q = 0; q < ROWS; ++q) fk.row[q] = a.p + rows[q] * n3;
    block_sum_rows<ROWS, U, THREADS>(fk, n3, a.H_d, sc, round, kin);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < ROWS; ++q) {
            const int64_t row = row0 + q;
            if (row >= g.C) break;
            if (memo) {
                g.memo_sum[(int64_t)way[q] * g.C + row] = chi2[q];
                a.memo_state[row] = hit[q] ? 1 : 0;
                a.memo_state[g.C + row] = (uint8_t)way[q];
            }
            const double lp_lik = row_result(g, row, chi2[q]);
            const double lp_prior = a.prior_scale * prior[q];
            double lp = 0.0;                     // ((t0 + t1) + t2) + ..., binf_sum_terms_f64
            for (int k = 0; k < a.n_terms; ++k) {
                const int kind = a.term_kind[k];
                const double v = kind == 0 ? lp_prior
                               : kind == 1 ? lp_lik
                               : (a.extra[kind - 2] ? a.extra[kind - 2][row] : a.extra_scalar[kind - 2]);
                lp = (k == 0) ? v : lp + v;
            }
            if (a.log_prob) a.log_prob[row] = lp;
            a.energy[row] = 0.5 * kin[q] - lp;
        }
    }
}

}  // namespace binf
