// The rank layer of the convergence diagnostics: a segmented sort of the whole record per
// dimension, and what follows from it -- sorted values, tie-averaged ranks looked up in a
// table of normal scores, quantiles -- plus the two element-wise maps (fold, indicator) and
// the last combination of rank_summary.  Build-defined, like diagnostics.hip.
//
// Pooled set of dimension i: the S = split * n * C values x[t'][c][i], t' the compressed time
// index of the split record (segment 1 starts at T - n), element e = t' * C + c.  The contract
// is in include/binf_hip.h; tests/rank_diagnostics_ref.py restates it in numpy.  Every output
// is a function of the values alone (ranks are integers, sorted values are unique), so the
// sorting network below is not part of the contract.
//
// Keys: an order-preserving u64 image of the double (sign bit flipped for x >= +0.0, all bits
// for x < 0): -0.0 < +0.0 as keys, every NaN becomes RANK_NAN_KEY above +inf, and the pad key
// sorts after that.  P = the power of two >= S; the workspace holds keys [D x P] (u64) and
// element indices [D x P] (u32).
//
// Kernels (gfx950, wave64):
//   load      a transposing copy, draws -> keys: a workgroup reads 256 elements x 1..8 adjacent
//             dimensions with lanes along the dimension (the record's unit stride) and writes
//             each dimension's 256 keys as one 2 KiB run.  Pads included.
//   tile      one tile of RANK_TILE = 8192 (key, index) pairs in LDS, 96 KiB: every stage of
//             the bitonic network with a stride below the tile.  P <= 8192: the whole sort of
//             a dimension (P <= 1024: a 12 KiB tile, so that small records fill a CU).
//   pass      the strides at or above the tile, a compare-exchange over the workspace; up to
//             three strides per pass (eight elements per thread) while that many are left
//             above the tile.
//   finish    sorted values out; a position's rank from its neighbours (no tie: the position
//             itself) or from two binary searches of its tie group; ztab[k] scattered through
//             the element index.
#include "common.hpp"
#include "diag_draws.hpp"

namespace binf {

constexpr uint64_t RANK_NAN_KEY = 0xFFFFFFFFFFFFFFFEull;
constexpr uint64_t RANK_PAD_KEY = 0xFFFFFFFFFFFFFFFFull;
constexpr uint64_t RANK_NEG_ZERO_KEY = 0x7FFFFFFFFFFFFFFFull;
constexpr uint64_t RANK_POS_ZERO_KEY = 0x8000000000000000ull;
constexpr int RANK_TILE = 8192;
constexpr int RANK_SMALL_TILE = 1024;
constexpr int64_t RANK_MAX_S = (int64_t)1 << 30;

__device__ inline uint64_t rank_key(double x)
{
    if (x != x) return RANK_NAN_KEY;
    const uint64_t b = (uint64_t)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | RANK_POS_ZERO_KEY);
}

__device__ inline double rank_value(uint64_t k)
{
    return __longlong_as_double((long long)((k >> 63) ? (k & ~RANK_POS_ZERO_KEY) : ~k));
}

// ties are by numeric equality: the two zeros are one group
__device__ inline uint64_t rank_tie_key(uint64_t k) { return k == RANK_NEG_ZERO_KEY ? RANK_POS_ZERO_KEY : k; }

struct RankArgs {
    DiagDraws d;
    int64_t S, P;
    int32_t logP;
    int32_t dt;                 // dimensions per workgroup of the load: 1, 2, 4 or 8
    int64_t n_etiles;           // ceil(P / 256)
    uint64_t *keys;             // [D x P]
    uint32_t *idx;              // [D x P]
    const double *ztab;         // [2 S + 1]
    double *sorted;             // [D x S] or NULL
    double *z;                  // [S x D] or NULL
};

// element e of the pooled set -> offset of x[t][c][0]
__device__ inline int64_t rank_element_offset(const DiagDraws &d, int64_t e)
{
    const int64_t tp = e <= 0xffffffffLL && d.C <= 0xffffffffLL ? (int64_t)((uint32_t)e / (uint32_t)d.C) : e / d.C;
    const int64_t c = e - tp * d.C;
    const int64_t t = tp < d.n ? tp : tp + (d.T - 2 * d.n);
    return t * d.st + c * d.sc;
}

// ---------------------------------------------------------------------------------------
// load
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) rank_load_kernel(const RankArgs a)
{
    __shared__ uint64_t sm[8][257];
    const int tid = threadIdx.x;
    const int64_t et = (int64_t)blockIdx.x % a.n_etiles;
    const int64_t dti = (int64_t)blockIdx.x / a.n_etiles;
    const int64_t e0 = et * 256;
    const int dt = a.dt, epp = 256 / dt;
    const int il = tid % dt, el = tid / dt;
    const int64_t i = dti * dt + il;
    for (int pass = 0; pass < dt; ++pass) {
        const int le = pass * epp + el;
        const int64_t e = e0 + le;
        if (i < a.d.D && e < a.P)
            sm[il][le] = e < a.S ? rank_key(a.d.x[rank_element_offset(a.d, e) + i]) : RANK_PAD_KEY;
    }
    __syncthreads();
    const int64_t e = e0 + tid;
    if (e >= a.P) return;
    for (int q = 0; q < dt; ++q) {
        const int64_t i2 = dti * dt + q;
        if (i2 < a.d.D) a.keys[i2 * a.P + e] = sm[q][tid];
    }
}

// ---------------------------------------------------------------------------------------
// tile: the strides below the tile, in LDS
// ---------------------------------------------------------------------------------------
// MERGE false: stages k = 2 .. min(TILE, P) from the loaded keys (the index starts as the
// position); MERGE true: strides TILE / 2 .. 1 of stage k.
template <int TILE, int THREADS, bool MERGE>
__global__ void __launch_bounds__(THREADS) rank_tile_kernel(const RankArgs a, const int64_t k_merge)
{
    __shared__ uint64_t sk[TILE];
    __shared__ uint32_t si[TILE];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int len = a.P < TILE ? (int)a.P : TILE;
    const int64_t tpd = a.P / len;                                  // tiles per dimension
    const int64_t dim = (int64_t)blockIdx.x / tpd;
    const int64_t tile = (int64_t)blockIdx.x - dim * tpd;
    const int64_t first = tile * len;                               // position of the tile's first pair
    const int64_t base = dim * a.P + first;
    for (int q = tid; q < len; q += nt) {
        sk[q] = a.keys[base + q];
        si[q] = MERGE ? a.idx[base + q] : (uint32_t)(first + q);
    }
    __syncthreads();
    auto stage = [&](int64_t k, int j) {
        for (int p = tid; p < len / 2; p += nt) {
            const int lo = ((p & ~(j - 1)) << 1) | (p & (j - 1));
            const int hi = lo | j;
            const bool asc = ((first + lo) & k) == 0;
            const uint64_t ka = sk[lo], kb = sk[hi];
            if (asc ? ka > kb : ka < kb) {
                sk[lo] = kb;
                sk[hi] = ka;
                const uint32_t ia = si[lo];
                si[lo] = si[hi];
                si[hi] = ia;
            }
        }
        __syncthreads();
    };
    if (MERGE) {
        for (int j = len / 2; j > 0; j >>= 1) stage(k_merge, j);
    } else {
        for (int k = 2; k <= len; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) stage(k, j);
    }
    for (int q = tid; q < len; q += nt) {
        a.keys[base + q] = sk[q];
        a.idx[base + q] = si[q];
    }
}

// ---------------------------------------------------------------------------------------
// pass: the strides at or above the tile, over the workspace
// ---------------------------------------------------------------------------------------
__device__ inline void rank_cmpx(uint64_t &ka, uint64_t &kb, uint32_t &ia, uint32_t &ib, bool asc)
{
    if (asc ? ka > kb : ka < kb) {
        const uint64_t k = ka;
        ka = kb;
        kb = k;
        const uint32_t i = ia;
        ia = ib;
        ib = i;
    }
}

// R strides of stage k per pass, j the largest: a thread holds the 2^R elements that differ in
// those R index bits and runs their part of the network in registers.
template <int R>
__global__ void __launch_bounds__(256) rank_pass_kernel(const RankArgs a, const int64_t k, const int64_t j)
{
    constexpr int N = 1 << R;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int shift = a.logP - R;
    const int64_t dim = p >> shift;
    if (dim >= a.d.D) return;
    const int64_t q = p & (((int64_t)1 << shift) - 1);
    const int64_t low = j >> (R - 1);                       // the smallest stride of the pass
    const int64_t i0 = ((q & ~(low - 1)) << R) | (q & (low - 1));
    const bool asc = (i0 & k) == 0;
    uint64_t *keys = a.keys + dim * a.P + i0;
    uint32_t *idx = a.idx + dim * a.P + i0;
    uint64_t kk[N];
    uint32_t xx[N];
#pragma unroll
    for (int m = 0; m < N; ++m) {
        kk[m] = keys[m * low];
        xx[m] = idx[m * low];
    }
#pragma unroll
    for (int s = R - 1; s >= 0; --s)
#pragma unroll
        for (int m = 0; m < N; ++m)
            if (!(m & (1 << s))) rank_cmpx(kk[m], kk[m | (1 << s)], xx[m], xx[m | (1 << s)], asc);
#pragma unroll
    for (int m = 0; m < N; ++m) {
        keys[m * low] = kk[m];
        idx[m * low] = xx[m];
    }
}

// ---------------------------------------------------------------------------------------
// finish
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) rank_finish_kernel(const RankArgs a)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t dim = p >> a.logP;
    const int64_t j = p & (a.P - 1);
    if (dim >= a.d.D || j >= a.S) return;
    const uint64_t *row = a.keys + dim * a.P;
    const uint64_t key = row[j];
    if (a.sorted) a.sorted[dim * a.S + j] = rank_value(key);
    if (!a.z) return;
    const int64_t out = (int64_t)a.idx[dim * a.P + j] * a.d.D + dim;
    if (row[a.S - 1] == RANK_NAN_KEY) {                     // NaNs sort last: the dimension holds one
        a.z[out] = __longlong_as_double(0x7ff8000000000000LL);
        return;
    }
    const uint64_t tk = rank_tie_key(key);
    int64_t lo = j, hi = j;                                 // first and last position of the tie group
    if (j > 0 && rank_tie_key(row[j - 1]) == tk) {
        int64_t l = 0, r = j - 1;                           // the first position in [0, j - 1] that holds tk
        while (l < r) {
            const int64_t m = (l + r) >> 1;
            if (rank_tie_key(row[m]) < tk) l = m + 1; else r = m;
        }
        lo = l;
    }
    if (j + 1 < a.S && rank_tie_key(row[j + 1]) == tk) {
        int64_t l = j + 1, r = a.S - 1;                     // the last position in [j + 1, S - 1] that holds tk
        while (l < r) {
            const int64_t m = (l + r + 1) >> 1;
            if (rank_tie_key(row[m]) > tk) r = m - 1; else l = m;
        }
        hi = l;
    }
    a.z[out] = a.ztab[lo + hi + 2];
}

// ---------------------------------------------------------------------------------------
// quantiles, maps, combination
// ---------------------------------------------------------------------------------------
struct RankProbs { double p[16]; };

__global__ void __launch_bounds__(256) rank_quantiles_kernel(const double *sorted, int64_t S, int64_t D,
                                                             const RankProbs probs, int32_t Q, double *out)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (int64_t)Q * D) return;
    const int64_t q = p / D, i = p - q * D;
    const double *row = sorted + i * S;
    const double last = row[S - 1];
    if (last != last) {
        out[p] = last;
        return;
    }
    const double h = (double)(S - 1) * probs.p[q];
    const double fl = floor(h);
    const double g = h - fl;
    const int64_t lo = (int64_t)fl;
    const double va = row[lo], vb = row[lo + 1 < S ? lo + 1 : S - 1];
    const double d = vb - va;
    out[p] = g < 0.5 ? va + d * g : vb - d * (1.0 - g);
}

__global__ void __launch_bounds__(256) rank_map_kernel(const DiagDraws a, int32_t op, const double *param, double *out)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= a.split * a.n * a.C * a.D) return;
    const int64_t e = p <= 0xffffffffLL && a.D <= 0xffffffffLL ? (int64_t)((uint32_t)p / (uint32_t)a.D) : p / a.D;
    const int64_t i = p - e * a.D;
    const double x = a.x[rank_element_offset(a, e) + i];
    const double c = param[i];
    out[p] = op == BINF_DRAWS_MAP_FOLD ? fabs(x - c) : (x <= c ? 1.0 : 0.0);
}

struct RankCombineArgs {
    const double *rhat_bulk, *rhat_folded, *ess_lo, *ess_hi;
    const uint8_t *flags[4];
    double *rhat, *ess_tail;
    uint8_t *truncated;
    int64_t D;
};

__global__ void __launch_bounds__(256) rank_combine_kernel(const RankCombineArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.D) return;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const double rb = a.rhat_bulk[i], rf = a.rhat_folded[i];
    a.rhat[i] = (rb != rb || rf != rf) ? nan : (rb > rf ? rb : rf);
    const double el = a.ess_lo[i], eh = a.ess_hi[i];
    a.ess_tail[i] = (el != el || eh != eh) ? nan : (el < eh ? el : eh);
    uint8_t t = 0;
#pragma unroll
    for (int f = 0; f < 4; ++f) t |= a.flags[f][i] ? 1 : 0;
    a.truncated[i] = t;
}

static int64_t rank_pow2(int64_t S, int32_t &logP)
{
    logP = 1;
    while (((int64_t)1 << logP) < S) ++logP;
    return (int64_t)1 << logP;
}

}  // namespace binf

using namespace binf;

extern "C" int64_t binf_rank_sort_workspace_bytes(int64_t S, int64_t D)
{
    if (S < 2 || S > RANK_MAX_S || D < 1) return 0;
    int32_t logP;
    const int64_t P = rank_pow2(S, logP);
    const __int128 need = (__int128)D * P * 12 + 256;
    return need > ((__int128)1 << 62) ? 0 : (int64_t)need;
}

extern "C" int32_t binf_rank_normalise_f64(const double *draws, int64_t stride_t, int64_t stride_c,
                                           int64_t stride_i, int64_t T, int64_t C, int64_t D,
                                           int32_t split, const double *ztab, double *sorted, double *z,
                                           void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *what = "rank_normalise";
    RankArgs a = {};
    const int32_t rc = diag_draws(what, draws, stride_t, stride_c, stride_i, T, C, D, split, a.d);
    if (rc) return rc;
    if ((__int128)a.d.M * a.d.n > RANK_MAX_S)
        return fail(BINF_E_UNSUPPORTED, "%s: a pooled set of more than 2^30 values per dimension", what);
    if (!sorted && !z) return fail(BINF_E_ARG, "%s: neither sorted nor z asked for", what);
    if (z && !ztab) return fail(BINF_E_ARG, "%s: z needs the table ztab", what);
    a.S = a.d.M * a.d.n;
    a.P = rank_pow2(a.S, a.logP);
    const int64_t need = binf_rank_sort_workspace_bytes(a.S, D);
    if (need == 0) return fail(BINF_E_UNSUPPORTED, "%s: workspace size overflows", what);
    if (!workspace || workspace_bytes < need)
        return fail(BINF_E_ARG, "%s: needs %lld bytes of workspace (binf_rank_sort_workspace_bytes), got %lld",
                    what, (long long)need, (long long)workspace_bytes);
    if (((uintptr_t)workspace & 7) != 0) return fail(BINF_E_ARG, "%s: the workspace is not 8-byte aligned", what);
    const int64_t SD = a.S * D;
    if ((__int128)SD > ((__int128)1 << 60)) return fail(BINF_E_UNSUPPORTED, "%s: S * D too large", what);
    struct Buf { const void *p; int64_t bytes; };
    const Buf in[2] = {{draws, a.d.span * 8}, {z ? ztab : nullptr, (2 * a.S + 1) * 8}};
    const Buf out[3] = {{sorted, SD * 8}, {z, SD * 8}, {workspace, need}};
    for (int o = 0; o < 3; ++o) {
        for (int q = 0; q < 2; ++q)
            if (overlap_bytes(out[o].p, out[o].bytes, in[q].p, in[q].bytes))
                return fail(BINF_E_ALIAS, "%s: an output or the workspace overlaps an input", what);
        for (int q = o + 1; q < 3; ++q)
            if (overlap_bytes(out[o].p, out[o].bytes, out[q].p, out[q].bytes))
                return fail(BINF_E_ALIAS, "%s: outputs overlap each other or the workspace", what);
    }
    a.dt = D >= 8 ? 8 : (D > 2 ? 4 : (int32_t)D);
    a.n_etiles = (a.P + 255) / 256;
    const int64_t n_dtiles = (D + a.dt - 1) / a.dt;
    const __int128 load_blocks = (__int128)a.n_etiles * n_dtiles;
    const __int128 flat_blocks = ((__int128)D * a.P + 255) / 256;
    if (load_blocks > 0x7fffffffLL || flat_blocks > 0x7fffffffLL || D > 0x7fffffffLL)
        return fail(BINF_E_UNSUPPORTED, "%s: D * P too large for one launch", what);
    a.keys = (uint64_t *)workspace;
    a.idx = (uint32_t *)(a.keys + D * a.P);
    a.ztab = ztab;
    a.sorted = sorted;
    a.z = z;
    hipStream_t st = (hipStream_t)stream;
    rank_load_kernel<<<dim3((unsigned)load_blocks), 256, 0, st>>>(a);
    if (a.P <= RANK_SMALL_TILE) {
        const int threads = a.P / 2 < 64 ? 64 : (a.P / 2 > 256 ? 256 : (int)(a.P / 2));
        rank_tile_kernel<RANK_SMALL_TILE, 256, false><<<dim3((unsigned)D), threads, 0, st>>>(a, 0);
    } else {
        const int64_t tiles = a.P <= RANK_TILE ? D : D * (a.P / RANK_TILE);
        rank_tile_kernel<RANK_TILE, 1024, false><<<dim3((unsigned)tiles), 1024, 0, st>>>(a, 0);
        for (int64_t k = 2 * (int64_t)RANK_TILE; k <= a.P; k <<= 1) {
            int64_t j = k >> 1;
            while (j >= RANK_TILE) {
                const int64_t left = j / (RANK_TILE / 2);       // 2^(strides at or above the tile still to do)
                const int r = left >= 8 ? 3 : (left >= 4 ? 2 : 1);
                const dim3 grid((unsigned)(((D * a.P >> r) + 255) / 256));
                if (r == 3) rank_pass_kernel<3><<<grid, 256, 0, st>>>(a, k, j);
                else if (r == 2) rank_pass_kernel<2><<<grid, 256, 0, st>>>(a, k, j);
                else rank_pass_kernel<1><<<grid, 256, 0, st>>>(a, k, j);
                j >>= r;
            }
            rank_tile_kernel<RANK_TILE, 1024, true><<<dim3((unsigned)tiles), 1024, 0, st>>>(a, k);
        }
    }
    rank_finish_kernel<<<dim3((unsigned)flat_blocks), 256, 0, st>>>(a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what);
    return 0;
}

extern "C" int32_t binf_sorted_quantiles_f64(const double *sorted, int64_t S, int64_t D, const double *probs,
                                             int32_t Q, double *out, void *stream)
{
    const char *what = "sorted_quantiles";
    if (S < 1 || D < 1) return fail(BINF_E_ARG, "%s: S >= 1 and D >= 1 required", what);
    if (Q < 1 || Q > 16) return fail(BINF_E_ARG, "%s: Q = %d probabilities (1 .. 16 required)", what, Q);
    if (!sorted || !probs || !out) return fail(BINF_E_ARG, "%s: null buffer", what);
    RankProbs pr = {};
    for (int q = 0; q < Q; ++q) {
        if (!(probs[q] >= 0.0 && probs[q] <= 1.0))
            return fail(BINF_E_ARG, "%s: probability %g outside [0, 1]", what, probs[q]);
        pr.p[q] = probs[q];
    }
    if ((__int128)S * D > ((__int128)1 << 60)) return fail(BINF_E_UNSUPPORTED, "%s: S * D too large", what);
    if (overlap_f64(out, (int64_t)Q * D, sorted, S * D)) return fail(BINF_E_ALIAS, "%s: out overlaps sorted", what);
    const int64_t blocks = ((int64_t)Q * D + 255) / 256;
    if (blocks > 0x7fffffffLL) return fail(BINF_E_UNSUPPORTED, "%s: Q * D too large for one launch", what);
    rank_quantiles_kernel<<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(sorted, S, D, pr, Q, out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what);
    return 0;
}

extern "C" int32_t binf_draws_map_f64(const double *draws, int64_t stride_t, int64_t stride_c, int64_t stride_i,
                                      int64_t T, int64_t C, int64_t D, int32_t split, int32_t op,
                                      const double *param, double *out, void *stream)
{
    const char *what = "draws_map";
    DiagDraws d;
    const int32_t rc = diag_draws(what, draws, stride_t, stride_c, stride_i, T, C, D, split, d);
    if (rc) return rc;
    if (op != BINF_DRAWS_MAP_FOLD && op != BINF_DRAWS_MAP_LE)
        return fail(BINF_E_ARG, "%s: op %d is neither BINF_DRAWS_MAP_FOLD nor BINF_DRAWS_MAP_LE", what, op);
    if (!param || !out) return fail(BINF_E_ARG, "%s: null buffer", what);
    const __int128 total = (__int128)d.M * d.n * D;
    if (total > ((__int128)1 << 60)) return fail(BINF_E_UNSUPPORTED, "%s: the record is too large", what);
    if (overlap_f64(out, (int64_t)total, draws, d.span) || overlap_f64(out, (int64_t)total, param, D))
        return fail(BINF_E_ALIAS, "%s: out overlaps an input", what);
    const __int128 blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffLL) return fail(BINF_E_UNSUPPORTED, "%s: the record is too large for one launch", what);
    rank_map_kernel<<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(d, op, param, out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what);
    return 0;
}

extern "C" int32_t binf_rank_diag_combine_f64(const double *rhat_bulk, const double *rhat_folded,
                                              const double *ess_lo, const double *ess_hi,
                                              const uint8_t *trunc_mean, const uint8_t *trunc_bulk,
                                              const uint8_t *trunc_lo, const uint8_t *trunc_hi, int64_t D,
                                              double *rhat, double *ess_tail, uint8_t *truncated, void *stream)
{
    const char *what = "rank_diag_combine";
    if (D < 1) return fail(BINF_E_ARG, "%s: D >= 1 required", what);
    if (!rhat_bulk || !rhat_folded || !ess_lo || !ess_hi || !trunc_mean || !trunc_bulk || !trunc_lo ||
        !trunc_hi || !rhat || !ess_tail || !truncated)
        return fail(BINF_E_ARG, "%s: null buffer", what);
    if (D > ((int64_t)1 << 38)) return fail(BINF_E_UNSUPPORTED, "%s: D too large for one launch", what);
    struct Buf { const void *p; int64_t bytes; };
    const Buf in[8] = {{rhat_bulk, D * 8}, {rhat_folded, D * 8}, {ess_lo, D * 8}, {ess_hi, D * 8},
                       {trunc_mean, D}, {trunc_bulk, D}, {trunc_lo, D}, {trunc_hi, D}};
    const Buf out[3] = {{rhat, D * 8}, {ess_tail, D * 8}, {truncated, D}};
    for (int o = 0; o < 3; ++o) {
        for (int q = 0; q < 8; ++q)
            if (overlap_bytes(out[o].p, out[o].bytes, in[q].p, in[q].bytes))
                return fail(BINF_E_ALIAS, "%s: an output overlaps an input", what);
        for (int q = o + 1; q < 3; ++q)
            if (overlap_bytes(out[o].p, out[o].bytes, out[q].p, out[q].bytes))
                return fail(BINF_E_ALIAS, "%s: outputs overlap each other", what);
    }
    RankCombineArgs a = {};
    a.rhat_bulk = rhat_bulk; a.rhat_folded = rhat_folded; a.ess_lo = ess_lo; a.ess_hi = ess_hi;
    a.flags[0] = trunc_mean; a.flags[1] = trunc_bulk; a.flags[2] = trunc_lo; a.flags[3] = trunc_hi;
    a.rhat = rhat; a.ess_tail = ess_tail; a.truncated = truncated; a.D = D;
    rank_combine_kernel<<<dim3((unsigned)((D + 255) / 256)), 256, 0, (hipStream_t)stream>>>(a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what);
    return 0;
}
