// Linear forward model (mock = Theta . A for ANY constant design matrix A [K x N]) and
// its fusion with the Gaussian error model.  gfx950 (MI355X), wave64.
//
// Reference lines replaced:
//   AbstractForwardModel._evaluate of a linear model   binf/model/forwardmodels.py:23-28
//   Likelihood._evaluate_log_prob                      binf/pdf/likelihoods.py:141-146
//   GaussianErrorModel._evaluate_log_prob              binf/example/likelihood.py:54-57
//
// The product runs on the matrix pipe (v_mfma_f64_16x16x4_f64, tiles of 16 data points
// x 16 chains).  In the log-prob kernel the [C x N] mock data never leaves registers:
// residual, square and the running chi^2 are taken from the accumulator tile.
//
// Summation order.  A chain's chi^2 is summed over PIECES of the data range whose length
// is a constant (PIECE_TILES tiles), inside a piece per lane over n = lk, lk + 4, ... and
// then over the four lane partials as (0 + 1) + (2 + 3); the pieces are joined in piece
// order.  The k order of a mock datum follows from K alone.  Nothing depends on C or on
// where a chain sits in its batch: a shard reproduces the full batch bit for bit.
#include "common.hpp"

#include <math.h>

namespace binf {

typedef double lin_v4d __attribute__((ext_vector_type(4)));

constexpr int LIN_LDA = 17;          // padded row length of the staged A tile (doubles)
constexpr int PIECE_TILES = 64;      // data tiles (of 16 points) per piece: 1024 points

struct LinArgs {
    const double *theta;     // [C x K]
    const double *A;         // [K x N]
    const double *ys;        // [N]
    const double *tau_chain; // [C] or null
    double tau;
    double n_data;
    double *out;             // finish: log-prob [C]; else partial chi^2 [pieces x C]
    int64_t C;
    int32_t K;
    int32_t N;
    int32_t finish;          // 1: one piece, the error model's epilogue is applied here
};

// lp = -0.5 * chi2 * tau + N * 0.5 * log(tau): the epilogue of binf_poly_gauss_logp_f64
// (rowsum.hpp: row_result with scale 1), expression for expression
__device__ inline double lin_gauss_logp(double chi2, double t, double n_data)
{
    const double v = 1.0 * chi2;
    const double logZ = n_data * 0.5 * log(t);
    return -0.5 * v * t + logZ;
}

template <int B> struct LinBuf { static constexpr int value = B; };

// KS forward k-steps on the MFMA pipe (coefficients 0 .. 4 KS - 1), KV trailing
// coefficients on the VALU (K = 33: 8 MFMAs + 4 FMAs per tile instead of 9 MFMAs), CT
// 16-chain tiles per wave, as in poly_grad_mfma_kernel.  FULL: every tile whole
// (N % 16 == 0) and every staging offset inside 32 bits -- the prefetch goes through a
// buffer resource (tile offset in an SGPR, no VALU) and no validity select is left in
// the loop.  Either way the tile loop is unrolled over the two LDS buffers, so every LDS
// address is a per-thread base plus an immediate.
//
// Rows of the staged tile beyond K must be ZERO (a copy of row K - 1 would meet the zero
// coefficients of the padding as 0 * A, NaN for a non-finite design entry): they are
// zeroed once, and the threads that stage them write to 16 spare rows instead -- a row
// index chosen once per thread, not a select per tile.
template <int KS, int KV, int CT, bool FULL>
__global__ void __launch_bounds__(256, 2) linear_chi2_kernel(const LinArgs a)
{
    constexpr int KB = 4 * KS;
    constexpr int ROWS = KB + KV;
    constexpr int PASSES = (ROWS + 15) / 16;
    constexpr int SPARE = ROWS;                      // rows SPARE .. SPARE + 15
    __shared__ double sA[2][ROWS + 16][LIN_LDA];
    __shared__ double sY[2][16];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int lc = lane & 15;
    const int lk = lane >> 4;
    const int K = a.K, N = a.N;

    int64_t chain[CT];
    bool cvalid[CT];
    double th[CT][KS];
    double thv[CT][KV > 0 ? KV : 1];
    double chi[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        chain[c] = ((int64_t)blockIdx.y * 4 + wave) * (16 * CT) + 16 * c + lc;
        cvalid[c] = chain[c] < a.C;
        // B operands: theta[chain][4s + lk]
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int k = 4 * s + lk;
            th[c][s] = (cvalid[c] && k < K) ? a.theta[chain[c] * K + k] : 0.0;
        }
#pragma unroll
        for (int v = 0; v < KV; ++v)
            thv[c][v] = (cvalid[c] && KB + v < K) ? a.theta[chain[c] * K + KB + v] : 0.0;
        chi[c] = 0.0;
    }

    const int ntiles = (N + 15) / 16;
    const int t0 = (int)blockIdx.x * PIECE_TILES;
    int t1 = t0 + PIECE_TILES;
    if (t1 > ntiles) t1 = ntiles;

    for (int i = tid; i < 2 * (ROWS + 16) * LIN_LDA; i += 256) (&sA[0][0][0])[i] = 0.0;

    // staging: thread (srow, scol) moves A[16*pass + srow][16 t + scol]
    const int srow = tid >> 4, scol = tid & 15;
    int wrow[PASSES];                              // LDS row it lands in
    unsigned voff[PASSES];                         // FULL: byte offset inside a tile's columns
    int krow[PASSES];
#pragma unroll
    for (int ps = 0; ps < PASSES; ++ps) {
        const int k = 16 * ps + srow;
        wrow[ps] = k < K ? k : SPARE + srow;
        krow[ps] = k < K ? k : K - 1;
        voff[ps] = ((unsigned)krow[ps] * (unsigned)N + (unsigned)scol) * 8u;
    }
    const unsigned yoff = (unsigned)scol * 8u;
    __amdgpu_buffer_rsrc_t rA, rY;
    if constexpr (FULL) {
        rA = __builtin_amdgcn_make_buffer_rsrc((void *)a.A, 0, (unsigned)((int64_t)K * N * 8),
                                               0x00020000);
        rY = __builtin_amdgcn_make_buffer_rsrc((void *)a.ys, 0, (unsigned)((int64_t)N * 8),
                                               0x00020000);
    }
    double pre[PASSES];
    double prey = 0.0;
    auto fetch = [&](int t) {
        if constexpr (FULL) {
            const int soff = t * 128;              // 16 doubles per tile
#pragma unroll
            for (int ps = 0; ps < PASSES; ++ps)
                pre[ps] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rA, voff[ps], soff, 0));
            prey = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rY, yoff, soff, 0));
        } else {
            // unconditional loads at clamped indices (a load under a per-lane branch is
            // waited for at the join, before the tile's first MFMA)
            const int n = t * 16 + scol;
            const int nc = n < N ? n : N - 1;
#pragma unroll
            for (int ps = 0; ps < PASSES; ++ps) pre[ps] = a.A[(int64_t)krow[ps] * N + nc];
            prey = a.ys[nc];
        }
    };
    auto stash = [&](auto bc, int t) {
        constexpr int buf = decltype(bc)::value;
        const bool nv = FULL || t * 16 + scol < N;
#pragma unroll
        for (int ps = 0; ps < PASSES; ++ps) sA[buf][wrow[ps]][scol] = nv ? pre[ps] : 0.0;
        if (tid < 16) sY[buf][tid] = nv ? prey : 0.0;
    };
    auto tile = [&](auto bc, int t) {
        constexpr int buf = decltype(bc)::value;
        fetch(t + 1 < t1 ? t + 1 : t);             // in flight during the MFMAs
        __builtin_amdgcn_sched_barrier(0);
        // M^T[n][c] = sum_k A[k][n] theta[c][k]
        lin_v4d acc[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[c] = (lin_v4d){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const double av = sA[buf][4 * s + lk][lc];
#pragma unroll
            for (int c = 0; c < CT; ++c)
                acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, th[c][s], acc[c], 0, 0, 0);
        }
        // trailing coefficients on the VALU: lane holds (n = lk + 4r, c = lc)
#pragma unroll
        for (int v = 0; v < KV; ++v)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double av = sA[buf][KB + v][lk + 4 * r];
#pragma unroll
                for (int c = 0; c < CT; ++c)
                    acc[c][r] = __builtin_fma(thv[c][v], av, acc[c][r]);
            }
        // residual, square, running chi^2; a padding column (n >= N) holds 0 * theta,
        // NaN for a non-finite coefficient, and is left out by a select
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int nl = lk + 4 * r;
            const double yv = sY[buf][nl];
            const bool nv = FULL || t * 16 + nl < N;
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                const double d = acc[c][r] - yv;
                const double s = __builtin_fma(d, d, chi[c]);
                chi[c] = nv ? s : chi[c];
            }
        }
        if (t + 1 < t1) stash(LinBuf<buf ^ 1>(), t + 1);
        __syncthreads();
    };

    __syncthreads();                               // the zeroed rows, before anything lands
    if (t0 < t1) {
        fetch(t0);
        stash(LinBuf<0>(), t0);
    }
    __syncthreads();
    int t = t0;
    for (; t + 1 < t1; t += 2) {
        tile(LinBuf<0>(), t);
        tile(LinBuf<1>(), t + 1);
    }
    if (t < t1) tile(LinBuf<0>(), t);

#pragma unroll
    for (int c = 0; c < CT; ++c) {
        // the four lk partials of a chain: (0 + 1) + (2 + 3)
        chi[c] = chi[c] + shfl_xor_f64(chi[c], 16);
        chi[c] = chi[c] + shfl_xor_f64(chi[c], 32);
        if (cvalid[c] && lk == 0) {
            if (a.finish) {
                const double tc = a.tau_chain ? a.tau_chain[chain[c]] : a.tau;
                a.out[chain[c]] = lin_gauss_logp(chi[c], tc, a.n_data);
            } else {
                a.out[(int64_t)blockIdx.x * a.C + chain[c]] = chi[c];
            }
        }
    }
}

// chi2[c] = part[0][c] + part[1][c] + ... in piece order, then the error model
__global__ void __launch_bounds__(256)
linear_finish_kernel(const double *part, int32_t pieces, double tau, const double *tau_chain,
                     double *out, int64_t C, double n_data)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double s = part[c];
    for (int k = 1; k < pieces; ++k) s = s + part[(int64_t)k * C + c];
    out[c] = lin_gauss_logp(s, tau_chain ? tau_chain[c] : tau, n_data);
}

// out[c][n] = sum_k theta[c][k] A[k][n].  Chains are the ROWS of the product here (A
// operand theta[c0 + lc][4s + lk], B operand A[4s + lk][n0 + lc]): a result register
// then holds 16 consecutive data points of a chain and the stores are 128-byte rows.
// One wave per 16-chain tile, operands straight from global memory (the design matrix
// stays in L2; the kernel is bound by the [C x N] it writes).  Padding rows and columns
// enter as zeros on both sides and are never stored.
template <int KS>
__global__ void __launch_bounds__(256)
linear_forward_kernel(const double *theta, const double *A, double *out, int64_t C, int32_t K,
                      int32_t N)
{
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int lc = lane & 15;
    const int lk = lane >> 4;
    const int64_t c0 = ((int64_t)blockIdx.y * 4 + wave) * 16;
    if (c0 >= C) return;                           // wave-uniform; the kernel has no barrier
    const int64_t ca = c0 + lc;
    double th[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int k = 4 * s + lk;
        th[s] = (ca < C && k < K) ? theta[ca * K + k] : 0.0;
    }
    const int ntiles = (N + 15) / 16;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int n = t * 16 + lc;
        const bool nv = n < N;
        const int nc = nv ? n : N - 1;
        double b[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int k = 4 * s + lk;
            const double v = A[(int64_t)(k < K ? k : K - 1) * N + nc];
            b[s] = (k < K && nv) ? v : 0.0;
        }
        lin_v4d acc = (lin_v4d){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < KS; ++s)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(th[s], b[s], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t c = c0 + lk + 4 * r;
            if (c < C && nv) out[c * N + n] = acc[r];
        }
    }
}

template <int KS, int KV>
static hipError_t chi2_launch(const LinArgs &a, int ct, bool full, dim3 grid, hipStream_t st)
{
    if (full) {
        if (ct == 2) linear_chi2_kernel<KS, KV, 2, true><<<grid, 256, 0, st>>>(a);
        else         linear_chi2_kernel<KS, KV, 1, true><<<grid, 256, 0, st>>>(a);
    } else {
        if (ct == 2) linear_chi2_kernel<KS, KV, 2, false><<<grid, 256, 0, st>>>(a);
        else         linear_chi2_kernel<KS, KV, 1, false><<<grid, 256, 0, st>>>(a);
    }
    return hipGetLastError();
}

// the split of K into MFMA k-steps and VALU coefficients is that of the gradient kernel
static hipError_t chi2_dispatch(const LinArgs &a, int64_t K, int ct, bool full, dim3 grid,
                                hipStream_t st)
{
    if (K <= 4)       return chi2_launch<1, 0>(a, ct, full, grid, st);
    else if (K <= 8)  return chi2_launch<2, 0>(a, ct, full, grid, st);
    else if (K <= 16) return chi2_launch<4, 0>(a, ct, full, grid, st);
    else if (K == 17) return chi2_launch<4, 1>(a, ct, full, grid, st);
    else if (K == 18) return chi2_launch<4, 2>(a, ct, full, grid, st);
    else if (K <= 32) return chi2_launch<8, 0>(a, ct, full, grid, st);
    else if (K == 33) return chi2_launch<8, 1>(a, ct, full, grid, st);
    else if (K == 34) return chi2_launch<8, 2>(a, ct, full, grid, st);
    else if (K <= 36) return chi2_launch<9, 0>(a, ct, full, grid, st);
    else if (K <= 48) return chi2_launch<12, 0>(a, ct, full, grid, st);
    else if (K == 49) return chi2_launch<12, 1>(a, ct, full, grid, st);
    else if (K == 50) return chi2_launch<12, 2>(a, ct, full, grid, st);
    return chi2_launch<16, 0>(a, ct, full, grid, st);
}

static int64_t linear_pieces(int64_t N)
{
    const int64_t ntiles = (N + 15) / 16;
    const int64_t np = (ntiles + PIECE_TILES - 1) / PIECE_TILES;
    return np < 1 ? 1 : np;
}

static int32_t check_linear(const char *what, int64_t C, int64_t K, int64_t N)
{
    if (C < 0 || K < 1 || N < 0)
        return fail(BINF_E_ARG, "%s: need C>=0, K>=1, N>=0", what);
    if (K > 64)
        return fail(BINF_E_UNSUPPORTED, "%s: K=%lld coefficients > 64 not covered by the native linear kernels", what, (long long)K);
    if (C > 65535 * 64LL || N > 0x7fffffffLL - 16)
        return fail(BINF_E_UNSUPPORTED, "%s: too large", what);
    return 0;
}

}  // namespace binf

using namespace binf;

extern "C" int32_t binf_linear_forward_f64(const double *coeffs, const double *design,
                                           double *out, int64_t C, int64_t K, int64_t N,
                                           void *stream)
{
    int32_t rc = check_linear("linear_forward", C, K, N);
    if (rc) return rc;
    if (C == 0 || N == 0) return 0;
    if (!coeffs || !design || !out) return fail(BINF_E_ARG, "linear_forward: null buffer");
    if (overlap_f64(out, C * N, coeffs, C * K) || overlap_f64(out, C * N, design, K * N))
        return fail(BINF_E_ALIAS, "linear_forward: out overlaps coeffs or design");
    const int64_t ntiles = (N + 15) / 16;
    dim3 grid((unsigned)(ntiles < 256 ? ntiles : 256), (unsigned)((C + 63) / 64));
    hipStream_t st = (hipStream_t)stream;
    const int32_t k = (int32_t)K, n = (int32_t)N;
    if (K <= 4)       linear_forward_kernel<1><<<grid, 256, 0, st>>>(coeffs, design, out, C, k, n);
    else if (K <= 8)  linear_forward_kernel<2><<<grid, 256, 0, st>>>(coeffs, design, out, C, k, n);
    else if (K <= 16) linear_forward_kernel<4><<<grid, 256, 0, st>>>(coeffs, design, out, C, k, n);
    else if (K <= 32) linear_forward_kernel<8><<<grid, 256, 0, st>>>(coeffs, design, out, C, k, n);
    else if (K <= 36) linear_forward_kernel<9><<<grid, 256, 0, st>>>(coeffs, design, out, C, k, n);
    else if (K <= 48) linear_forward_kernel<12><<<grid, 256, 0, st>>>(coeffs, design, out, C, k, n);
    else              linear_forward_kernel<16><<<grid, 256, 0, st>>>(coeffs, design, out, C, k, n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "linear_forward launch");
    return 0;
}

extern "C" int64_t binf_linear_gauss_logp_workspace_bytes(int64_t C, int64_t K, int64_t N)
{
    if (C <= 0 || K <= 0 || N <= 0) return 0;
    const int64_t np = linear_pieces(N);
    return np > 1 ? np * C * (int64_t)sizeof(double) : 0;
}

extern "C" int32_t binf_linear_gauss_logp_f64(const double *coeffs, const double *design,
                                              const double *ys, double precision,
                                              const double *precision_chain, double *out,
                                              void *workspace, int64_t workspace_bytes,
                                              int64_t C, int64_t K, int64_t N, void *stream)
{
    int32_t rc = check_linear("linear_gauss_logp", C, K, N);
    if (rc) return rc;
    if (C == 0) return 0;
    if (!coeffs || !out || ((!design || !ys) && N > 0))
        return fail(BINF_E_ARG, "linear_gauss_logp: null buffer");
    if (overlap_f64(out, C, coeffs, C * K) || overlap_f64(out, C, design, K * N) ||
        overlap_f64(out, C, ys, N) || overlap_f64(out, C, precision_chain, C))
        return fail(BINF_E_ALIAS, "linear_gauss_logp: out overlaps an input");
    // The pieces follow from N alone (never from C), so a missing or short workspace is
    // an error, never a silent change of summation order.
    const int64_t np = linear_pieces(N);
    const int64_t need = np > 1 ? np * C * (int64_t)sizeof(double) : 0;
    if (need > 0) {
        if (!workspace || workspace_bytes < need)
            return fail(BINF_E_ARG, "linear_gauss_logp: needs %lld bytes of workspace "
                        "(binf_linear_gauss_logp_workspace_bytes), got %lld",
                        (long long)need, (long long)workspace_bytes);
        if (overlap_f64(workspace, need / 8, out, C) || overlap_f64(workspace, need / 8, coeffs, C * K) ||
            overlap_f64(workspace, need / 8, design, K * N) || overlap_f64(workspace, need / 8, ys, N) ||
            overlap_f64(workspace, need / 8, precision_chain, C))
            return fail(BINF_E_ALIAS, "linear_gauss_logp: the workspace overlaps a buffer");
    }
    LinArgs a;
    a.theta = coeffs; a.A = design; a.ys = ys; a.tau_chain = precision_chain; a.tau = precision;
    a.n_data = (double)N; a.C = C; a.K = (int32_t)K; a.N = (int32_t)N;
    a.finish = np > 1 ? 0 : 1;
    a.out = np > 1 ? (double *)workspace : out;
    const int ct = C >= 4096 ? 2 : 1;              // as the gradient kernel (poly.hip: grad_ct)
    const bool full = N >= 16 && N % 16 == 0 && K * N < (1LL << 28);
    dim3 grid((unsigned)np, (unsigned)((C + 64 * ct - 1) / (64 * ct)));
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = chi2_dispatch(a, K, ct, full, grid, st);
    if (e != hipSuccess) return hip_fail(e, "linear_gauss_logp launch");
    if (np > 1) {
        linear_finish_kernel<<<dim3((unsigned)((C + 255) / 256)), 256, 0, st>>>(
            (const double *)workspace, (int32_t)np, precision, precision_chain, out, C, (double)N);
        e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, "linear_gauss_logp finish launch");
    }
    return 0;
}
