// Convergence diagnostics over the kept draws of many chains: per-chain moments, lagged
// autocovariances, split-R^ and Geyer's effective sample size.  Build-defined: the
// reference runs one chain and has none of this (it thins the chain by hand and judges the
// run by histograms, example_script.py:41-47).
//
// Draws x[t][c][i], t < T, c < C, i < D, element strides (stride_t, stride_c, 1): the
// sample store's buffer, a column slice of a wider slot and every R-th chain of a ladder are
// read where they lie.  split in {1, 2}, n = T / split; segment 0 is draws [0, n), segment
// 1 is [T - n, T); split chain m = s * C + c, M = split * C.  The arithmetic is stated in
// include/binf_hip.h and restated in numpy by tests/diagnostics_ref.py; every multiply and
// add is rounded separately, and every sum has one fixed order:
//   over draws   sequential in t (from 0.0),
//   over chains  sequential inside blocks of 64 consecutive split chains (from 0.0), then
//                sequential over the block sums (from 0.0) -- a function of M only.
//
// Kernels (gfx950, wave64):
//   moments   one thread per (c, i), lanes along i: every draw row is one coalesced read
//             and both halves advance in the same loop -- one pass over the store, HBM-bound.
//   autocov   a workgroup = one block of 64 split chains x a tile of 1..8 dimensions x a tile
//             of DIAG_LT = 16 lags.  A thread owns (chain, dimension) and the 16 lags: it walks
//             its n draws with the next 32 centred draws of the lagged side in registers, 16
//             multiply-adds per load (diag_core.hpp).  The 64 per-chain results meet in LDS and
//             are added in chain order by 16 x tile threads.  The lag tiles of the same draws
//             run on one XCD, so the record comes from HBM about once.
//   summary   block sums of m2 / (n - 1) and of the means (a thread per block and dimension),
//             the grand mean (a thread per dimension), block sums of (mean - g)^2, and the
//             per-dimension tail (rho, pair sums, monotone clamp, tau) with a lane per dimension.
#include "common.hpp"
#include "diag_core.hpp"
#include "diag_draws.hpp"

namespace binf {

// ---------------------------------------------------------------------------------------
// moments
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) diag_moments_kernel(const DiagDraws a, double *mean, double *m2)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= a.C * a.D) return;
    const int64_t c = p <= 0xffffffffLL && a.D <= 0xffffffffLL ? (int64_t)((uint32_t)p / (uint32_t)a.D) : p / a.D;
    const int64_t i = p - c * a.D;
    const double *x0 = a.x + c * a.sc + i;
    const double dn = (double)a.n;
    DiagMoments s0;
    s0.start(x0[0]);
    if (a.split == 2) {
        const double *x1 = x0 + (a.T - a.n) * a.st;
        DiagMoments s1;
        s1.start(x1[0]);
#pragma unroll 4
        for (int64_t t = 0; t < a.n; ++t) {
            s0.add(x0[t * a.st]);
            s1.add(x1[t * a.st]);
        }
        mean[(a.C + c) * a.D + i] = s1.mean(dn);
        m2[(a.C + c) * a.D + i] = s1.m2(dn);
    } else {
#pragma unroll 8
        for (int64_t t = 0; t < a.n; ++t) s0.add(x0[t * a.st]);
    }
    mean[p] = s0.mean(dn);
    m2[p] = s0.m2(dn);
}

// ---------------------------------------------------------------------------------------
// autocovariance
// ---------------------------------------------------------------------------------------
struct DiagAutocovArgs {
    DiagDraws d;
    const double *mean;         // [M x D]
    double *part;               // [nblocks x (K + 1) x D]
    int64_t K;
    int64_t n_blocks, n_dtiles, n_ltiles;
    int32_t dt;                 // dimensions per workgroup: 1, 2, 4 or 8
    int32_t g;                  // chains per pass: min(64, 256 / dt); the workgroup has g * dt threads
};

__global__ void __launch_bounds__(256) diag_autocov_kernel(const DiagAutocovArgs a)
{
    __shared__ double sm[64 * DIAG_LT * 4];                 // g * DIAG_LT * dt = 4096 doubles at most
    const int dt = a.dt, g = a.g;
    // Workgroups are dealt to the 8 XCDs round robin by index, and the lag tiles of one (chain
    // block, dimension tile) read the same draws: index = (chunk of 8 data tiles, lag tile,
    // data tile in the chunk) puts them on ONE XCD next to each other in time, so all but the
    // first find the draws in that XCD's L2.
    const int64_t bid = blockIdx.x;
    const int64_t r = bid % (8 * a.n_ltiles);
    const int64_t lt = r / 8;
    const int64_t tile = bid / (8 * a.n_ltiles) * 8 + r % 8;
    const int64_t dti = tile % a.n_dtiles;
    const int64_t b = tile / a.n_dtiles;
    if (b >= a.n_blocks) return;                            // the last chunk's spare tiles
    const int tid = threadIdx.x;
    const int ml = tid / dt, il = tid - ml * dt;
    const int64_t i = dti * dt + il;
    const int64_t k0 = lt * DIAG_LT;
    const double dn = (double)a.d.n;
    // the threads that add the chains of the block, one per (lag, dimension) of the tile
    const int rj = tid / dt;
    const bool reducer = tid < DIAG_LT * dt;
    double bacc = 0.0;
    for (int pass = 0; pass < DIAG_CHAIN_BLOCK / g; ++pass) {
        const int64_t m = b * DIAG_CHAIN_BLOCK + (int64_t)pass * g + ml;
        if (m < a.d.M && i < a.d.D) {
            const int64_t s = m >= a.d.C ? 1 : 0;
            const int64_t c = m - s * a.d.C;
            const double *x = a.d.x + (s ? (a.d.T - a.d.n) * a.d.st : 0) + c * a.d.sc + i;
            double acc[DIAG_LT];
            diag_autocov_lags(x, a.d.st, a.d.n, a.mean[m * a.d.D + i], k0, acc);
#pragma unroll
            for (int j = 0; j < DIAG_LT; ++j) sm[(ml * DIAG_LT + j) * dt + il] = acc[j] / dn;
        }
        __syncthreads();
        if (reducer && i < a.d.D) {
            const int64_t m0 = b * DIAG_CHAIN_BLOCK + (int64_t)pass * g;
            const int64_t left = a.d.M - m0;
            const int cnt = left < g ? (left < 0 ? 0 : (int)left) : g;
            for (int q = 0; q < cnt; ++q) bacc = bacc + sm[(q * DIAG_LT + rj) * dt + il];
        }
        __syncthreads();
    }
    if (reducer && i < a.d.D && k0 + rj <= a.K) a.part[(b * (a.K + 1) + k0 + rj) * a.d.D + i] = bacc;
}

// ---------------------------------------------------------------------------------------
// summary
// ---------------------------------------------------------------------------------------
struct DiagSummaryArgs {
    const double *mean, *m2, *part;
    double *post_mean, *varplus, *sd, *W, *rhat, *ess, *mcse;
    uint8_t *truncated;
    double *ws;                 // [3 x nblocks x D]: block sums of m2 / (n - 1), mean, (mean - g)^2
    int64_t n, M, D, K, nblocks;
};

// phase 0: block sums of m2 / (n - 1) and of mean; phase 1: of (mean - g)^2, g = post_mean
template <int PHASE>
__global__ void __launch_bounds__(256) diag_block_sums_kernel(const DiagSummaryArgs a)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= a.nblocks * a.D) return;
    const int64_t b = p <= 0xffffffffLL && a.D <= 0xffffffffLL ? (int64_t)((uint32_t)p / (uint32_t)a.D) : p / a.D;
    const int64_t i = p - b * a.D;
    const int64_t m0 = b * DIAG_CHAIN_BLOCK;
    const int cnt = a.M - m0 < DIAG_CHAIN_BLOCK ? (int)(a.M - m0) : DIAG_CHAIN_BLOCK;
    if (PHASE == 0) {
        const double dn1 = (double)(a.n - 1);
        double sw = 0.0, sg = 0.0;
        for (int q = 0; q < cnt; ++q) {
            sw = sw + a.m2[(m0 + q) * a.D + i] / dn1;
            sg = sg + a.mean[(m0 + q) * a.D + i];
        }
        a.ws[p] = sw;
        a.ws[a.nblocks * a.D + p] = sg;
    } else {
        const double g = a.post_mean[i];
        double sb = 0.0;
        for (int q = 0; q < cnt; ++q) {
            const double e = a.mean[(m0 + q) * a.D + i] - g;
            sb = sb + e * e;
        }
        a.ws[2 * a.nblocks * a.D + p] = sb;
    }
}

__global__ void __launch_bounds__(64) diag_grand_mean_kernel(const DiagSummaryArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= a.D) return;
    const double *sg = a.ws + a.nblocks * a.D;
    double s = 0.0;
    for (int64_t b = 0; b < a.nblocks; ++b) s = s + sg[b * a.D + i];
    a.post_mean[i] = s / (double)a.M;
}

__global__ void __launch_bounds__(64) diag_tail_kernel(const DiagSummaryArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= a.D) return;
    const double dn = (double)a.n, dn1 = (double)(a.n - 1), dM = (double)a.M, dM1 = (double)(a.M - 1);
    const double *sw = a.ws, *sb = a.ws + 2 * a.nblocks * a.D;
    double w = 0.0, bn = 0.0;
    for (int64_t b = 0; b < a.nblocks; ++b) {
        w = w + sw[b * a.D + i];
        bn = bn + sb[b * a.D + i];
    }
    const double W = w / dM;
    const double Bn = bn / dM1;
    const double vp = (dn1 / dn) * W + Bn;
    a.W[i] = W;
    a.varplus[i] = vp;
    if (a.sd) a.sd[i] = sqrt(vp);
    a.rhat[i] = sqrt(vp / W);
    if (!a.part) return;
    auto rho = [&](int64_t k) {
        double s = 0.0;
        for (int64_t b = 0; b < a.nblocks; ++b) s = s + a.part[(b * (a.K + 1) + k) * a.D + i];
        const double A = s / dM;
        return 1.0 - (W - (A * dn) / dn1) / vp;
    };
    double sum = 0.0, prev = 0.0;
    bool negative = false;
    for (int64_t j = 0; 2 * j + 1 <= a.K; ++j) {
        const double r0 = rho(2 * j);
        const double r1 = rho(2 * j + 1);
        double P = r0 + r1;
        if (P < 0.0) {
            negative = true;
            break;
        }
        if (j > 0 && prev < P) P = prev;
        sum = sum + P;
        prev = P;
    }
    const double tau = -1.0 + 2.0 * sum;
    const double ess = (dM * dn) / tau;
    a.ess[i] = ess;
    a.mcse[i] = sqrt(vp / ess);
    a.truncated[i] = negative ? 0 : 1;
}

static int64_t diag_blocks(int64_t M) { return (M + DIAG_CHAIN_BLOCK - 1) / DIAG_CHAIN_BLOCK; }

}  // namespace binf

using namespace binf;

extern "C" int32_t binf_chain_moments_f64(const double *draws, int64_t stride_t, int64_t stride_c,
                                          int64_t stride_i, int64_t T, int64_t C, int64_t D,
                                          int32_t split, double *mean, double *m2, void *stream)
{
    const char *what = "chain_moments";
    DiagDraws d;
    const int32_t rc = diag_draws(what, draws, stride_t, stride_c, stride_i, T, C, D, split, d);
    if (rc) return rc;
    if (!mean || !m2) return fail(BINF_E_ARG, "%s: null buffer", what);
    const int64_t MD = d.M * D;
    if (overlap_f64(mean, MD, draws, d.span) || overlap_f64(m2, MD, draws, d.span))
        return fail(BINF_E_ALIAS, "%s: an output overlaps the draws", what);
    if (overlap_f64(mean, MD, m2, MD)) return fail(BINF_E_ALIAS, "%s: mean overlaps m2", what);
    const int64_t blocks = (C * D + 255) / 256;
    if (blocks > 0x7fffffffLL) return fail(BINF_E_UNSUPPORTED, "%s: C * D too large for one launch", what);
    diag_moments_kernel<<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(d, mean, m2);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what);
    return 0;
}

extern "C" int64_t binf_chain_autocov_workspace_bytes(int64_t M, int64_t D, int64_t max_lag)
{
    if (M < 1 || D < 1 || max_lag < 0) return 0;
    const __int128 need = (__int128)diag_blocks(M) * (max_lag + 1) * D * 8;
    return need > ((__int128)1 << 62) ? 0 : (int64_t)need;
}

extern "C" int32_t binf_chain_autocov_f64(const double *draws, int64_t stride_t, int64_t stride_c,
                                          int64_t stride_i, int64_t T, int64_t C, int64_t D,
                                          int32_t split, const double *mean, int64_t max_lag,
                                          void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *what = "chain_autocov";
    DiagAutocovArgs a = {};
    const int32_t rc = diag_draws(what, draws, stride_t, stride_c, stride_i, T, C, D, split, a.d);
    if (rc) return rc;
    if (max_lag < 0 || max_lag > a.d.n - 1)
        return fail(BINF_E_ARG, "%s: max_lag %lld outside [0, n - 1 = %lld]", what, (long long)max_lag,
                    (long long)(a.d.n - 1));
    if (!mean) return fail(BINF_E_ARG, "%s: null buffer", what);
    const int64_t need = binf_chain_autocov_workspace_bytes(a.d.M, D, max_lag);
    if (need == 0) return fail(BINF_E_UNSUPPORTED, "%s: workspace size overflows", what);
    if (!workspace || workspace_bytes < need)
        return fail(BINF_E_ARG, "%s: needs %lld bytes of workspace (binf_chain_autocov_workspace_bytes), "
                    "got %lld", what, (long long)need, (long long)workspace_bytes);
    const int64_t MD = a.d.M * D;
    if (overlap_f64(workspace, need / 8, draws, a.d.span) || overlap_f64(workspace, need / 8, mean, MD))
        return fail(BINF_E_ALIAS, "%s: the workspace overlaps an input", what);
    a.mean = mean;
    a.part = (double *)workspace;
    a.K = max_lag;
    a.dt = D >= 8 ? 8 : (D > 2 ? 4 : (int32_t)D);
    a.g = 256 / a.dt < DIAG_CHAIN_BLOCK ? 256 / a.dt : DIAG_CHAIN_BLOCK;
    a.n_dtiles = (D + a.dt - 1) / a.dt;
    a.n_ltiles = (max_lag + DIAG_LT) / DIAG_LT;
    a.n_blocks = diag_blocks(a.d.M);
    const __int128 blocks = ((__int128)a.n_blocks * a.n_dtiles + 7) / 8 * 8 * a.n_ltiles;
    if (blocks > 0x7fffffffLL) return fail(BINF_E_UNSUPPORTED, "%s: too many tiles for one launch", what);
    diag_autocov_kernel<<<dim3((unsigned)blocks), a.g * a.dt, 0, (hipStream_t)stream>>>(a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what);
    return 0;
}

extern "C" int64_t binf_diag_summary_workspace_bytes(int64_t M, int64_t D)
{
    if (M < 1 || D < 1) return 0;
    const __int128 need = (__int128)3 * diag_blocks(M) * D * 8;
    return need > ((__int128)1 << 62) ? 0 : (int64_t)need;
}

extern "C" int32_t binf_diag_summary_f64(const double *mean, const double *m2, const double *autocov,
                                         int64_t n, int64_t M, int64_t D, int64_t max_lag,
                                         double *post_mean, double *varplus, double *sd, double *W,
                                         double *rhat, double *ess, double *mcse, uint8_t *truncated,
                                         void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *what = "diag_summary";
    if (D < 1) return fail(BINF_E_ARG, "%s: D >= 1 required", what);
    if (n < 2) return fail(BINF_E_ARG, "%s: n >= 2 required", what);
    if (M < 2)
        return fail(BINF_E_ARG, "%s: M >= 2 split chains required (one chain has no between-chain "
                    "variance; its moments stay available)", what);
    if (autocov && (max_lag < 0 || max_lag > n - 1))
        return fail(BINF_E_ARG, "%s: max_lag %lld outside [0, n - 1 = %lld]", what, (long long)max_lag,
                    (long long)(n - 1));
    if (!mean || !m2 || !post_mean || !varplus || !W || !rhat || (autocov && (!ess || !mcse || !truncated)))
        return fail(BINF_E_ARG, "%s: null buffer", what);
    if ((__int128)M * D > ((__int128)1 << 60)) return fail(BINF_E_UNSUPPORTED, "%s: M * D too large", what);
    const int64_t need = binf_diag_summary_workspace_bytes(M, D);
    if (!workspace || workspace_bytes < need)
        return fail(BINF_E_ARG, "%s: needs %lld bytes of workspace (binf_diag_summary_workspace_bytes), "
                    "got %lld", what, (long long)need, (long long)workspace_bytes);
    const int64_t nblocks = diag_blocks(M);
    const int64_t part_bytes = autocov ? binf_chain_autocov_workspace_bytes(M, D, max_lag) : 0;
    if (autocov && part_bytes == 0) return fail(BINF_E_UNSUPPORTED, "%s: autocovariance size overflows", what);
    struct Buf { const void *p; int64_t bytes; };
    const Buf in[3] = {{mean, M * D * 8}, {m2, M * D * 8}, {autocov, part_bytes}};
    const Buf out[9] = {{post_mean, D * 8}, {varplus, D * 8}, {sd, D * 8}, {W, D * 8}, {rhat, D * 8},
                        {autocov ? ess : nullptr, D * 8}, {autocov ? mcse : nullptr, D * 8},
                        {autocov ? truncated : nullptr, D}, {workspace, need}};
    for (int o = 0; o < 9; ++o) {
        for (int q = 0; q < 3; ++q)
            if (overlap_bytes(out[o].p, out[o].bytes, in[q].p, in[q].bytes))
                return fail(BINF_E_ALIAS, "%s: an output or the workspace overlaps an input", what);
        for (int q = o + 1; q < 9; ++q)
            if (overlap_bytes(out[o].p, out[o].bytes, out[q].p, out[q].bytes))
                return fail(BINF_E_ALIAS, "%s: outputs overlap each other or the workspace", what);
    }
    const int64_t blocks = (nblocks * D + 255) / 256;
    if (blocks > 0x7fffffffLL) return fail(BINF_E_UNSUPPORTED, "%s: M * D too large for one launch", what);
    DiagSummaryArgs a = {};
    a.mean = mean; a.m2 = m2; a.part = autocov;
    a.post_mean = post_mean; a.varplus = varplus; a.sd = sd; a.W = W; a.rhat = rhat;
    a.ess = ess; a.mcse = mcse; a.truncated = truncated;
    a.ws = (double *)workspace;
    a.n = n; a.M = M; a.D = D; a.K = max_lag; a.nblocks = nblocks;
    hipStream_t st = (hipStream_t)stream;
    const unsigned dblocks = (unsigned)((D + 63) / 64);
    diag_block_sums_kernel<0><<<dim3((unsigned)blocks), 256, 0, st>>>(a);
    diag_grand_mean_kernel<<<dim3(dblocks), 64, 0, st>>>(a);
    diag_block_sums_kernel<1><<<dim3((unsigned)blocks), 256, 0, st>>>(a);
    diag_tail_kernel<<<dim3(dblocks), 64, 0, st>>>(a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what);
    return 0;
}
