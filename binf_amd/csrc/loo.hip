// Model comparison by predictive fit: the pointwise log-likelihood record of a Gaussian error
// model, and Pareto-smoothed importance-sampling leave-one-out (PSIS-LOO; Vehtari, Gelman &
// Gabry 2017; Vehtari, Simpson, Gelman, Yao & Gabry 2024) with WAIC from the same walk.  The
// contract, with every formula and the order of every sum, is in include/binf_hip.h; the host
// restatement is tests/loo_ref.py.
//
//   record:  out[s, i] = predictive_term(mock[s, i], ys[i], precision[s], 0.5 log precision[s])
//   PSIS:    per observation i, from its S log-likelihoods in ascending order (what
//            binf_rank_normalise_f64 writes as sorted [N x S]; nothing here sorts): the M
//            largest importance ratios are replaced by the order statistics of a generalised
//            Pareto fit to them (Zhang & Stephens 2009, m = 30 + sqrt(M) profile candidates),
//            then elpd_loo, khat, n_eff, lppd and p_waic.
//
// Layout.
//
// The record is element-wise and memory-bound (16 bytes per element): a workgroup owns
// LOO_ROWS rows, its first lanes take 0.5 log(precision) ONCE per row into LDS, and its 256
// lanes then walk the columns, 2 KiB per row and instruction, each ys[i] loaded once for the
// LOO_ROWS rows.
//
// PSIS is three launches, because two different shapes of work hide in it:
//   * psis_fit_kernel, one 256-thread workgroup per observation.  The fit is small and
//     latency-bound: M <= 6144 exceedances (M = 679 at S = 51200) live in LDS, 8 M bytes of
//     dynamic LDS, so that a workgroup of the example's size asks for 8 KiB and eight of them
//     share a CU (32 waves), while the largest supported S (2^22, 48 KiB) still leaves three.
//     Candidates go round the four waves; a candidate's sum over the tail is lane-strided over
//     the wave's 64 lanes and joined by the xor butterfly, which is the balanced tree over
//     neighbours and leaves the same bits in every lane -- no LDS traffic and no barrier per
//     candidate.  Consecutive lanes read consecutive doubles (ds_read_b64, conflict-free).  The
//     m weights are m^2 <= 11664 exponentials, one candidate per thread; the few sums over m
//     that follow are formed by EVERY thread from LDS broadcasts instead of by one thread and a
//     barrier.  The same workgroup takes the column mean (one streaming pass, no
//     transcendental) and the tail's share of the weight sums.
//   * psis_body_kernel, one workgroup per observation and per LOO_CHUNK = 8192 column
//     elements: the S - M raw weights and the lppd terms, two FP64 exponentials per element,
//     which is where the time goes (8.4e8 elements at the example's size).  The chunk length
//     is a constant, NOT a function of the grid as predict.hip's is: the contract makes every
//     output independent of how many observations share the launch, so the cut may depend on
//     S alone.  At N = 150, S = 51200 that is 1050 workgroups instead of 150 on 256 CUs; at
//     N = 16384 the chunks cost nothing (each still streams 64 KiB).  The raw weight of a body
//     draw times its likelihood is exp(a[0]) exactly, so the numerator's body is one product,
//     not a third exponential per element.
//   * psis_finish_kernel, one thread per observation: chunks joined in ascending order, the
//     four logarithms, the outputs.
// Partials and the per-observation header travel through the caller's workspace across the
// kernel boundaries; there are no atomics and no in-launch hand-offs.  Every sum has one fixed
// order (header), so every output is a function of the column's values alone.
//
// exp is np_exp (gauss_common.hpp: the device library's algorithm on the whole real line), as
// in predict.hip; log, log1p, expm1 and sqrt are the device library's.
#include "common.hpp"
#include "gauss_common.hpp"
#include "gauss_error_term.hpp"

namespace binf {

constexpr int LOO_T = 256;                   // threads per workgroup
constexpr int LOO_ROWS = 4;                  // record rows per workgroup
constexpr int LOO_CHUNK = 8192;              // column elements per body workgroup
constexpr int64_t LOO_MAX_S = 1LL << 22;     // tail length 6144 there: 48 KiB of LDS
constexpr int LOO_MAX_CAND = 30 + 78;        // 30 + floor(sqrt(6144))
constexpr int LOO_HDR = 8;                   // doubles per observation in front of the partials
constexpr int LOO_PART = 4;                  // sums per observation and chunk

__device__ inline bool finite_f64(double x) { return __builtin_fabs(x) < __builtin_inf(); }

// balanced tree over the 64 lanes of a wave, neighbours first; every lane ends with the same
// bits (IEEE addition is commutative)
__device__ inline double wave_tree_sum(double v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = v + shfl_xor_f64(v, m);
    return v;
}

__device__ inline double wave_nan_max(double v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = nan_max(v, shfl_xor_f64(v, m));
    return v;
}

// the same tree over the 256 threads of the workgroup: (w0 + w1) + (w2 + w3) of the waves
__device__ inline double block_tree_sum(double v, double *red)
{
    v = wave_tree_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ inline double block_nan_max(double v, double *red)
{
    v = wave_nan_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return nan_max(nan_max(red[0], red[1]), nan_max(red[2], red[3]));
}

__global__ void __launch_bounds__(LOO_T)
gauss_pointwise_loglik_kernel(const double *mock, const double *precision, const double *ys,
                              double *out, int64_t S, int64_t N, double half_log_2pi)
{
    __shared__ double pr[LOO_ROWS], hl[LOO_ROWS];
    const int tid = threadIdx.x;
    const int64_t s0 = (int64_t)blockIdx.x * LOO_ROWS;
    const int nr = (S - s0 < LOO_ROWS) ? (int)(S - s0) : LOO_ROWS;
    if (tid < nr) {
        const double p = precision[s0 + tid];
        pr[tid] = p;
        hl[tid] = 0.5 * log(p);                  // once per row
    }
    __syncthreads();
    for (int64_t i = tid; i < N; i += LOO_T) {
        const double y = ys[i];
        for (int r = 0; r < nr; ++r) {
            const int64_t e = (s0 + r) * N + i;
            out[e] = predictive_term(mock[e], y, pr[r], hl[r], half_log_2pi);
        }
    }
}

// hdr[i] = { valid, khat, sh1, sh2, abar, T1, T1q, T2 }
__global__ void __launch_bounds__(LOO_T)
psis_fit_kernel(const double *sorted, int64_t S, int M, int m, int q, double *hdr)
{
    extern __shared__ double xs[];               // [max(M, 1)]: exceedances, then the tail's log weights
    __shared__ double red[4];
    __shared__ double cb[LOO_MAX_CAND], cL[LOO_MAX_CAND], cw[LOO_MAX_CAND];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double *a = sorted + (int64_t)blockIdx.x * S;
    double *h = hdr + (int64_t)blockIdx.x * LOO_HDR;
    const double inf = __builtin_inf();
    const double a0 = a[0], aL = a[S - 1];
    if (!(finite_f64(a0) && finite_f64(aL))) {   // the whole workgroup alike
        if (tid == 0) h[0] = 0.0;
        return;
    }
    // the column mean, for the two-pass variance of the body kernel
    double acc = 0.0;
    for (int64_t j = tid; j < S; j += LOO_T) acc += a[j];
    const double abar = block_tree_sum(acc, red) / (double)S;

    const double lc = a0 - a[M];
    const double ec = np_exp(lc);
    for (int t = 1 + tid; t <= M; t += LOO_T) xs[t - 1] = np_exp(a0 - a[M - t]) - ec;
    __syncthreads();
    const double xM = M > 0 ? xs[M - 1] : 0.0;
    const bool smooth = M >= 5 && xM > 0.0 && xM < inf;
    double khat = inf;
    if (smooth) {
        const double d3 = 3.0 * xs[q - 1], ixM = 1.0 / xM, dM = (double)M;
        for (int j = wave; j < m; j += LOO_T / 64) {          // candidate j + 1
            const double b = (1.0 - sqrt((double)m / ((double)(j + 1) - 0.5))) / d3 + ixM;
            double s = 0.0;
            for (int t = lane; t < M; t += 64) s += log1p(-b * xs[t]);
            const double k = wave_tree_sum(s) / dM;
            if (lane == 0) {
                cb[j] = b;
                cL[j] = dM * (log(-b / k) - k - 1.0);
            }
        }
        __syncthreads();
        if (tid < m) {
            const double Lj = cL[tid];
            double s = 0.0;
            for (int l = 0; l < m; ++l) s += np_exp(cL[l] - Lj);
            cw[tid] = 1.0 / s;
        }
        __syncthreads();
        // A weight below the cut is dropped; one that falls on the other side of it on another
        // implementation moves bhat by about 1e-15 of itself.
        const double cut = 10.0 * 0x1p-52;
        double wsum = 0.0;
        for (int l = 0; l < m; ++l) {
            const double w = cw[l];
            if (!(w < cut)) wsum += w;
        }
        double bhat = 0.0;
        for (int l = 0; l < m; ++l) {
            const double w = cw[l];
            if (!(w < cut)) bhat += cb[l] * (w / wsum);
        }
        double s = 0.0;
        for (int t = lane; t < M; t += 64) s += log1p(-bhat * xs[t]);
        const double kp = wave_tree_sum(s) / dM;
        const double sigma = -kp / bhat;
        khat = (dM * kp + 5.0) / (dM + 10.0);
        __syncthreads();                                      // every wave has read the exceedances
        for (int t = 1 + tid; t <= M; t += LOO_T) {
            const double p = ((double)t - 0.5) / dM;
            const double qt = sigma * expm1(-khat * log1p(-p)) / khat;
            const double lw = log(qt + ec);
            xs[M - t] = (lw > 0.0) ? 0.0 : lw;                // min(lw, 0); a NaN stays
        }
    } else {
        __syncthreads();                                      // xs[M - 1] has been read
        for (int j = tid; j < M; j += LOO_T) xs[j] = a0 - a[j];
    }
    __syncthreads();
    // xs[j] is now the log weight of sorted draw j < M; the body's are a0 - a[j], largest at j = M
    double m1 = lc, m2 = a0;
    for (int j = tid; j < M; j += LOO_T) {
        const double lw = xs[j];
        m1 = nan_max(m1, lw);
        m2 = nan_max(m2, lw + a[j]);
    }
    const double sh1 = block_nan_max(m1, red);
    const double sh2 = block_nan_max(m2, red);
    double t1 = 0.0, t1q = 0.0, t2 = 0.0;
    for (int j = tid; j < M; j += LOO_T) {
        const double lw = xs[j];
        const double e = np_exp(lw - sh1);
        t1 += e;
        t1q += e * e;
        t2 += np_exp((lw + a[j]) - sh2);
    }
    const double T1 = block_tree_sum(t1, red);
    const double T1q = block_tree_sum(t1q, red);
    const double T2 = block_tree_sum(t2, red);
    if (tid == 0) {
        h[0] = 1.0;
        h[1] = khat;
        h[2] = sh1;
        h[3] = sh2;
        h[4] = abar;
        h[5] = T1;
        h[6] = T1q;
        h[7] = T2;
    }
}

// part[i][c] = { sum w, sum w^2, sum exp(a - a[S-1]), sum (a - abar)^2 } over chunk c; w = 0 for j < M
__global__ void __launch_bounds__(LOO_T)
psis_body_kernel(const double *sorted, int64_t S, int M, const double *hdr, double *part, int nchunks)
{
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const int64_t i = blockIdx.x;
    const int c = blockIdx.y;
    const double *a = sorted + i * S;
    const double *h = hdr + i * LOO_HDR;
    if (h[0] == 0.0) return;                     // the whole workgroup alike
    const double a0 = a[0], aL = a[S - 1], sh1 = h[2], abar = h[4];
    const int64_t lo = (int64_t)c * LOO_CHUNK;
    const int64_t hi = (lo + LOO_CHUNK < S) ? lo + LOO_CHUNK : S;
    double s1 = 0.0, s1q = 0.0, s3 = 0.0, s4 = 0.0;
    for (int64_t j = lo + tid; j < hi; j += LOO_T) {
        const double v = a[j];
        const double e = (j < M) ? 0.0 : np_exp((a0 - v) - sh1);
        s1 += e;
        s1q += e * e;
        s3 += np_exp(v - aL);
        const double d = v - abar;
        s4 += d * d;
    }
    const double r1 = block_tree_sum(s1, red);
    const double r1q = block_tree_sum(s1q, red);
    const double r3 = block_tree_sum(s3, red);
    const double r4 = block_tree_sum(s4, red);
    if (tid == 0) {
        double *o = part + (i * nchunks + c) * LOO_PART;
        o[0] = r1;
        o[1] = r1q;
        o[2] = r3;
        o[3] = r4;
    }
}

struct PsisOut {
    double *elpd_loo, *khat, *n_eff, *lppd, *p_waic;
    int32_t *tail_len;
};

__global__ void psis_finish_kernel(const double *sorted, int64_t S, int64_t N, int M, const double *hdr,
                                   const double *part, int nchunks, const PsisOut o)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const double *h = hdr + i * LOO_HDR;
    o.tail_len[i] = M;
    if (h[0] == 0.0) {
        const double nan = __builtin_nan("");
        o.elpd_loo[i] = nan;
        o.khat[i] = nan;
        o.n_eff[i] = nan;
        o.lppd[i] = nan;
        o.p_waic[i] = nan;
        return;
    }
    const double a0 = sorted[i * S], aL = sorted[i * S + S - 1];
    const double sh1 = h[2], sh2 = h[3];
    double s1 = h[5], s1q = h[6], s3 = 0.0, s4 = 0.0;
    for (int c = 0; c < nchunks; ++c) {
        const double *p = part + (i * nchunks + c) * LOO_PART;
        s1 += p[0];
        s1q += p[1];
        s3 += p[2];
        s4 += p[3];
    }
    const double s2 = h[7] + (double)(S - M) * np_exp(a0 - sh2);
    o.elpd_loo[i] = (sh2 - sh1) + (log(s2) - log(s1));
    o.khat[i] = h[1];
    o.n_eff[i] = (s1 * s1) / s1q;
    o.lppd[i] = aL + (log(s3) - log((double)S));
    o.p_waic[i] = s4 / (double)(S - 1);
}

// out[2 r] = sum_i d[r][i], out[2 r + 1] = sum_i (d[r][i] - out[2 r] / N)^2, d = x - y (or x);
// workgroup R: out[2 R] = the number of khat[i] > threshold
__global__ void __launch_bounds__(LOO_T)
pointwise_totals_kernel(const double *x, const double *y, int64_t R, int64_t N, const double *khat,
                        double threshold, double *out)
{
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x;
    if (r == R) {
        double n = 0.0;
        for (int64_t i = tid; i < N; i += LOO_T) n += (khat[i] > threshold) ? 1.0 : 0.0;
        n = block_tree_sum(n, red);
        if (tid == 0) out[2 * R] = n;
        return;
    }
    const double *xr = x + r * N, *yr = y ? y + r * N : nullptr;
    double s = 0.0;
    for (int64_t i = tid; i < N; i += LOO_T) s += yr ? xr[i] - yr[i] : xr[i];
    const double sum = block_tree_sum(s, red);
    const double mean = sum / (double)N;
    double ss = 0.0;
    for (int64_t i = tid; i < N; i += LOO_T) {
        const double d = (yr ? xr[i] - yr[i] : xr[i]) - mean;
        ss += d * d;
    }
    ss = block_tree_sum(ss, red);
    if (tid == 0) {
        out[2 * r] = sum;
        out[2 * r + 1] = ss;
    }
}

}  // namespace binf

using namespace binf;

// M = min(floor(S / 5), ceil(3 sqrt(S))), m = 30 + floor(sqrt(M)), q = floor(M / 4 + 0.5), in
// integers: ceil(3 sqrt(S)) is the smallest c with c^2 >= 9 S
static void psis_plan(int64_t S, int *M, int *m, int *q)
{
    int64_t c = 0;
    while (c * c < 9 * S) ++c;                   // at most 6144 steps
    const int64_t fifth = S / 5;
    const int64_t Mv = fifth < c ? fifth : c;
    int64_t r = 0;
    while ((r + 1) * (r + 1) <= Mv) ++r;
    *M = (int)Mv;
    *m = 30 + (int)r;
    *q = (int)((Mv + 2) / 4);
}

static int64_t psis_chunks(int64_t S) { return (S + LOO_CHUNK - 1) / LOO_CHUNK; }

extern "C" int32_t binf_gauss_pointwise_loglik_f64(const double *mock, const double *precision,
                                                   const double *ys, double *out, int64_t S,
                                                   int64_t N, double half_log_2pi, void *stream)
{
    if (S < 0 || N < 0) return fail(BINF_E_ARG, "gauss_pointwise_loglik: need S>=0, N>=0");
    if (S == 0 || N == 0) return 0;
    if (!mock || !precision || !ys || !out)
        return fail(BINF_E_ARG, "gauss_pointwise_loglik: null buffer");
    const int64_t blocks = (S + LOO_ROWS - 1) / LOO_ROWS;
    if (blocks > 0x7fffffffLL || N > (1LL << 53) / S)
        return fail(BINF_E_UNSUPPORTED, "gauss_pointwise_loglik: a record of %lld x %lld is too large",
                    (long long)S, (long long)N);
    if (overlap_f64(out, S * N, mock, S * N) || overlap_f64(out, S * N, precision, S) ||
        overlap_f64(out, S * N, ys, N))
        return fail(BINF_E_ALIAS, "gauss_pointwise_loglik: out overlaps an input");
    gauss_pointwise_loglik_kernel<<<dim3((unsigned)blocks), LOO_T, 0, (hipStream_t)stream>>>(
        mock, precision, ys, out, S, N, half_log_2pi);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "gauss_pointwise_loglik launch");
    return 0;
}

extern "C" int64_t binf_psis_loo_workspace_bytes(int64_t S, int64_t N)
{
    if (S < 2 || S > LOO_MAX_S || N < 1 || N > 0x7fffffffLL) return 0;
    return N * (LOO_HDR + LOO_PART * psis_chunks(S)) * (int64_t)sizeof(double);
}

extern "C" int32_t binf_psis_loo_f64(const double *sorted_ll, int64_t S, int64_t N, double *elpd_loo,
                                     double *khat, double *n_eff, double *lppd, double *p_waic,
                                     int32_t *tail_len, void *workspace, int64_t workspace_bytes,
                                     void *stream)
{
    if (S < 2 || N < 1)
        return fail(BINF_E_ARG, "psis_loo: need S>=2 draws and N>=1 observations (got %lld, %lld)",
                    (long long)S, (long long)N);
    if (S > LOO_MAX_S || N > 0x7fffffffLL)
        return fail(BINF_E_UNSUPPORTED, "psis_loo: S <= 2^22 draws (the tail lives in LDS) and "
                    "N < 2^31 observations per call (got %lld, %lld)", (long long)S, (long long)N);
    if (!sorted_ll || !elpd_loo || !khat || !n_eff || !lppd || !p_waic || !tail_len)
        return fail(BINF_E_ARG, "psis_loo: null buffer");
    const int64_t need = binf_psis_loo_workspace_bytes(S, N);
    if (!workspace || workspace_bytes < need)
        return fail(BINF_E_ARG, "psis_loo: needs %lld bytes of workspace (binf_psis_loo_workspace_bytes), "
                    "got %lld", (long long)need, (long long)workspace_bytes);
    if (((uintptr_t)workspace & 7) != 0)
        return fail(BINF_E_ARG, "psis_loo: the workspace is not 8-byte aligned");
    // tail_len is int32: N int32 values cover (N + 1) / 2 doubles
    const void *bufs[7] = {elpd_loo, khat, n_eff, lppd, p_waic, tail_len, workspace};
    const int64_t lens[7] = {N, N, N, N, N, (N + 1) / 2, need / 8};
    for (int u = 0; u < 7; ++u) {
        if (overlap_f64(bufs[u], lens[u], sorted_ll, S * N))
            return fail(BINF_E_ALIAS, "psis_loo: an output or the workspace overlaps sorted_ll");
        for (int v = u + 1; v < 7; ++v)
            if (overlap_f64(bufs[u], lens[u], bufs[v], lens[v]))
                return fail(BINF_E_ALIAS, "psis_loo: outputs and workspace overlap each other");
    }
    int M, m, q;
    psis_plan(S, &M, &m, &q);
    const int nchunks = (int)psis_chunks(S);
    double *hdr = (double *)workspace, *part = hdr + N * LOO_HDR;
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)(M > 0 ? M : 1) * sizeof(double);
    psis_fit_kernel<<<dim3((unsigned)N), LOO_T, lds, st>>>(sorted_ll, S, M, m, q, hdr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "psis_loo fit launch");
    psis_body_kernel<<<dim3((unsigned)N, (unsigned)nchunks), LOO_T, 0, st>>>(sorted_ll, S, M, hdr, part, nchunks);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "psis_loo body launch");
    PsisOut o;
    o.elpd_loo = elpd_loo; o.khat = khat; o.n_eff = n_eff; o.lppd = lppd; o.p_waic = p_waic;
    o.tail_len = tail_len;
    psis_finish_kernel<<<dim3((unsigned)((N + 255) / 256)), 256, 0, st>>>(sorted_ll, S, N, M, hdr, part,
                                                                         nchunks, o);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "psis_loo finish launch");
    return 0;
}

extern "C" int32_t binf_pointwise_totals_f64(const double *x, const double *y, int64_t R, int64_t N,
                                             const double *khat, double threshold, double *out,
                                             void *stream)
{
    if (R < 1 || N < 1) return fail(BINF_E_ARG, "pointwise_totals: need R>=1 rows of N>=1 values");
    if (R > 65536 || N > (1LL << 53) / R)
        return fail(BINF_E_UNSUPPORTED, "pointwise_totals: %lld rows x %lld values is too large",
                    (long long)R, (long long)N);
    if (!x || !out) return fail(BINF_E_ARG, "pointwise_totals: null buffer");
    const int64_t no = 2 * R + (khat ? 1 : 0);
    if (overlap_f64(out, no, x, R * N) || overlap_f64(out, no, y, R * N) || overlap_f64(out, no, khat, N))
        return fail(BINF_E_ALIAS, "pointwise_totals: out overlaps an input");
    pointwise_totals_kernel<<<dim3((unsigned)(R + (khat ? 1 : 0))), LOO_T, 0, (hipStream_t)stream>>>(
        x, y, R, N, khat, threshold, out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "pointwise_totals launch");
    return 0;
}
