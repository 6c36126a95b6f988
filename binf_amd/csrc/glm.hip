// Generalised linear models on a linear forward model (mock = Theta . A, A [K x N]):
// the binomial-logit and Poisson-log error terms (glm_term.hpp) element-wise, and fused
// between the two f64 MFMA products of the log-prob, the gradient and the leapfrog.
// gfx950 (MI355X), wave64.
//
// Reference lines replaced (the reference has no GLM; these are the lines a user's
// error model would run through):
//   AbstractForwardModel._evaluate of a linear model   binf/model/forwardmodels.py:23-28
//   Likelihood._evaluate_log_prob / _evaluate_gradient binf/pdf/likelihoods.py:141-155
//   HMCSampler._leapfrog                               binf/samplers/hmc.py:92-125
//
// The tile loops are those of linear_chi2_kernel (linear.hip) and poly_grad_mfma_kernel
// (poly.hip), general variants: the error term adds an exp, a log1p and a division per
// element on the VALU, so the whole-tile variants' savings are not what bounds these.
//
// Summation orders.  Log-prob: as binf_linear_gauss_logp_f64 -- pieces of PIECE_TILES
// tiles, inside a piece per lane over n = lk, lk + 4, ..., the four lane partials as
// (0 + 1) + (2 + 3), pieces joined in piece order, log_norm added last; a function of
// (K, N) alone.  Gradient: as binf_poly_gauss_grad_f64 -- data splits that follow from
// (C, N), partial sums joined in split order.
//
// The negative binomial (FAMILY = BINF_GLM_NEGBIN_LOG, entry points of its own) runs the
// same templates: a lane holds one chain, so the chain's lam = log(phi) and phi = exp(lam)
// are two registers per chain tile, loaded and computed at the top (one exp per chain and
// launch); the term is the binomial one at z = eta - lam with m = y + phi, two more
// roundings per element and no new transcendental; the trials row of sD is unused; the
// log-prob adds the chain's log_norm_chain[c] (the count term of negbin.hip) last, in the
// finishing launch too.  The orders above are unchanged.
#include "common.hpp"
#include "glm_term.hpp"

#include <math.h>

namespace binf {

typedef double glm_v4d __attribute__((ext_vector_type(4)));

constexpr int GLM_LDA = 17;              // padded row length of the staged A tile (doubles)
constexpr int GLM_PIECE_TILES = 64;      // as linear.hip: 1024 data points per piece

// ---------------------------------------------------------------------------
// element-wise: the error models as written, and the pointwise record
// ---------------------------------------------------------------------------
template <int FAMILY>
__global__ void __launch_bounds__(256)
glm_pointwise_kernel(const double *mock, const double *ys, const double *trials,
                     const double *offset, const double *lconst, double *out_ll,
                     double *out_grad, int64_t total, int64_t N)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * 256) {
        const int64_t n = i % N;
        const double eta = glm_eta<FAMILY>(mock[i], offset ? offset[n] : 0.0);
        const double y = ys[n];
        const double m = trials ? trials[n] : 1.0;
        double ll = 0.0, g = 0.0;
        if (out_ll && out_grad) glm_term<FAMILY, true, true>(eta, y, m, ll, g);
        else if (out_ll)        glm_term<FAMILY, true, false>(eta, y, m, ll, g);
        else                    glm_term<FAMILY, false, true>(eta, y, m, ll, g);
        if (out_ll) out_ll[i] = lconst ? ll + lconst[n] : ll;
        if (out_grad) out_grad[i] = g;
    }
}

// The negative binomial's record: row s of mock under lam[s].  phi = exp(lam) as in the
// fused kernels.  out_ll = ll, then + prefix[s][prefix_index[n]] (the count term's
// sum_{j<y_n} log(phi_s + j), negbin.hip), then + lconst[n], each where given and in that
// order; -inf for a lam outside the regular range.  An index outside [0, J) is clamped.
__global__ void __launch_bounds__(256)
negbin_pointwise_kernel(const double *mock, const double *ys, const double *offset,
                        const double *lam, const double *prefix, const int32_t *prefix_index,
                        const double *lconst, double *out_ll, double *out_grad, int64_t total,
                        int64_t N, int64_t J)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * 256) {
        const int64_t n = i % N, s = i / N;
        const double eta = glm_eta<BINF_GLM_NEGBIN_LOG>(mock[i], offset ? offset[n] : 0.0);
        const double y = ys[n];
        const double l = lam[s];
        const double lc = negbin_lam(l);
        const double phi = exp(lc);
        double ll = 0.0, g = 0.0;
        if (out_ll && out_grad) glm_term_chain<BINF_GLM_NEGBIN_LOG, true, true>(eta, y, 1.0, lc, phi, ll, g);
        else if (out_ll)        glm_term_chain<BINF_GLM_NEGBIN_LOG, true, false>(eta, y, 1.0, lc, phi, ll, g);
        else                    glm_term_chain<BINF_GLM_NEGBIN_LOG, false, true>(eta, y, 1.0, lc, phi, ll, g);
        if (out_ll) {
            if (prefix) {
                int64_t k = prefix_index[n];
                k = k < 0 ? 0 : (k >= J ? J - 1 : k);
                ll = ll + prefix[s * J + k];
            }
            if (lconst) ll = ll + lconst[n];
            out_ll[i] = negbin_regular(l) ? ll : -INFINITY;
        }
        if (out_grad) out_grad[i] = g;
    }
}

// ---------------------------------------------------------------------------
// fused log-prob: linear_chi2_kernel's loop with the GLM term in place of the residual
// ---------------------------------------------------------------------------
struct GlmLogpArgs {
    const double *theta;     // [C x K]
    const double *A;         // [K x N]
    const double *ys;        // [N]
    const double *trials;    // [N] or null (1.0)
    const double *offset;    // [N] or null (0.0)
    const double *lam;       // negative binomial: log dispersion [C]; else unused
    const double *lnc;       // negative binomial: log_norm_chain [C]; else unused
    double log_norm;
    double *out;             // finish: log-prob [C]; else partial sums [pieces x C]
    int64_t C;
    int32_t K;
    int32_t N;
    int32_t finish;          // 1: one piece, log_norm is added here
};

// KS forward k-steps on the MFMA pipe, KV trailing coefficients on the VALU, CT 16-chain
// tiles per wave.  Staging as in the gradient kernel below: rows of the tile beyond K and
// columns beyond N are written as zeros.  sD holds y, m and the offset of the tile's 16
// data points beside the A tile.  One tile body, the LDS buffer chosen by index: the
// error term is what the loop spends its time on, and a body per buffer (as the
// whole-tile Gaussian kernel has) doubles the live transcendental state for nothing.
template <int FAMILY, int KS, int KV, int CT>
__global__ void __launch_bounds__(256) glm_logp_kernel(const GlmLogpArgs a)
{
    constexpr int KB = 4 * KS;
    constexpr int ROWS = KB + KV;
    constexpr int PASSES = (ROWS + 15) / 16;
    __shared__ double sA[2][ROWS][GLM_LDA];
    __shared__ double sD[2][3][16];

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
    double ll[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        chain[c] = ((int64_t)blockIdx.y * 4 + wave) * (16 * CT) + 16 * c + lc;
        cvalid[c] = chain[c] < a.C;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int k = 4 * s + lk;
            th[c][s] = (cvalid[c] && k < K) ? a.theta[chain[c] * K + k] : 0.0;
        }
#pragma unroll
        for (int v = 0; v < KV; ++v)
            thv[c][v] = (cvalid[c] && KB + v < K) ? a.theta[chain[c] * K + KB + v] : 0.0;
        ll[c] = 0.0;
    }
    // negative binomial: the chain's lam and phi = exp(lam), two registers per chain tile
    [[maybe_unused]] double lam[CT], phi[CT];
    [[maybe_unused]] bool regular[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        lam[c] = 0.0; phi[c] = 0.0; regular[c] = true;
        if constexpr (FAMILY == BINF_GLM_NEGBIN_LOG) {
            const double l = cvalid[c] ? a.lam[chain[c]] : 0.0;
            regular[c] = negbin_regular(l);
            lam[c] = negbin_lam(l);
            phi[c] = exp(lam[c]);
        }
    }

    const int ntiles = (N + 15) / 16;
    const int t0 = (int)blockIdx.x * GLM_PIECE_TILES;
    int t1 = t0 + GLM_PIECE_TILES;
    if (t1 > ntiles) t1 = ntiles;

    // staging: thread (srow, scol) moves A[16*pass + srow][16 t + scol]; threads 0 .. 47
    // also move y, m and the offset of column scol.  Unconditional loads at clamped
    // indices, invalid entries zeroed on the way into LDS.
    const int srow = tid >> 4, scol = tid & 15;
    const double *dsrc = srow == 0 ? a.ys : (srow == 1 ? a.trials : a.offset);
    const bool dhave = dsrc != nullptr;
    if (!dhave || srow >= 3) dsrc = a.ys;          // a load that is always legal, then unused
    const double dmiss = srow == 1 ? 1.0 : 0.0;
    double pre[PASSES];
    double pred = 0.0;
    auto fetch = [&](int t) {
        const int n = t * 16 + scol;
        const int nc = n < N ? n : N - 1;
#pragma unroll
        for (int ps = 0; ps < PASSES; ++ps) {
            const int k = 16 * ps + srow;
            pre[ps] = a.A[(int64_t)(k < K ? k : K - 1) * N + nc];
        }
        const double dv = dsrc[nc];
        pred = dhave ? dv : dmiss;
    };
    auto stash = [&](int buf, int t) {
        const bool nv = t * 16 + scol < N;
#pragma unroll
        for (int ps = 0; ps < PASSES; ++ps) {
            const int k = 16 * ps + srow;
            if (k < ROWS) sA[buf][k][scol] = (k < K && nv) ? pre[ps] : 0.0;
        }
        if (srow < 3) sD[buf][srow][scol] = nv ? pred : dmiss;
    };

    if (t0 < t1) {
        fetch(t0);
        stash(0, t0);
    }
    __syncthreads();
    for (int t = t0; t < t1; ++t) {
        const int buf = (t - t0) & 1;
        fetch(t + 1 < t1 ? t + 1 : t);             // in flight during the MFMAs
        __builtin_amdgcn_sched_barrier(0);
        // M^T[n][c] = sum_k A[k][n] theta[c][k]
        glm_v4d acc[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[c] = (glm_v4d){0.0, 0.0, 0.0, 0.0};
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
        // the term of glm_term.hpp from the accumulator registers; a padding column
        // (n >= N) is left out by a select
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int nl = lk + 4 * r;
            const double yv = sD[buf][0][nl], mv = sD[buf][1][nl], ov = sD[buf][2][nl];
            const bool nv = t * 16 + nl < N;
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                double l = 0.0, g = 0.0;
                glm_term_chain<FAMILY, true, false>(glm_eta<FAMILY>(acc[c][r], ov), yv, mv,
                                                    lam[c], phi[c], l, g);
                const double s = ll[c] + l;
                ll[c] = nv ? s : ll[c];
            }
        }
        if (t + 1 < t1) stash(buf ^ 1, t + 1);
        __syncthreads();
    }

#pragma unroll
    for (int c = 0; c < CT; ++c) {
        // the four lk partials of a chain: (0 + 1) + (2 + 3)
        ll[c] = ll[c] + shfl_xor_f64(ll[c], 16);
        ll[c] = ll[c] + shfl_xor_f64(ll[c], 32);
        if (cvalid[c] && lk == 0) {
            if (!a.finish) {
                a.out[(int64_t)blockIdx.x * a.C + chain[c]] = ll[c];
            } else if constexpr (FAMILY == BINF_GLM_NEGBIN_LOG) {
                // the chain's own constant last; a lam outside the regular range: -inf
                const double s = ll[c] + a.lnc[chain[c]];
                a.out[chain[c]] = regular[c] ? s : -INFINITY;
            } else {
                a.out[chain[c]] = ll[c] + a.log_norm;
            }
        }
    }
}

// out[c] = (part[0][c] + part[1][c] + ...) + log_norm, pieces in piece order
__global__ void __launch_bounds__(256)
glm_finish_kernel(const double *part, int32_t pieces, double log_norm, double *out, int64_t C)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double s = part[c];
    for (int k = 1; k < pieces; ++k) s = s + part[(int64_t)k * C + c];
    out[c] = s + log_norm;
}

// the same with the negative binomial's per-chain constant: out[c] = (part[0][c] + ...) +
// log_norm_chain[c], -inf for a lam outside the regular range
__global__ void __launch_bounds__(256)
glm_finish_chain_kernel(const double *part, int32_t pieces, const double *lam, const double *lnc,
                        double *out, int64_t C)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double s = part[c];
    for (int k = 1; k < pieces; ++k) s = s + part[(int64_t)k * C + c];
    s = s + lnc[c];
    out[c] = negbin_regular(lam[c]) ? s : -INFINITY;
}

// ---------------------------------------------------------------------------
// fused gradient: poly_grad_mfma_kernel's two chained products, rr = nv ? g : 0
// ---------------------------------------------------------------------------
struct GlmGradArgs {
    const double *theta;     // [C x K]
    const double *A;         // [K x N]
    const double *ys;        // [N]
    const double *trials;    // [N] or null
    const double *offset;    // [N] or null
    const double *lam;       // negative binomial: log dispersion [C]; else unused
    double *part;            // [NS x C x K] partial sums (or the output if NS == 1)
    int64_t C;
    int32_t K;
    int32_t N;
    int32_t tiles_per_split; // data tiles (of 16) per blockIdx.y
};

template <int FAMILY, int KS, int RT, int KV, int CT>
__global__ void __launch_bounds__(256) glm_grad_kernel(const GlmGradArgs a)
{
    constexpr int KB = 4 * KS;                       // first VALU coefficient
    constexpr int ROWS0 = (4 * KS > 16 * RT) ? 4 * KS : 16 * RT;
    constexpr int ROWS = ROWS0 + KV;
    constexpr int PASSES = (ROWS + 15) / 16;
    static_assert(KV == 0 || 4 * KS == 16 * RT, "VALU tail needs 4*KS == 16*RT");
    __shared__ double sA[2][ROWS][GLM_LDA];
    __shared__ double sD[2][3][16];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int lc = lane & 15;
    const int lk = lane >> 4;
    const int K = a.K, N = a.N;

    int64_t chain[CT];
    bool cvalid[CT];
    double th[CT][KS];
    double thv[CT][KV > 0 ? KV : 1], gv[CT][KV > 0 ? KV : 1];
    glm_v4d G[CT][RT];
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        chain[c] = ((int64_t)blockIdx.x * 4 + wave) * (16 * CT) + 16 * c + lc;
        cvalid[c] = chain[c] < a.C;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int k = 4 * s + lk;
            th[c][s] = (cvalid[c] && k < K) ? a.theta[chain[c] * K + k] : 0.0;
        }
#pragma unroll
        for (int v = 0; v < KV; ++v) {
            thv[c][v] = (cvalid[c] && KB + v < K) ? a.theta[chain[c] * K + KB + v] : 0.0;
            gv[c][v] = 0.0;
        }
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) G[c][rt] = (glm_v4d){0.0, 0.0, 0.0, 0.0};
    }
    // negative binomial: the chain's lam and phi = exp(lam), as in the log-prob kernel
    [[maybe_unused]] double lam[CT], phi[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        lam[c] = 0.0; phi[c] = 0.0;
        if constexpr (FAMILY == BINF_GLM_NEGBIN_LOG) {
            lam[c] = negbin_lam(cvalid[c] ? a.lam[chain[c]] : 0.0);
            phi[c] = exp(lam[c]);
        }
    }

    const int t0 = blockIdx.y * a.tiles_per_split;
    int t1 = t0 + a.tiles_per_split;
    const int ntiles = (N + 15) / 16;
    if (t1 > ntiles) t1 = ntiles;

    // staging: unconditional loads at clamped indices, invalid entries zeroed on the way
    // into LDS (poly_grad_mfma_kernel)
    const int srow = tid >> 4, scol = tid & 15;
    const double *dsrc = srow == 0 ? a.ys : (srow == 1 ? a.trials : a.offset);
    const bool dhave = dsrc != nullptr;
    if (!dhave || srow >= 3) dsrc = a.ys;          // a load that is always legal, then unused
    const double dmiss = srow == 1 ? 1.0 : 0.0;
    double pre[PASSES];
    double pred = 0.0;
    auto fetch = [&](int t) {
        const int n = t * 16 + scol;
        const int nc = n < N ? n : N - 1;
#pragma unroll
        for (int ps = 0; ps < PASSES; ++ps) {
            const int k = 16 * ps + srow;
            pre[ps] = a.A[(int64_t)(k < K ? k : K - 1) * N + nc];
        }
        const double dv = dsrc[nc];
        pred = dhave ? dv : dmiss;
    };
    auto stash = [&](int buf, int t) {
        const bool nv = t * 16 + scol < N;
#pragma unroll
        for (int ps = 0; ps < PASSES; ++ps) {
            const int k = 16 * ps + srow;
            if (k < ROWS) sA[buf][k][scol] = (k < K && nv) ? pre[ps] : 0.0;
        }
        if (srow < 3) sD[buf][srow][scol] = nv ? pred : dmiss;
    };

    if (t0 < t1) {
        fetch(t0);
        stash(0, t0);
    }
    __syncthreads();
    for (int t = t0; t < t1; ++t) {
        const int buf = (t - t0) & 1;
        fetch(t + 1 < t1 ? t + 1 : t);         // in flight during the MFMAs
        __builtin_amdgcn_sched_barrier(0);
        // forward: M^T[n][c] = sum_k A[k][n] theta[c][k]
        glm_v4d acc[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[c] = (glm_v4d){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const double av = sA[buf][4 * s + lk][lc];
#pragma unroll
            for (int c = 0; c < CT; ++c)
                acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, th[c][s], acc[c], 0, 0, 0);
        }
#pragma unroll
        for (int v = 0; v < KV; ++v)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double av = sA[buf][KB + v][lk + 4 * r];
#pragma unroll
                for (int c = 0; c < CT; ++c)
                    acc[c][r] = __builtin_fma(thv[c][v], av, acc[c][r]);
            }
        // error-model gradient in place: r[n][c] = g of glm_term.hpp, 0 beyond N
        double rr[CT][4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int nl = lk + 4 * r;
            const double yv = sD[buf][0][nl], mv = sD[buf][1][nl], ov = sD[buf][2][nl];
            const bool nv = t * 16 + nl < N;
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                double l = 0.0, g = 0.0;
                glm_term_chain<FAMILY, false, true>(glm_eta<FAMILY>(acc[c][r], ov), yv, mv,
                                                    lam[c], phi[c], l, g);
                rr[c][r] = nv ? g : 0.0;
            }
        }
        // backward: G^T[i][c] += sum_n A[i][n] r[n][c]
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const double av = sA[buf][16 * rt + lc][4 * s + lk];
#pragma unroll
                for (int c = 0; c < CT; ++c)
                    G[c][rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, rr[c][s], G[c][rt], 0, 0, 0);
            }
#pragma unroll
        for (int v = 0; v < KV; ++v)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double av = sA[buf][KB + v][lk + 4 * r];
#pragma unroll
                for (int c = 0; c < CT; ++c)
                    gv[c][v] = __builtin_fma(av, rr[c][r], gv[c][v]);
            }
        if (t + 1 < t1) stash(buf ^ 1, t + 1);
        __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < CT; ++c) {
#pragma unroll
        for (int v = 0; v < KV; ++v) {
            gv[c][v] = gv[c][v] + shfl_xor_f64(gv[c][v], 16);
            gv[c][v] = gv[c][v] + shfl_xor_f64(gv[c][v], 32);
        }
        if (cvalid[c]) {
            double *dst = a.part + ((int64_t)blockIdx.y * a.C + chain[c]) * K;
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = 16 * rt + lk + 4 * r;
                    if (i < K) dst[i] = G[c][rt][r];
                }
            if (lk == 0) {
#pragma unroll
                for (int v = 0; v < KV; ++v)
                    if (KB + v < K) dst[KB + v] = gv[c][v];
            }
        }
    }
}

// out[j] = part[0][j] + part[1][j] + ... in split order
__global__ void __launch_bounds__(256)
glm_split_reduce_kernel(const double *part, double *out, int64_t n, int32_t ns)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    double s = part[j];
    for (int k = 1; k < ns; ++k) s = s + part[(int64_t)k * n + j];
    out[j] = s;
}

// The same sum, Posterior.gradient's sum with the prior's force k * (q - x0) when there
// is one (two terms: either order gives the same bits), the kick it feeds and the drift
// that follows (hmc.py:116-123).  leap: 1 half kick + drift, 2 kick + drift, 3 half kick.
template <bool FMA, bool PRIOR>
__global__ void __launch_bounds__(256)
glm_reduce_kick_drift_kernel(const double *part, double *q, double *p, const double *dt_chain,
                             double timestep, double prior_k, double prior_x0, int64_t n,
                             int32_t K, int32_t ns, int32_t leap)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    double g = part[j];
    for (int k = 1; k < ns; ++k) g = g + part[(int64_t)k * n + j];
    const double qv = q[j];
    if constexpr (PRIOR) g = g + prior_k * (qv - prior_x0);
    const double d = dt_chain ? dt_chain[j / K] : timestep;
    const double step = (leap == 2) ? d : 0.5 * d;          // "0.5 * timestep" first
    const double pv = p[j];
    const double pn = FMA ? __builtin_fma(-step, g, pv) : pv - step * g;
    p[j] = pn;
    if (leap != 3) q[j] = FMA ? __builtin_fma(pn, d, qv) : qv + pn * d;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
template <int FAMILY, int KS, int KV>
static hipError_t glm_logp_launch(const GlmLogpArgs &a, int ct, dim3 grid, hipStream_t st)
{
    if (ct == 2) glm_logp_kernel<FAMILY, KS, KV, 2><<<grid, 256, 0, st>>>(a);
    else         glm_logp_kernel<FAMILY, KS, KV, 1><<<grid, 256, 0, st>>>(a);
    return hipGetLastError();
}

// the split of K into MFMA k-steps and VALU coefficients is chi2_dispatch's (linear.hip)
template <int FAMILY>
static hipError_t glm_logp_dispatch(const GlmLogpArgs &a, int64_t K, int ct, dim3 grid, hipStream_t st)
{
    if (K <= 4)       return glm_logp_launch<FAMILY, 1, 0>(a, ct, grid, st);
    else if (K <= 8)  return glm_logp_launch<FAMILY, 2, 0>(a, ct, grid, st);
    else if (K <= 16) return glm_logp_launch<FAMILY, 4, 0>(a, ct, grid, st);
    else if (K == 17) return glm_logp_launch<FAMILY, 4, 1>(a, ct, grid, st);
    else if (K == 18) return glm_logp_launch<FAMILY, 4, 2>(a, ct, grid, st);
    else if (K <= 32) return glm_logp_launch<FAMILY, 8, 0>(a, ct, grid, st);
    else if (K == 33) return glm_logp_launch<FAMILY, 8, 1>(a, ct, grid, st);
    else if (K == 34) return glm_logp_launch<FAMILY, 8, 2>(a, ct, grid, st);
    else if (K <= 36) return glm_logp_launch<FAMILY, 9, 0>(a, ct, grid, st);
    else if (K <= 48) return glm_logp_launch<FAMILY, 12, 0>(a, ct, grid, st);
    else if (K == 49) return glm_logp_launch<FAMILY, 12, 1>(a, ct, grid, st);
    else if (K == 50) return glm_logp_launch<FAMILY, 12, 2>(a, ct, grid, st);
    return glm_logp_launch<FAMILY, 16, 0>(a, ct, grid, st);
}

template <int FAMILY, int KS, int RT, int KV>
static hipError_t glm_grad_launch(const GlmGradArgs &a, int ct, dim3 grid, hipStream_t st)
{
    if (ct == 2) glm_grad_kernel<FAMILY, KS, RT, KV, 2><<<grid, 256, 0, st>>>(a);
    else         glm_grad_kernel<FAMILY, KS, RT, KV, 1><<<grid, 256, 0, st>>>(a);
    return hipGetLastError();
}

// grad_dispatch's K table (poly.hip)
template <int FAMILY>
static hipError_t glm_grad_dispatch_k(const GlmGradArgs &a, int64_t K, int ct, dim3 grid, hipStream_t st)
{
    if (K <= 4)       return glm_grad_launch<FAMILY, 1, 1, 0>(a, ct, grid, st);
    else if (K <= 8)  return glm_grad_launch<FAMILY, 2, 1, 0>(a, ct, grid, st);
    else if (K <= 16) return glm_grad_launch<FAMILY, 4, 1, 0>(a, ct, grid, st);
    else if (K == 17) return glm_grad_launch<FAMILY, 4, 1, 1>(a, ct, grid, st);
    else if (K == 18) return glm_grad_launch<FAMILY, 4, 1, 2>(a, ct, grid, st);
    else if (K <= 32) return glm_grad_launch<FAMILY, 8, 2, 0>(a, ct, grid, st);
    else if (K == 33) return glm_grad_launch<FAMILY, 8, 2, 1>(a, ct, grid, st);
    else if (K == 34) return glm_grad_launch<FAMILY, 8, 2, 2>(a, ct, grid, st);
    else if (K <= 36) return glm_grad_launch<FAMILY, 9, 3, 0>(a, ct, grid, st);
    else if (K <= 48) return glm_grad_launch<FAMILY, 12, 3, 0>(a, ct, grid, st);
    else if (K == 49) return glm_grad_launch<FAMILY, 12, 3, 1>(a, ct, grid, st);
    else if (K == 50) return glm_grad_launch<FAMILY, 12, 3, 2>(a, ct, grid, st);
    return glm_grad_launch<FAMILY, 16, 4, 0>(a, ct, grid, st);
}

static hipError_t glm_grad_dispatch(int32_t family, const GlmGradArgs &a, int64_t K, int ct,
                                    dim3 grid, hipStream_t st)
{
    if (family == BINF_GLM_NEGBIN_LOG)
        return glm_grad_dispatch_k<BINF_GLM_NEGBIN_LOG>(a, K, ct, grid, st);
    return family == BINF_GLM_BINOMIAL_LOGIT
        ? glm_grad_dispatch_k<BINF_GLM_BINOMIAL_LOGIT>(a, K, ct, grid, st)
        : glm_grad_dispatch_k<BINF_GLM_POISSON_LOG>(a, K, ct, grid, st);
}

// chain tiles per wave and data splits: those of the Gaussian gradient (poly.hip:
// grad_ct, grad_splits), restated -- the two must stay in step
static int glm_ct(int64_t C) { return C >= 4096 ? 2 : 1; }

static int glm_splits(int64_t C, int64_t N)
{
    const int64_t wgx = (C + 64 * glm_ct(C) - 1) / (64 * glm_ct(C));
    const int64_t ntiles = (N + 15) / 16;
    constexpr int64_t target = 512;
    int64_t ns = (target + wgx - 1) / wgx;
    if (ns > 64) ns = 64;
    if (ns > ntiles) ns = ntiles;
    if (ns < 1) ns = 1;
    return (int)ns;
}

static int64_t glm_pieces(int64_t N)
{
    const int64_t ntiles = (N + 15) / 16;
    const int64_t np = (ntiles + GLM_PIECE_TILES - 1) / GLM_PIECE_TILES;
    return np < 1 ? 1 : np;
}

// check_linear's limits (linear.hip), and the family (the negative binomial has entry
// points of its own, which take its log dispersion: the family argument never names it)
static int32_t check_glm(const char *what, int32_t family, int64_t C, int64_t K, int64_t N,
                         bool negbin = false)
{
    if (C < 0 || K < 1 || N < 0)
        return fail(BINF_E_ARG, "%s: need C>=0, K>=1, N>=0", what);
    if (negbin ? family != BINF_GLM_NEGBIN_LOG
               : (family != BINF_GLM_BINOMIAL_LOGIT && family != BINF_GLM_POISSON_LOG))
        return fail(BINF_E_ARG, "%s: unknown family %d", what, family);
    if (K > 64)
        return fail(BINF_E_UNSUPPORTED, "%s: K=%lld coefficients > 64 not covered by the native linear kernels", what, (long long)K);
    if (C > 65535 * 64LL || N > 0x7fffffffLL - 16)
        return fail(BINF_E_UNSUPPORTED, "%s: too large", what);
    return 0;
}

static void glm_grad_args(GlmGradArgs &a, const double *theta, const double *design,
                          const double *ys, const double *trials, const double *offset,
                          double *part, int64_t C, int64_t K, int64_t N, int ns,
                          const double *lam = nullptr)
{
    const int ntiles = (int)((N + 15) / 16);
    a.theta = theta; a.A = design; a.ys = ys; a.trials = trials; a.offset = offset;
    a.lam = lam;
    a.part = part; a.C = C; a.K = (int32_t)K; a.N = (int32_t)N;
    a.tiles_per_split = (ntiles + ns - 1) / ns;
    if (a.tiles_per_split < 1) a.tiles_per_split = 1;
}

}  // namespace binf

using namespace binf;

extern "C" int32_t binf_glm_pointwise_f64(const double *mock, const double *ys,
                                          const double *trials, const double *offset,
                                          const double *lconst, int32_t family, double *out_ll,
                                          double *out_grad, int64_t S, int64_t N, void *stream)
{
    const char *what = "glm_pointwise";
    if (S < 0 || N < 0) return fail(BINF_E_ARG, "%s: need S>=0, N>=0", what);
    if (family != BINF_GLM_BINOMIAL_LOGIT && family != BINF_GLM_POISSON_LOG)
        return fail(BINF_E_ARG, "%s: unknown family %d", what, family);
    if (!out_ll && !out_grad) return fail(BINF_E_ARG, "%s: no output", what);
    if (N >= 0x7fffffffLL || (S > 0 && N > (1LL << 53) / S))
        return fail(BINF_E_UNSUPPORTED, "%s: too large", what);
    if (S == 0 || N == 0) return 0;
    if (!mock || !ys) return fail(BINF_E_ARG, "%s: null buffer", what);
    const int64_t total = S * N;
    double *outs[2] = {out_ll, out_grad};
    for (double *o : outs) {
        if (!o) continue;
        if (overlap_f64(o, total, mock, total) || overlap_f64(o, total, ys, N) ||
            overlap_f64(o, total, trials, N) || overlap_f64(o, total, offset, N) ||
            overlap_f64(o, total, lconst, N))
            return fail(BINF_E_ALIAS, "%s: an output overlaps an input", what);
    }
    if (overlap_f64(out_ll, total, out_grad, total))
        return fail(BINF_E_ALIAS, "%s: the outputs overlap", what);
    int64_t blocks = (total + 255) / 256;
    if (blocks > 65535 * 16) blocks = 65535 * 16;
    hipStream_t st = (hipStream_t)stream;
    if (family == BINF_GLM_BINOMIAL_LOGIT)
        glm_pointwise_kernel<BINF_GLM_BINOMIAL_LOGIT><<<dim3((unsigned)blocks), 256, 0, st>>>(
            mock, ys, trials, offset, lconst, out_ll, out_grad, total, N);
    else
        glm_pointwise_kernel<BINF_GLM_POISSON_LOG><<<dim3((unsigned)blocks), 256, 0, st>>>(
            mock, ys, trials, offset, lconst, out_ll, out_grad, total, N);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "glm_pointwise launch");
    return 0;
}

extern "C" int64_t binf_linear_glm_logp_workspace_bytes(int64_t C, int64_t K, int64_t N)
{
    if (C <= 0 || K <= 0 || N <= 0) return 0;
    const int64_t np = glm_pieces(N);
    return np > 1 ? np * C * (int64_t)sizeof(double) : 0;
}

// the fused log-prob of every family; lam, lnc [C]: the negative binomial's log dispersion
// and per-chain constant (else null and unread)
static int32_t glm_logp_run(const char *what, const double *coeffs, const double *design,
                            const double *ys, const double *trials, const double *offset,
                            int32_t family, const double *lam, const double *lnc,
                            double log_norm, double *out, void *workspace,
                            int64_t workspace_bytes, int64_t C, int64_t K, int64_t N,
                            void *stream, bool nb)
{
    int32_t rc = check_glm(what, family, C, K, N, nb);
    if (rc) return rc;
    if (C == 0) return 0;
    if (N < 1) return fail(BINF_E_UNSUPPORTED, "%s: no data points", what);
    if (!coeffs || !out || !design || !ys || (nb && (!lam || !lnc)))
        return fail(BINF_E_ARG, "%s: null buffer", what);
    if (overlap_f64(out, C, coeffs, C * K) || overlap_f64(out, C, design, K * N) ||
        overlap_f64(out, C, ys, N) || overlap_f64(out, C, trials, N) ||
        overlap_f64(out, C, offset, N) || overlap_f64(out, C, lam, C) ||
        overlap_f64(out, C, lnc, C))
        return fail(BINF_E_ALIAS, "%s: out overlaps an input", what);
    // The pieces follow from N alone (never from C), so a missing or short workspace is
    // an error, never a silent change of summation order.
    const int64_t np = glm_pieces(N);
    const int64_t need = np > 1 ? np * C * (int64_t)sizeof(double) : 0;
    if (need > 0) {
        if (!workspace || workspace_bytes < need)
            return fail(BINF_E_ARG, "%s: needs %lld bytes of workspace "
                        "(binf_linear_glm_logp_workspace_bytes), got %lld", what,
                        (long long)need, (long long)workspace_bytes);
        if (overlap_f64(workspace, need / 8, out, C) || overlap_f64(workspace, need / 8, coeffs, C * K) ||
            overlap_f64(workspace, need / 8, design, K * N) || overlap_f64(workspace, need / 8, ys, N) ||
            overlap_f64(workspace, need / 8, trials, N) || overlap_f64(workspace, need / 8, offset, N) ||
            overlap_f64(workspace, need / 8, lam, C) || overlap_f64(workspace, need / 8, lnc, C))
            return fail(BINF_E_ALIAS, "%s: the workspace overlaps a buffer", what);
    }
    GlmLogpArgs a;
    a.theta = coeffs; a.A = design; a.ys = ys; a.trials = trials; a.offset = offset;
    a.lam = lam; a.lnc = lnc;
    a.log_norm = log_norm; a.C = C; a.K = (int32_t)K; a.N = (int32_t)N;
    a.finish = np > 1 ? 0 : 1;
    a.out = np > 1 ? (double *)workspace : out;
    const int ct = glm_ct(C);
    dim3 grid((unsigned)np, (unsigned)((C + 64 * ct - 1) / (64 * ct)));
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = nb ? glm_logp_dispatch<BINF_GLM_NEGBIN_LOG>(a, K, ct, grid, st)
        : family == BINF_GLM_BINOMIAL_LOGIT
        ? glm_logp_dispatch<BINF_GLM_BINOMIAL_LOGIT>(a, K, ct, grid, st)
        : glm_logp_dispatch<BINF_GLM_POISSON_LOG>(a, K, ct, grid, st);
    if (e != hipSuccess) return hip_fail(e, "linear_glm_logp launch");
    if (np > 1) {
        const dim3 fgrid((unsigned)((C + 255) / 256));
        if (nb) glm_finish_chain_kernel<<<fgrid, 256, 0, st>>>(
                    (const double *)workspace, (int32_t)np, lam, lnc, out, C);
        else    glm_finish_kernel<<<fgrid, 256, 0, st>>>(
                    (const double *)workspace, (int32_t)np, log_norm, out, C);
        e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, "linear_glm_logp finish launch");
    }
    return 0;
}

extern "C" int32_t binf_linear_glm_logp_f64(const double *coeffs, const double *design,
                                            const double *ys, const double *trials,
                                            const double *offset, int32_t family,
                                            double log_norm, double *out, void *workspace,
                                            int64_t workspace_bytes, int64_t C, int64_t K,
                                            int64_t N, void *stream)
{
    return glm_logp_run("linear_glm_logp", coeffs, design, ys, trials, offset, family, nullptr,
                        nullptr, log_norm, out, workspace, workspace_bytes, C, K, N, stream,
                        false);
}

extern "C" int32_t binf_linear_negbin_logp_f64(const double *coeffs, const double *design,
                                               const double *ys, const double *offset,
                                               const double *log_dispersion,
                                               const double *log_norm_chain, double *out,
                                               void *workspace, int64_t workspace_bytes,
                                               int64_t C, int64_t K, int64_t N, void *stream)
{
    return glm_logp_run("linear_negbin_logp", coeffs, design, ys, nullptr, offset,
                        BINF_GLM_NEGBIN_LOG, log_dispersion, log_norm_chain, 0.0, out, workspace,
                        workspace_bytes, C, K, N, stream, true);
}

extern "C" int64_t binf_linear_glm_grad_workspace_bytes(int64_t C, int64_t K, int64_t N)
{
    if (C <= 0 || K <= 0 || N <= 0) return 0;
    const int ns = glm_splits(C, N);
    return ns > 1 ? (int64_t)ns * C * K * (int64_t)sizeof(double) : 0;
}

static int32_t glm_grad_run(const char *what, const double *coeffs, const double *design,
                            const double *ys, const double *trials, const double *offset,
                            int32_t family, const double *lam, double *out, void *workspace,
                            int64_t workspace_bytes, int64_t C, int64_t K, int64_t N,
                            void *stream, bool nb)
{
    int32_t rc = check_glm(what, family, C, K, N, nb);
    if (rc) return rc;
    if (C == 0) return 0;
    if (N < 1) return fail(BINF_E_UNSUPPORTED, "%s: no data points", what);
    if (!coeffs || !out || !design || !ys || (nb && !lam))
        return fail(BINF_E_ARG, "%s: null buffer", what);
    if (overlap_f64(out, C * K, coeffs, C * K) || overlap_f64(out, C * K, design, K * N) ||
        overlap_f64(out, C * K, ys, N) || overlap_f64(out, C * K, trials, N) ||
        overlap_f64(out, C * K, offset, N) || overlap_f64(out, C * K, lam, C))
        return fail(BINF_E_ALIAS, "%s: out overlaps an input", what);
    // ns follows from (C, N) alone (the Gaussian gradient's contract): a missing or short
    // workspace is an error, never a silent change of summation order
    const int ns = glm_splits(C, N);
    const int64_t need = ns > 1 ? (int64_t)ns * C * K * (int64_t)sizeof(double) : 0;
    if (need > 0) {
        if (!workspace || workspace_bytes < need)
            return fail(BINF_E_ARG, "%s: needs %lld bytes of workspace "
                        "(binf_linear_glm_grad_workspace_bytes), got %lld", what,
                        (long long)need, (long long)workspace_bytes);
        if (overlap_f64(workspace, need / 8, out, C * K) || overlap_f64(workspace, need / 8, coeffs, C * K) ||
            overlap_f64(workspace, need / 8, design, K * N) || overlap_f64(workspace, need / 8, ys, N) ||
            overlap_f64(workspace, need / 8, trials, N) || overlap_f64(workspace, need / 8, offset, N) ||
            overlap_f64(workspace, need / 8, lam, C))
            return fail(BINF_E_ALIAS, "%s: the workspace overlaps a buffer", what);
    }
    GlmGradArgs a;
    glm_grad_args(a, coeffs, design, ys, trials, offset, ns > 1 ? (double *)workspace : out,
                  C, K, N, ns, lam);
    const int ct = glm_ct(C);
    dim3 grid((unsigned)((C + 64 * ct - 1) / (64 * ct)), (unsigned)ns);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = glm_grad_dispatch(family, a, K, ct, grid, st);
    if (e != hipSuccess) return hip_fail(e, "linear_glm_grad launch");
    if (ns > 1) {
        const int64_t n = C * K;
        glm_split_reduce_kernel<<<dim3((unsigned)((n + 255) / 256)), 256, 0, st>>>(
            (const double *)workspace, out, n, ns);
        e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, "linear_glm_grad reduce launch");
    }
    return 0;
}

extern "C" int32_t binf_linear_glm_grad_f64(const double *coeffs, const double *design,
                                            const double *ys, const double *trials,
                                            const double *offset, int32_t family, double *out,
                                            void *workspace, int64_t workspace_bytes,
                                            int64_t C, int64_t K, int64_t N, void *stream)
{
    return glm_grad_run("linear_glm_grad", coeffs, design, ys, trials, offset, family, nullptr,
                        out, workspace, workspace_bytes, C, K, N, stream, false);
}

extern "C" int32_t binf_linear_negbin_grad_f64(const double *coeffs, const double *design,
                                               const double *ys, const double *offset,
                                               const double *log_dispersion, double *out,
                                               void *workspace, int64_t workspace_bytes,
                                               int64_t C, int64_t K, int64_t N, void *stream)
{
    return glm_grad_run("linear_negbin_grad", coeffs, design, ys, nullptr, offset,
                        BINF_GLM_NEGBIN_LOG, log_dispersion, out, workspace, workspace_bytes,
                        C, K, N, stream, true);
}

extern "C" int64_t binf_linear_glm_leapfrog_workspace_bytes(int64_t C, int64_t K, int64_t N)
{
    if (C <= 0 || K <= 0 || N <= 0) return 0;
    return (int64_t)glm_splits(C, N) * C * K * (int64_t)sizeof(double);
}

static int32_t glm_leapfrog_run(const char *what, double *q, double *p, const double *design,
                                const double *ys, const double *trials, const double *offset,
                                int32_t family, const double *lam, int32_t has_prior,
                                double prior_k, double prior_x0, void *workspace,
                                int64_t workspace_bytes, int64_t C, int64_t K, int64_t N,
                                double timestep, const double *dt_chain, int32_t nsteps,
                                int32_t mode, void *stream, bool nb)
{
    int32_t rc = check_glm(what, family, C, K, N, nb);
    if (rc) return rc;
    if (nsteps < 1) return fail(BINF_E_ARG, "%s: nsteps >= 1 required", what);
    if (mode != BINF_MODE_EXACT && mode != BINF_MODE_FMA)
        return fail(BINF_E_ARG, "%s: unknown mode %d", what, mode);
    if (has_prior != 0 && has_prior != 1)
        return fail(BINF_E_ARG, "%s: has_prior must be 0 or 1", what);
    if (C == 0) return 0;
    if (N < 1) return fail(BINF_E_UNSUPPORTED, "%s: no data points", what);
    if (!q || !p || !design || !ys || (nb && !lam))
        return fail(BINF_E_ARG, "%s: null buffer", what);
    const int64_t need = binf_linear_glm_leapfrog_workspace_bytes(C, K, N);
    if (!workspace || workspace_bytes < need)
        return fail(BINF_E_ARG, "%s: needs %lld bytes of workspace "
                    "(binf_linear_glm_leapfrog_workspace_bytes), got %lld", what,
                    (long long)need, (long long)workspace_bytes);
    const int64_t n = C * K;
    if (overlap_f64(q, n, p, n) || overlap_f64(q, n, design, K * N) || overlap_f64(p, n, design, K * N) ||
        overlap_f64(q, n, ys, N) || overlap_f64(p, n, ys, N) || overlap_f64(q, n, trials, N) ||
        overlap_f64(p, n, trials, N) || overlap_f64(q, n, offset, N) || overlap_f64(p, n, offset, N) ||
        overlap_f64(q, n, dt_chain, C) || overlap_f64(p, n, dt_chain, C) ||
        overlap_f64(q, n, lam, C) || overlap_f64(p, n, lam, C))
        return fail(BINF_E_ALIAS, "%s: q or p overlaps another buffer", what);
    if (overlap_f64(workspace, need / 8, q, n) || overlap_f64(workspace, need / 8, p, n) ||
        overlap_f64(workspace, need / 8, design, K * N) || overlap_f64(workspace, need / 8, ys, N) ||
        overlap_f64(workspace, need / 8, trials, N) || overlap_f64(workspace, need / 8, offset, N) ||
        overlap_f64(workspace, need / 8, dt_chain, C) || overlap_f64(workspace, need / 8, lam, C))
        return fail(BINF_E_ALIAS, "%s: the workspace overlaps a buffer", what);
    const int ns = glm_splits(C, N);
    const int ct = glm_ct(C);
    GlmGradArgs a;
    glm_grad_args(a, q, design, ys, trials, offset, (double *)workspace, C, K, N, ns, lam);
    dim3 grid((unsigned)((C + 64 * ct - 1) / (64 * ct)), (unsigned)ns);
    hipStream_t st = (hipStream_t)stream;
    const dim3 rgrid((unsigned)((n + 255) / 256));
    const double *part = (const double *)workspace;
    const int32_t k32 = (int32_t)K;
    // hmc.py:116-123: half kick, (nsteps - 1) x [drift, kick], drift, half kick -- per
    // gradient one MFMA launch and one launch for partial sums + prior + kick + drift
    for (int l = 0; l <= nsteps; ++l) {
        const int leap = (l == 0) ? 1 : (l == nsteps ? 3 : 2);
        hipError_t e = glm_grad_dispatch(family, a, K, ct, grid, st);
        if (e != hipSuccess) return hip_fail(e, "linear_glm_leapfrog gradient launch");
        const bool fma = mode == BINF_MODE_FMA;
        if (has_prior) {
            if (fma) glm_reduce_kick_drift_kernel<true, true><<<rgrid, 256, 0, st>>>(
                         part, q, p, dt_chain, timestep, prior_k, prior_x0, n, k32, ns, leap);
            else     glm_reduce_kick_drift_kernel<false, true><<<rgrid, 256, 0, st>>>(
                         part, q, p, dt_chain, timestep, prior_k, prior_x0, n, k32, ns, leap);
        } else {
            if (fma) glm_reduce_kick_drift_kernel<true, false><<<rgrid, 256, 0, st>>>(
                         part, q, p, dt_chain, timestep, prior_k, prior_x0, n, k32, ns, leap);
            else     glm_reduce_kick_drift_kernel<false, false><<<rgrid, 256, 0, st>>>(
                         part, q, p, dt_chain, timestep, prior_k, prior_x0, n, k32, ns, leap);
        }
        e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, "linear_glm_leapfrog kick launch");
    }
    return 0;
}

extern "C" int32_t binf_linear_glm_leapfrog_f64(double *q, double *p, const double *design,
                                                const double *ys, const double *trials,
                                                const double *offset, int32_t family,
                                                int32_t has_prior, double prior_k,
                                                double prior_x0, void *workspace,
                                                int64_t workspace_bytes, int64_t C, int64_t K,
                                                int64_t N, double timestep,
                                                const double *dt_chain, int32_t nsteps,
                                                int32_t mode, void *stream)
{
    return glm_leapfrog_run("linear_glm_leapfrog", q, p, design, ys, trials, offset, family,
                            nullptr, has_prior, prior_k, prior_x0, workspace, workspace_bytes,
                            C, K, N, timestep, dt_chain, nsteps, mode, stream, false);
}

extern "C" int32_t binf_linear_negbin_leapfrog_f64(double *q, double *p, const double *design,
                                                   const double *ys, const double *offset,
                                                   const double *log_dispersion,
                                                   int32_t has_prior, double prior_k,
                                                   double prior_x0, void *workspace,
                                                   int64_t workspace_bytes, int64_t C,
                                                   int64_t K, int64_t N, double timestep,
                                                   const double *dt_chain, int32_t nsteps,
                                                   int32_t mode, void *stream)
{
    return glm_leapfrog_run("linear_negbin_leapfrog", q, p, design, ys, nullptr, offset,
                            BINF_GLM_NEGBIN_LOG, log_dispersion, has_prior, prior_k, prior_x0,
                            workspace, workspace_bytes, C, K, N, timestep, dt_chain, nsteps,
                            mode, stream, true);
}

extern "C" int32_t binf_negbin_pointwise_f64(const double *mock, const double *ys,
                                             const double *offset, const double *log_dispersion,
                                             const double *prefix, const int32_t *prefix_index,
                                             const double *lconst, double *out_ll,
                                             double *out_grad, int64_t S, int64_t N, int64_t J,
                                             void *stream)
{
    const char *what = "negbin_pointwise";
    if (S < 0 || N < 0 || J < 0) return fail(BINF_E_ARG, "%s: need S>=0, N>=0, J>=0", what);
    if (!out_ll && !out_grad) return fail(BINF_E_ARG, "%s: no output", what);
    if ((prefix != nullptr) != (prefix_index != nullptr) || (prefix && J < 1))
        return fail(BINF_E_ARG, "%s: prefix [S x J] and prefix_index [N] go together, J>=1", what);
    if (N >= 0x7fffffffLL || J > (1LL << 20) + 1 || (S > 0 && N > (1LL << 53) / S))
        return fail(BINF_E_UNSUPPORTED, "%s: too large", what);
    if (S == 0 || N == 0) return 0;
    if (!mock || !ys || !log_dispersion) return fail(BINF_E_ARG, "%s: null buffer", what);
    const int64_t total = S * N;
    double *outs[2] = {out_ll, out_grad};
    for (double *o : outs) {
        if (!o) continue;
        if (overlap_f64(o, total, mock, total) || overlap_f64(o, total, ys, N) ||
            overlap_f64(o, total, offset, N) || overlap_f64(o, total, lconst, N) ||
            overlap_f64(o, total, log_dispersion, S) || overlap_f64(o, total, prefix, S * J) ||
            overlap_f64(o, total, prefix_index, (N + 1) / 2))
            return fail(BINF_E_ALIAS, "%s: an output overlaps an input", what);
    }
    if (overlap_f64(out_ll, total, out_grad, total))
        return fail(BINF_E_ALIAS, "%s: the outputs overlap", what);
    int64_t blocks = (total + 255) / 256;
    if (blocks > 65535 * 16) blocks = 65535 * 16;
    negbin_pointwise_kernel<<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(
        mock, ys, offset, log_dispersion, prefix, prefix_index, lconst, out_ll, out_grad, total,
        N, J);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "negbin_pointwise launch");
    return 0;
}
