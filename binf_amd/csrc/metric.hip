// Diagonal HMC metric: the scaled entry points of the element-wise leapfrog kernel
// (leapfrog_ew.hpp: the kernel, its launcher and the argument check) and the two kernels of
// the windowed warm-up adaption -- streaming per-chain moments of the state, and the pooled
// per-group variance that becomes the new scale.  Build-defined: the reference integrates
// with the identity mass only (binf/samplers/hmc.py:92-125).  gfx950, wave64.
//
// A metric M = diag(1 / s^2) is carried through the WHITENED momentum r = p / sqrt(m): the
// momentum draw stays r ~ N(0, I) and the kinetic energy 0.5 sum r^2, so the energy, accept
// and adaption kernels are used as they are; kick and drift both take the per-element step
//     h = d * s[c % G][i],   d = dt_chain[c] or timestep (0.5 * d first for a half kick)
// (one rounding), then p - h * g and q + p * h, unfused (EXACT) or one fma each (FMA).  With
// s == 1.0, h == d exactly: the bits of the identity entry points (generic.hip), which are
// the same kernel with the scale compiled out.
//
// The arithmetic is stated in include/binf_hip.h and restated in numpy by
// tests/metric_ref.py; every multiply and add is rounded separately (common.hpp turns
// contraction off) and every sum over chains has the diagnostics' fixed order.
#include "leapfrog_ew.hpp"
#include "diag_core.hpp"

namespace binf {

template <int KIND>
static int32_t scaled_launch(double *q, double *p, const double *g, const double *scale, int64_t G,
                             double timestep, const double *dt_chain, int32_t half, int64_t C, int64_t D,
                             int32_t mode, void *stream, const char *what)
{
    int32_t rc = leapfrog_check_sizes(G, C, D, mode, what);
    if (rc != 0 || C == 0 || D == 0) return rc;
    rc = leapfrog_check<KIND>(q, p, g, scale, G, D, "scale", dt_chain, C, D, what);
    if (rc != 0) return rc;
    const LeapfrogEwArgs a{q, p, g, timestep, dt_chain, C * D, D};
    LeapfrogEwExtra<KIND, true> x;
    x.scale = scale; x.G = G;
    if constexpr (KIND == LF_KICK) x.half = half ? 1 : 0;
    return leapfrog_ew_launch<KIND, true>(a, x, mode, stream, what);
}

// ---------------------------------------------------------------------------
// streaming moments of the state: one DiagMoments per (chain, dimension) kept in three
// caller-owned [C x D] arrays, one element-wise pass per warm-up transition (32 bytes read,
// 24 written per element; the first pass of a window reads 8 and writes 24)
// ---------------------------------------------------------------------------
template <int VEC>
__global__ void __launch_bounds__(256)
metric_accumulate_kernel(const double *x, double *k0, double *s1, double *s2, int64_t n, int32_t first)
{
    const int64_t span = (int64_t)256 * VEC;
    for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * VEC; i < n; i += (int64_t)gridDim.x * span) {
        double xv[VEC], kv[VEC], av[VEC], bv[VEC];
        ew_load<VEC>(xv, x, i);
        if (!first) {
            ew_load<VEC>(kv, k0, i);
            ew_load<VEC>(av, s1, i);
            ew_load<VEC>(bv, s2, i);
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            DiagMoments m;
            if (first) {
                m.start(xv[v]);
            } else {
                m.k0 = kv[v];
                m.s1 = av[v];
                m.s2 = bv[v];
            }
            m.add(xv[v]);
            kv[v] = m.k0;
            av[v] = m.s1;
            bv[v] = m.s2;
        }
        if (first) ew_store<VEC>(k0, i, kv);
        ew_store<VEC>(s1, i, av);
        ew_store<VEC>(s2, i, bv);
    }
}

// ---------------------------------------------------------------------------
// pooled per-group variance -> scale
//
// A workgroup owns one group g and a tile of 64 dimensions: 4 waves, lanes along i, wave w
// sums chain block b0 + w of the group (a thread per (block, g, i): 64 consecutive chains of
// the group, sequential from 0.0); wave 0 then adds the four block sums in block order to its
// running totals (a thread per (g, i)).  The order is the diagnostics': a function of C / G
// only.  Two rounds of it: W and the sum of the means, then B about their mean.
// ---------------------------------------------------------------------------
struct MetricPoolArgs {
    const double *k0, *s1, *s2;
    double *scale;
    int64_t n, C, D, G, ntiles;
    int32_t regularise;
};

constexpr int MT_POOL_WAVES = 4;

__global__ void __launch_bounds__(64 * MT_POOL_WAVES) metric_pool_kernel(const MetricPoolArgs a)
{
    __shared__ double sm[2][MT_POOL_WAVES][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t g = (int64_t)blockIdx.x / a.ntiles;
    const int64_t i = ((int64_t)blockIdx.x - g * a.ntiles) * 64 + lane;
    const bool valid = i < a.D;
    const int64_t Cg = a.C / a.G;
    const int64_t nb = (Cg + DIAG_CHAIN_BLOCK - 1) / DIAG_CHAIN_BLOCK;
    const double dn = (double)a.n;
    // the moments of the q-th chain of block b of this group: chain g + (64 b + q) G
    auto at = [&](int64_t b, int q) {
        const int64_t e = (g + (b * DIAG_CHAIN_BLOCK + q) * a.G) * a.D + i;
        DiagMoments m;
        m.k0 = a.k0[e];
        m.s1 = a.s1[e];
        m.s2 = a.s2[e];
        return m;
    };
    double W = 0.0, SM = 0.0;
    for (int64_t b0 = 0; b0 < nb; b0 += MT_POOL_WAVES) {
        const int64_t b = b0 + w;
        double sw = 0.0, sg = 0.0;
        if (valid && b < nb) {
            const int64_t left = Cg - b * DIAG_CHAIN_BLOCK;
            const int cnt = left < DIAG_CHAIN_BLOCK ? (int)left : DIAG_CHAIN_BLOCK;
            for (int q = 0; q < cnt; ++q) {
                const DiagMoments m = at(b, q);
                sw = sw + m.m2(dn);
                sg = sg + m.mean(dn);
            }
        }
        sm[0][w][lane] = sw;
        sm[1][w][lane] = sg;
        __syncthreads();
        if (w == 0)
            for (int s = 0; s < MT_POOL_WAVES && b0 + s < nb; ++s) {
                W = W + sm[0][s][lane];
                SM = SM + sm[1][s][lane];
            }
        __syncthreads();
    }
    if (w == 0) sm[0][0][lane] = SM / (double)Cg;
    __syncthreads();
    const double mbar = sm[0][0][lane];
    __syncthreads();
    double B = 0.0;
    for (int64_t b0 = 0; b0 < nb; b0 += MT_POOL_WAVES) {
        const int64_t b = b0 + w;
        double sb = 0.0;
        if (valid && b < nb) {
            const int64_t left = Cg - b * DIAG_CHAIN_BLOCK;
            const int cnt = left < DIAG_CHAIN_BLOCK ? (int)left : DIAG_CHAIN_BLOCK;
            for (int q = 0; q < cnt; ++q) {
                const double e = at(b, q).mean(dn) - mbar;
                sb = sb + e * e;
            }
        }
        sm[1][w][lane] = sb;
        __syncthreads();
        if (w == 0)
            for (int s = 0; s < MT_POOL_WAVES && b0 + s < nb; ++s) B = B + sm[1][s][lane];
        __syncthreads();
    }
    if (w != 0 || !valid) return;
    const double N = (double)(a.n * Cg);
    double var = (W + dn * B) / (N - 1.0);
    if (a.regularise) var = (N / (N + 5.0)) * var + 1e-3 * (5.0 / (N + 5.0));   // Stan's shrinkage
    // NaN, inf, zero (a constant dimension, one draw of one chain): the scale stays
    if (var > 0.0 && var <= 1.7976931348623157e308) a.scale[g * a.D + i] = sqrt(var);
}

}  // namespace binf

using namespace binf;

extern "C" int32_t binf_leapfrog_kick_scaled_f64(double *p, const double *grad, const double *scale,
                                                 int64_t G, double timestep, const double *dt_chain,
                                                 int32_t half, int64_t C, int64_t D, int32_t mode,
                                                 void *stream)
{
    return scaled_launch<LF_KICK>(nullptr, p, grad, scale, G, timestep, dt_chain, half, C, D, mode, stream,
                                  "leapfrog_kick_scaled");
}

extern "C" int32_t binf_leapfrog_drift_scaled_f64(double *q, const double *p, const double *scale,
                                                  int64_t G, double timestep, const double *dt_chain,
                                                  int64_t C, int64_t D, int32_t mode, void *stream)
{
    return scaled_launch<LF_DRIFT>(q, const_cast<double *>(p), nullptr, scale, G, timestep, dt_chain, 0, C, D,
                                   mode, stream, "leapfrog_drift_scaled");
}

extern "C" int32_t binf_leapfrog_kick_drift_scaled_f64(double *q, double *p, const double *grad,
                                                       const double *scale, int64_t G, double timestep,
                                                       const double *dt_chain, int64_t C, int64_t D,
                                                       int32_t mode, void *stream)
{
    return scaled_launch<LF_KICK_DRIFT>(q, p, grad, scale, G, timestep, dt_chain, 0, C, D, mode, stream,
                                        "leapfrog_kick_drift_scaled");
}

extern "C" int32_t binf_metric_accumulate_f64(const double *x, double *k0, double *s1, double *s2,
                                              int32_t first, int64_t C, int64_t D, void *stream)
{
    const char *what = "metric_accumulate";
    if (C < 0 || D < 0) return fail(BINF_E_ARG, "%s: negative size", what);
    if (C == 0 || D == 0) return 0;
    if (C > 0x7fffffffffffffffLL / D) return fail(BINF_E_ARG, "%s: C*D overflows", what);
    if (!x || !k0 || !s1 || !s2) return fail(BINF_E_ARG, "%s: null buffer", what);
    const int64_t n = C * D;
    const void *buf[4] = {x, k0, s1, s2};
    for (int o = 0; o < 4; ++o)
        for (int q = o + 1; q < 4; ++q)
            if (overlap_f64(buf[o], n, buf[q], n))
                return fail(BINF_E_ALIAS, "%s: x, k0, s1 and s2 must not overlap", what);
    hipStream_t st = (hipStream_t)stream;
    if (n % 2 == 0 && ew_aligned16(x, k0, s1, s2)) {
        int64_t b = (n / 2 + 255) / 256;
        if (b > (1 << 20)) b = 1 << 20;
        metric_accumulate_kernel<2><<<dim3((unsigned)b), 256, 0, st>>>(x, k0, s1, s2, n, first ? 1 : 0);
    } else {
        int64_t b = (n + 255) / 256;
        if (b > (1 << 20)) b = 1 << 20;
        metric_accumulate_kernel<1><<<dim3((unsigned)b), 256, 0, st>>>(x, k0, s1, s2, n, first ? 1 : 0);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what);
    return 0;
}

extern "C" int32_t binf_metric_pool_f64(const double *k0, const double *s1, const double *s2, int64_t n,
                                        int64_t C, int64_t D, int64_t G, int32_t regularise,
                                        double *scale, void *stream)
{
    const char *what = "metric_pool";
    if (C < 0 || D < 0) return fail(BINF_E_ARG, "%s: negative size", what);
    if (n < 1) return fail(BINF_E_ARG, "%s: n >= 1 draws required, got %lld", what, (long long)n);
    if (G < 1) return fail(BINF_E_ARG, "%s: G >= 1 required, got %lld", what, (long long)G);
    if (C % G != 0)
        return fail(BINF_E_ARG, "%s: C = %lld is not a multiple of G = %lld", what, (long long)C, (long long)G);
    if (C == 0 || D == 0) return 0;
    if (C > 0x7fffffffffffffffLL / D) return fail(BINF_E_ARG, "%s: C*D overflows", what);
    if (!k0 || !s1 || !s2 || !scale) return fail(BINF_E_ARG, "%s: null buffer", what);
    if (n > ((int64_t)1 << 53) / (C / G))
        return fail(BINF_E_UNSUPPORTED, "%s: n * C / G beyond 2^53", what);
    const int64_t CD = C * D;
    if (overlap_f64(scale, G * D, k0, CD) || overlap_f64(scale, G * D, s1, CD) || overlap_f64(scale, G * D, s2, CD))
        return fail(BINF_E_ALIAS, "%s: the scale overlaps the moments", what);
    MetricPoolArgs a;
    a.k0 = k0; a.s1 = s1; a.s2 = s2; a.scale = scale;
    a.n = n; a.C = C; a.D = D; a.G = G; a.ntiles = (D + 63) / 64; a.regularise = regularise ? 1 : 0;
    if (a.ntiles > 0x7fffffffLL / G) return fail(BINF_E_UNSUPPORTED, "%s: G * D too large for one launch", what);
    metric_pool_kernel<<<dim3((unsigned)(G * a.ntiles)), 64 * MT_POOL_WAVES, 0, (hipStream_t)stream>>>(a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what);
    return 0;
}
