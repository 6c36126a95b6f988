// Diagonal HMC metric: the scaled twins of the element-wise leapfrog kernels (generic.hip)
// and the two kernels of the windowed warm-up adaption -- streaming per-chain moments of the
// state, and the pooled per-group variance that becomes the new scale.  Build-defined: the
// reference integrates with the identity mass only (binf/samplers/hmc.py:92-125).  gfx950,
// wave64.
//
// A metric M = diag(1 / s^2) is carried through the WHITENED momentum r = p / sqrt(m): the
// momentum draw stays r ~ N(0, I) and the kinetic energy 0.5 sum r^2, so the energy, accept
// and adaption kernels are used as they are; kick and drift both take the per-element step
//     h = d * s[c % G][i],   d = dt_chain[c] or timestep (0.5 * d first for a half kick)
// (one rounding), then p - h * g and q + p * h, unfused (EXACT) or one fma each (FMA).  With
// s == 1.0, h == d exactly: the bits of the unscaled kernels.
//
// The arithmetic is stated in include/binf_hip.h and restated in numpy by
// tests/metric_ref.py; every multiply and add is rounded separately (common.hpp turns
// contraction off) and every sum over chains has the diagnostics' fixed order.
#include "common.hpp"
#include "diag_core.hpp"

namespace binf {

// ---------------------------------------------------------------------------
// scaled leapfrog pieces
//
// The launch shape of ew_kernel / kick_drift_kernel (generic.hip): a flat grid over the
// C * D elements, a thread owns MT_UNR aligned groups of VEC doubles, the groups of one
// unroll step contiguous across the workgroup.  With an even D and 16-byte aligned bases
// (the scale's too: an even D keeps every row of it aligned) both elements of a pair belong
// to one chain and to neighbouring columns, so the scale is one 16-byte load as well.  The
// scale rows are G * D doubles, read C / G times each: they stay in L2.
// ---------------------------------------------------------------------------
enum { MT_KICK = 0, MT_DRIFT = 1, MT_KICK_DRIFT = 2 };
constexpr int MT_UNR = 2;

struct MetricEwArgs {
    double *q;              // drift, kick_drift: positions
    double *p;              // momenta (read only by the drift)
    const double *g;        // kick, kick_drift: gradient
    const double *scale;    // [G x D]
    const double *dt_chain;
    double timestep;
    int64_t n;              // C * D
    int64_t D;
    int64_t G;
    int32_t half;
};

template <int VEC>
__device__ inline void mt_load(double (&r)[VEC], const double *p, int64_t i)
{
    if (VEC == 2) {
        const double2 v = *reinterpret_cast<const double2 *>(p + i);
        r[0] = v.x;
        r[VEC - 1] = v.y;
    } else {
        r[0] = p[i];
    }
}

template <int VEC>
__device__ inline void mt_store(double *p, int64_t i, const double (&r)[VEC])
{
    if (VEC == 2) {
        double2 v;
        v.x = r[0];
        v.y = r[VEC - 1];
        *reinterpret_cast<double2 *>(p + i) = v;
    } else {
        p[i] = r[0];
    }
}

template <int KIND, bool FMA, int VEC>
__global__ void __launch_bounds__(256) metric_ew_kernel(const MetricEwArgs a)
{
    // 32-bit division whenever it fits: the element index by D, then the chain by G
    const bool small = a.n <= 0xffffffffLL;
    const int64_t span = (int64_t)256 * VEC * MT_UNR;            // elements per workgroup pass
    for (int64_t b0 = (int64_t)blockIdx.x * span; b0 < a.n; b0 += (int64_t)gridDim.x * span) {
        double qv[MT_UNR][VEC], pv[MT_UNR][VEC], gv[MT_UNR][VEC], sv[MT_UNR][VEC], dt[MT_UNR];
        int64_t idx[MT_UNR];
#pragma unroll
        for (int r = 0; r < MT_UNR; ++r) {
            idx[r] = b0 + ((int64_t)r * 256 + threadIdx.x) * VEC;
            if (idx[r] < a.n) {
                const int64_t c = small ? (int64_t)((uint32_t)idx[r] / (uint32_t)a.D) : idx[r] / a.D;
                const int64_t i = idx[r] - c * a.D;
                int64_t row = 0;
                if (a.G > 1) row = small ? (int64_t)((uint32_t)c % (uint32_t)a.G) : c % a.G;
                if (KIND != MT_DRIFT) mt_load<VEC>(gv[r], a.g, idx[r]);
                mt_load<VEC>(pv[r], a.p, idx[r]);
                if (KIND != MT_KICK) mt_load<VEC>(qv[r], a.q, idx[r]);
                mt_load<VEC>(sv[r], a.scale, row * a.D + i);
                dt[r] = a.dt_chain ? a.dt_chain[c] : a.timestep;
            }
        }
#pragma unroll
        for (int r = 0; r < MT_UNR; ++r) {
            if (idx[r] >= a.n) continue;
            double d = dt[r];
            if (KIND == MT_KICK && a.half) d = 0.5 * d;           // "0.5 * timestep" first
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const double h = d * sv[r][v];
                if (KIND != MT_DRIFT)           // p -= h * grad
                    pv[r][v] = FMA ? __builtin_fma(-h, gv[r][v], pv[r][v]) : pv[r][v] - h * gv[r][v];
                if (KIND != MT_KICK)            // q += p * h (the new p after a kick)
                    qv[r][v] = FMA ? __builtin_fma(pv[r][v], h, qv[r][v]) : qv[r][v] + pv[r][v] * h;
            }
            if (KIND != MT_DRIFT) mt_store<VEC>(a.p, idx[r], pv[r]);
            if (KIND != MT_KICK) mt_store<VEC>(a.q, idx[r], qv[r]);
        }
    }
}

static inline bool mt_aligned16(const void *a, const void *b, const void *c = nullptr,
                                const void *d = nullptr)
{
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}

static inline unsigned mt_blocks(int64_t n, int vec)
{
    const int64_t span = (int64_t)256 * vec * MT_UNR;
    int64_t b = (n + span - 1) / span;
    if (b > (1 << 20)) b = 1 << 20;                  // grid-stride beyond 2^20 workgroups
    return (unsigned)b;
}

template <int KIND, int VEC>
static void metric_ew_dispatch(bool fma, const MetricEwArgs &a, hipStream_t st)
{
    const dim3 grid(mt_blocks(a.n, VEC));
    if (fma) metric_ew_kernel<KIND, true, VEC><<<grid, 256, 0, st>>>(a);
    else     metric_ew_kernel<KIND, false, VEC><<<grid, 256, 0, st>>>(a);
}

// exact aliasing of an element-wise input with the output it feeds is the same element in
// the same thread; any other overlap is a race
static inline bool partial_overlap_f64(const void *a, const void *b, int64_t elems)
{
    return a != b && overlap_f64(a, elems, b, elems);
}

template <int KIND>
static int32_t metric_ew_launch(double *q, double *p, const double *g, const double *scale,
                                int64_t G, double timestep, const double *dt_chain, int32_t half,
                                int64_t C, int64_t D, int32_t mode, void *stream, const char *what)
{
    if (C < 0 || D < 0) return fail(BINF_E_ARG, "%s: negative size", what);
    if (mode != BINF_MODE_EXACT && mode != BINF_MODE_FMA)
        return fail(BINF_E_ARG, "%s: unknown mode %d", what, mode);
    if (G < 1) return fail(BINF_E_ARG, "%s: G >= 1 required, got %lld", what, (long long)G);
    if (C % G != 0)
        return fail(BINF_E_ARG, "%s: C = %lld is not a multiple of G = %lld", what, (long long)C, (long long)G);
    if (C == 0 || D == 0) return 0;
    if (C > 0x7fffffffffffffffLL / D) return fail(BINF_E_ARG, "%s: C*D overflows", what);
    if ((KIND != MT_KICK && !q) || !p || (KIND != MT_DRIFT && !g) || !scale)
        return fail(BINF_E_ARG, "%s: null buffer", what);
    const int64_t n = C * D, ns = G * D;
    // written: p (kick, kick_drift), q (drift, kick_drift)
    if ((KIND != MT_DRIFT && overlap_f64(scale, ns, p, n)) || (KIND != MT_KICK && overlap_f64(scale, ns, q, n)))
        return fail(BINF_E_ALIAS, "%s: the scale overlaps a buffer that is written", what);
    if (dt_chain && ((KIND != MT_DRIFT && overlap_f64(dt_chain, C, p, n)) ||
                     (KIND != MT_KICK && overlap_f64(dt_chain, C, q, n))))
        return fail(BINF_E_ALIAS, "%s: dt_chain overlaps a buffer that is written", what);
    if (KIND != MT_KICK && overlap_f64(q, n, p, n)) return fail(BINF_E_ALIAS, "%s: q overlaps p", what);
    if (KIND != MT_DRIFT && (partial_overlap_f64(g, p, n) || (KIND == MT_KICK_DRIFT && overlap_f64(g, n, q, n))))
        return fail(BINF_E_ALIAS, "%s: the gradient overlaps a buffer that is written", what);
    MetricEwArgs a;
    a.q = q; a.p = p; a.g = g; a.scale = scale; a.dt_chain = dt_chain; a.timestep = timestep;
    a.n = n; a.D = D; a.G = G; a.half = half ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    const bool fma = mode == BINF_MODE_FMA;
    if (D % 2 == 0 && mt_aligned16(q, p, g, scale)) metric_ew_dispatch<KIND, 2>(fma, a, st);
    else                                            metric_ew_dispatch<KIND, 1>(fma, a, st);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what);
    return 0;
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
        mt_load<VEC>(xv, x, i);
        if (!first) {
            mt_load<VEC>(kv, k0, i);
            mt_load<VEC>(av, s1, i);
            mt_load<VEC>(bv, s2, i);
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
        if (first) mt_store<VEC>(k0, i, kv);
        mt_store<VEC>(s1, i, av);
        mt_store<VEC>(s2, i, bv);
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
    return metric_ew_launch<MT_KICK>(nullptr, p, grad, scale, G, timestep, dt_chain, half, C, D, mode,
                                     stream, "leapfrog_kick_scaled");
}

extern "C" int32_t binf_leapfrog_drift_scaled_f64(double *q, const double *p, const double *scale,
                                                  int64_t G, double timestep, const double *dt_chain,
                                                  int64_t C, int64_t D, int32_t mode, void *stream)
{
    return metric_ew_launch<MT_DRIFT>(q, const_cast<double *>(p), nullptr, scale, G, timestep, dt_chain, 0,
                                      C, D, mode, stream, "leapfrog_drift_scaled");
}

extern "C" int32_t binf_leapfrog_kick_drift_scaled_f64(double *q, double *p, const double *grad,
                                                       const double *scale, int64_t G, double timestep,
                                                       const double *dt_chain, int64_t C, int64_t D,
                                                       int32_t mode, void *stream)
{
    return metric_ew_launch<MT_KICK_DRIFT>(q, p, grad, scale, G, timestep, dt_chain, 0, C, D, mode, stream,
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
    if (n % 2 == 0 && mt_aligned16(x, k0, s1, s2)) {
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
