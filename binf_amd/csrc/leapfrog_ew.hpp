// The element-wise leapfrog kernel -- kick, drift and kick_drift, with the identity mass or a
// diagonal metric -- its launcher, and the argument check that every metric entry point
// (scaled: metric.hip, dense: dense_metric.hip) runs before it launches.  gfx950, wave64.
//
// Reference lines replaced: binf/samplers/hmc.py:116-123.  Per element, with
//     d = dt_chain[c] or timestep (0.5 * d first for a half kick)
//     h = d                       identity
//     h = d * s[c % G][i]         diagonal metric M = diag(1 / s^2) (one rounding)
// a kick is p - h * g and a drift q + p * h, unfused (EXACT) or one fma each (FMA); a
// kick_drift is the kick, then the drift with the new p, in one pass over memory.  The
// arithmetic is stated in include/binf_hip.h and restated in numpy by tests/metric_ref.py
// (a scale of ones is the identity, bit for bit).
#pragma once
#include "common.hpp"

namespace binf {

// the pieces of a leapfrog step, for the element-wise and the dense kernels alike
enum { LF_KICK = 0, LF_DRIFT = 1, LF_KICK_DRIFT = 2 };

// ---------------------------------------------------------------------------
// Flat grid over the C*D elements, 16-byte accesses: a thread owns EW_UNR aligned groups of
// VEC doubles (the groups of one unroll step are contiguous across the workgroup, so every
// load / store instruction of a wave covers 1 KiB).  With an even D both elements of a pair
// belong to one chain and to neighbouring columns (the scale is then one 16-byte load as
// well: an even D keeps every row of it aligned); odd D or a pointer that is only 8-byte
// aligned (a view into a larger tensor) takes the VEC = 1 variant.  The per-chain step size,
// if any, is looked up from the element index.  The scale rows are G * D doubles, read C / G
// times each: they stay in L2.
// ---------------------------------------------------------------------------
constexpr int EW_UNR = 2;

template <int VEC>
__device__ inline void ew_load(double (&r)[VEC], const double *p, int64_t i)
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
__device__ inline void ew_store(double *p, int64_t i, const double (&r)[VEC])
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

static inline bool ew_aligned16(const void *a, const void *b, const void *c = nullptr,
                                const void *d = nullptr)
{
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}

static inline unsigned ew_blocks(int64_t n, int vec)
{
    const int64_t span = (int64_t)256 * vec * EW_UNR;
    int64_t b = (n + span - 1) / span;
    if (b > (1 << 20)) b = 1 << 20;                  // grid-stride beyond 2^20 workgroups
    return (unsigned)b;
}

// chain of element i (row-major [C x D]); 32-bit division whenever it fits
__device__ inline int64_t chain_of(int64_t i, int64_t D, bool small)
{
    return small ? (int64_t)((uint32_t)i / (uint32_t)D) : i / D;
}

// The kernel's arguments are what the instantiation reads and no more: seven that every piece
// takes (LeapfrogEwArgs), then those of LeapfrogEwExtra<KIND, SCALED> one by one -- the scale
// and its G with a diagonal metric, `half` for a kick, nothing for the identity drift and
// kick_drift, whose 56 bytes and the launch geometry behind them then share one 64-byte line
// of kernel arguments (with three unread arguments in between, kick_drift measured 0.7 %
// slower at 4096 x 1024).  Scalars, not one struct: as a struct the identity kick_drift,
// VEC = 2, is allocated two more SGPRs.
struct LeapfrogEwArgs {
    double *q;              // drift, kick_drift: positions
    double *p;              // momenta (read only by the drift)
    const double *g;        // kick, kick_drift: gradient
    double timestep;
    const double *dt_chain;
    int64_t n;              // C * D
    int64_t D;
};

template <int KIND, bool SCALED>
struct LeapfrogEwExtra {};
template <>
struct LeapfrogEwExtra<LF_KICK, false> {
    int32_t half;
};
template <int KIND>
struct LeapfrogEwExtra<KIND, true> {
    const double *scale;    // [G x D]
    int64_t G;
};
template <>
struct LeapfrogEwExtra<LF_KICK, true> {
    const double *scale;
    int64_t G;
    int32_t half;
};

template <int KIND, bool SCALED, bool FMA, int VEC, class... Extra>
__global__ void __launch_bounds__(256)
leapfrog_ew_kernel(double *q, double *p, const double *g, double timestep, const double *dt_chain, int64_t n,
                   int64_t D, Extra... extra)
{
    const LeapfrogEwExtra<KIND, SCALED> x{extra...};
    const bool small = n <= 0xffffffffLL;
    const int64_t span = (int64_t)256 * VEC * EW_UNR;             // elements per workgroup pass
    for (int64_t b0 = (int64_t)blockIdx.x * span; b0 < n; b0 += (int64_t)gridDim.x * span) {
        double qv[EW_UNR][VEC], pv[EW_UNR][VEC], gv[EW_UNR][VEC], sv[EW_UNR][VEC], dt[EW_UNR];
        int64_t idx[EW_UNR];
#pragma unroll
        for (int r = 0; r < EW_UNR; ++r) {
            idx[r] = b0 + ((int64_t)r * 256 + threadIdx.x) * VEC;
            if (idx[r] < n) {
                int64_t c = 0, s_at = 0;
                if constexpr (SCALED) {
                    // the chain by D, then its scale row by G (32-bit division whenever it fits)
                    const int64_t G = x.G;
                    c = chain_of(idx[r], D, small);
                    const int64_t i = idx[r] - c * D;
                    int64_t row = 0;
                    if (G > 1) row = small ? (int64_t)((uint32_t)c % (uint32_t)G) : c % G;
                    s_at = row * D + i;
                }
                if (KIND != LF_DRIFT) ew_load<VEC>(gv[r], g, idx[r]);
                ew_load<VEC>(pv[r], p, idx[r]);
                if (KIND != LF_KICK) ew_load<VEC>(qv[r], q, idx[r]);
                if constexpr (SCALED) ew_load<VEC>(sv[r], x.scale, s_at);
                // without a scale the chain is needed for a per-chain step only
                dt[r] = dt_chain ? dt_chain[SCALED ? c : chain_of(idx[r], D, small)] : timestep;
            }
        }
#pragma unroll
        for (int r = 0; r < EW_UNR; ++r) {
            if (idx[r] >= n) continue;
            double d = dt[r];
            if constexpr (KIND == LF_KICK)
                if (x.half) d = 0.5 * d;                          // "0.5 * timestep" first
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const double h = SCALED ? d * sv[r][v] : d;
                if (KIND != LF_DRIFT)           // p -= h * grad                 hmc.py:116,120,123
                    pv[r][v] = FMA ? __builtin_fma(-h, gv[r][v], pv[r][v]) : pv[r][v] - h * gv[r][v];
                if (KIND != LF_KICK)            // q += p * h (the new p after a kick)   hmc.py:119,122
                    qv[r][v] = FMA ? __builtin_fma(pv[r][v], h, qv[r][v]) : qv[r][v] + pv[r][v] * h;
            }
            if (KIND != LF_DRIFT) ew_store<VEC>(p, idx[r], pv[r]);
            if (KIND != LF_KICK) ew_store<VEC>(q, idx[r], qv[r]);
        }
    }
}

template <int KIND, bool SCALED, bool FMA, int VEC>
static void leapfrog_ew_enqueue(const LeapfrogEwArgs &a, const LeapfrogEwExtra<KIND, SCALED> &x, hipStream_t st)
{
    auto kernel = [&](auto... extra) {
        leapfrog_ew_kernel<KIND, SCALED, FMA, VEC><<<dim3(ew_blocks(a.n, VEC)), 256, 0, st>>>(
            a.q, a.p, a.g, a.timestep, a.dt_chain, a.n, a.D, extra...);
    };
    if constexpr (SCALED && KIND == LF_KICK) kernel(x.scale, x.G, x.half);
    else if constexpr (SCALED) kernel(x.scale, x.G);
    else if constexpr (KIND == LF_KICK) kernel(x.half);
    else kernel();
}

// launches the checked arguments: VEC = 2 for an even D on 16-byte aligned bases
template <int KIND, bool SCALED>
static int32_t leapfrog_ew_launch(const LeapfrogEwArgs &a, const LeapfrogEwExtra<KIND, SCALED> &x, int32_t mode,
                                  void *stream, const char *what)
{
    hipStream_t st = (hipStream_t)stream;
    const bool fma = mode == BINF_MODE_FMA;
    const void *scale = nullptr;
    if constexpr (SCALED) scale = x.scale;
    if (a.D % 2 == 0 && ew_aligned16(a.q, a.p, a.g, scale)) {
        if (fma) leapfrog_ew_enqueue<KIND, SCALED, true, 2>(a, x, st);
        else     leapfrog_ew_enqueue<KIND, SCALED, false, 2>(a, x, st);
    } else {
        if (fma) leapfrog_ew_enqueue<KIND, SCALED, true, 1>(a, x, st);
        else     leapfrog_ew_enqueue<KIND, SCALED, false, 1>(a, x, st);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what);
    return 0;
}

// ---------------------------------------------------------------------------
// the argument check of the metric entry points (scaled and dense), in two steps so that the
// dense launcher can put its limit on D between them, where it always stood: the sizes, then
// -- for a call that has something to do (C > 0 and D > 0) -- the overflows and the buffers.
// `metric` is the scale or the factor, G groups of `group_elems` doubles (D, or D * D of a
// D that the launcher has bounded), `noun` its name in the messages.
// ---------------------------------------------------------------------------
static inline int32_t leapfrog_check_sizes(int64_t G, int64_t C, int64_t D, int32_t mode, const char *what)
{
    if (C < 0 || D < 0) return fail(BINF_E_ARG, "%s: negative size", what);
    if (mode != BINF_MODE_EXACT && mode != BINF_MODE_FMA)
        return fail(BINF_E_ARG, "%s: unknown mode %d", what, mode);
    if (G < 1) return fail(BINF_E_ARG, "%s: G >= 1 required, got %lld", what, (long long)G);
    if (C % G != 0)
        return fail(BINF_E_ARG, "%s: C = %lld is not a multiple of G = %lld", what, (long long)C, (long long)G);
    return 0;
}

// exact aliasing of an element-wise input with the output it feeds is the same element in
// the same thread (the dense kernels stage the gradient before they write); any other
// overlap is a race
static inline bool partial_overlap_f64(const void *a, const void *b, int64_t elems)
{
    return a != b && overlap_f64(a, elems, b, elems);
}

template <int KIND>
static int32_t leapfrog_check(const double *q, const double *p, const double *g, const double *metric,
                              int64_t G, int64_t group_elems, const char *noun, const double *dt_chain,
                              int64_t C, int64_t D, const char *what)
{
    if (C > 0x7fffffffffffffffLL / D) return fail(BINF_E_ARG, "%s: C*D overflows", what);
    // (a factor only: the G * D doubles of a scale are no more than C * D)
    if (G > 0x7fffffffffffffffLL / group_elems) return fail(BINF_E_ARG, "%s: G*D*D overflows", what);
    if ((KIND != LF_KICK && !q) || !p || (KIND != LF_DRIFT && !g) || !metric)
        return fail(BINF_E_ARG, "%s: null buffer", what);
    const int64_t n = C * D, metric_elems = G * group_elems;
    // written: p (kick, kick_drift), q (drift, kick_drift)
    if ((KIND != LF_DRIFT && overlap_f64(metric, metric_elems, p, n)) ||
        (KIND != LF_KICK && overlap_f64(metric, metric_elems, q, n)))
        return fail(BINF_E_ALIAS, "%s: the %s overlaps a buffer that is written", what, noun);
    if (dt_chain && ((KIND != LF_DRIFT && overlap_f64(dt_chain, C, p, n)) ||
                     (KIND != LF_KICK && overlap_f64(dt_chain, C, q, n))))
        return fail(BINF_E_ALIAS, "%s: dt_chain overlaps a buffer that is written", what);
    if (KIND != LF_KICK && overlap_f64(q, n, p, n)) return fail(BINF_E_ALIAS, "%s: q overlaps p", what);
    if (KIND != LF_DRIFT && (partial_overlap_f64(g, p, n) || (KIND == LF_KICK_DRIFT && overlap_f64(g, n, q, n))))
        return fail(BINF_E_ALIAS, "%s: the gradient overlaps a buffer that is written", what);
    return 0;
}

}  // namespace binf
