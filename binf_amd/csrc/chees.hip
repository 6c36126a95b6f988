// ChEES criterion: the cross-chain statistic an adapting ChEESSampler learns its trajectory
// length from (Hoffman, Radul & Sountsov 2021).  The contract -- every sum's order -- is in
// include/binf_hip.h; the host restatement is tests/chees_ref.py.  gfx950, wave64.
//
//   accept_prob  one lane per chain.
//   means        a workgroup per (chunk of BINF_CHEES_CHUNK chains, tile of columns): one lane
//                per column (two with 16-byte accesses) walks down the chunk, so a wave's loads
//                are whole lines along D; partials to the slab, a finishing launch adds a
//                column's partials in ascending chunk order and divides once.
//   terms        one chain per group of 8 ... 256 lanes of a 256-thread workgroup, sized to the
//                row's pairwise tree (nuts.hip's geometry): a pairwise leaf belongs to 8 lanes,
//                which load their elements of the three rows ONCE and form the leaf's three
//                sums in rowsum.hpp's order; the leaves are joined in LDS, one lane per sum.
//   sums         a wave per chunk, one lane per chain, the balanced tree over neighbouring
//                lanes; chunk sums to the slab, a finishing launch adds them in ascending order.
// Plain stores and launch boundaries only.  Exact arithmetic (common.hpp: no contraction).
#include "rowsum.hpp"
#include "gauss_common.hpp"

namespace binf {

constexpr int CHEES_CHUNK = BINF_CHEES_CHUNK;
constexpr int CHEES_LEAF_T = PW_BLOCK / 8;      // elements of a full pairwise leaf per lane
static_assert(CHEES_CHUNK == 64, "a chunk of the sums is one wave");

__device__ inline bool chees_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }

// ---- accept_prob ---------------------------------------------------------------------
__global__ void __launch_bounds__(256)
chees_accept_prob_kernel(const double *e_before, const double *e_after, double *alpha, int64_t C)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const double ea = e_after[c];
    double x = e_before[c] - ea;
    const bool ok = chees_finite(ea) && x == x;
    x = (x < -308.0) ? -308.0 : x;
    x = (x > 709.0) ? 709.0 : x;
    double y = exp_clipped_range(ok ? x : 0.0);
    y = (y < 1.0) ? y : 1.0;
    alpha[c] = ok ? y : 0.0;
}

// ---- means -----------------------------------------------------------------------------
template <int VEC>
__device__ inline void chees_ld(double (&x)[VEC], const double *p)
{
    if (VEC == 2) {
        const double2 t = *reinterpret_cast<const double2 *>(p);
        x[0] = t.x;
        x[VEC - 1] = t.y;
    } else {
        x[0] = p[0];
    }
}

template <int VEC>
__global__ void __launch_bounds__(256)
chees_means_kernel(const double *q, const double *q_prop, const double *alpha, double *slab,
                   int64_t C, int64_t D, int64_t ntiles, int64_t nch)
{
    const int64_t chunk = blockIdx.x / ntiles, tile = blockIdx.x % ntiles;
    const int64_t col = (tile * 256 + threadIdx.x) * VEC;
    if (col >= D) return;
    const int64_t c0 = chunk * CHEES_CHUNK;
    const int64_t c1 = (C - c0 < CHEES_CHUNK) ? C : c0 + CHEES_CHUNK;
    double sq[VEC], sp[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) { sq[e] = 0.0; sp[e] = 0.0; }
#pragma unroll 4
    for (int64_t c = c0; c < c1; ++c) {
        const bool moved = alpha[c] > 0.0;              // the same for every lane of the workgroup
        double x[VEC], y[VEC];
        chees_ld<VEC>(x, q + c * D + col);
        if (moved) {
            chees_ld<VEC>(y, q_prop + c * D + col);
        } else {
#pragma unroll
            for (int e = 0; e < VEC; ++e) y[e] = x[e];
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e) { sq[e] = sq[e] + x[e]; sp[e] = sp[e] + y[e]; }
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        slab[chunk * D + col + e] = sq[e];
        slab[(nch + chunk) * D + col + e] = sp[e];
    }
}

__global__ void __launch_bounds__(256)
chees_means_finish_kernel(const double *slab, double *mean_q, double *mean_prop, int64_t C,
                          int64_t D, int64_t nch)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * D) return;
    const int64_t which = i / D, d = i % D;
    const double *p = slab + which * nch * D + d;
    double tot = 0.0;
    for (int64_t k = 0; k < nch; ++k) tot = tot + p[k * D];
    const double m = tot / (double)C;
    (which ? mean_prop : mean_q)[d] = m;
}

// ---- terms -----------------------------------------------------------------------------
struct CheesGeom {
    int32_t lpc;     // lanes per chain (power of two, 8 ... 256)
    int32_t H;       // pairwise tree height of a row
};

// The end of a pairwise leaf's sum as rowsum.hpp's leaf_sum_f forms it: the 8 lanes' running
// sums joined as ((0+1)+(2+3))+((4+5)+(6+7)), then the leaf's tail elements (len % 8, or all of
// a leaf shorter than 8) one after the other.  The 8 lanes of a group call it together.
__device__ inline double chees_leaf_end(double run, double tail, int T, int rem, int lane)
{
    const double r = sum8_f64(run);
    double res = (T > 0) ? r : -0.0;
    if (__any(rem != 0)) {
        const int leafbase = lane & ~7;
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            const double v = shfl_f64(tail, leafbase + i);
            const double s = res + v;
            res = (i < rem) ? s : res;
        }
    }
    return res;
}

__global__ void __launch_bounds__(256)
chees_terms_kernel(const double *q, const double *q_prop, const double *v, const double *alpha,
                   const double *mean_q, const double *mean_prop, double *g, int64_t C, int32_t D,
                   const CheesGeom geo)
{
    extern __shared__ double S[];                 // [chains of the workgroup][3][paths], then dep[paths]
    const int H = geo.H, npaths = 1 << H, lpc = geo.lpc, cpb = 256 / lpc;
    int *dep = reinterpret_cast<int *>(S + cpb * 3 * npaths);
    const int lane = threadIdx.x & 63, j = lane & 7;
    const int sub = threadIdx.x & (lpc - 1), cl = threadIdx.x / lpc;
    const int64_t c = (int64_t)blockIdx.x * cpb + cl;
    if ((int)threadIdx.x < npaths) dep[threadIdx.x] = pairwise_leaf(D, H, threadIdx.x).depth;
    const bool inb = c < C;
    const bool active = inb && alpha[c] > 0.0;     // a chain with alpha == 0: g = +0.0, nothing read
    const int64_t row = inb ? c * (int64_t)D : 0;
    const double *rq = q + row, *rp = q_prop + row, *rv = v + row;
    const int base = cl * 3 * npaths;
    const int nsub8 = lpc >> 3, s8 = sub >> 3;
    // the loop runs to the largest count among the wave's chains, so the cross-lane moves of
    // chees_leaf_end see whole groups
    for (int path = s8; __any(active && path < npaths); path += nsub8) {
        const bool act = active && path < npaths;
        const Leaf L = pairwise_leaf(D, H, act ? path : 0);
        const int T = (L.len >= 8) ? (L.len >> 3) : 0;
        const int rem = (L.len >= 8) ? (L.len & 7) : L.len;
        const int e0 = L.off + j;                  // the lane's element t is e0 + 8 t, its tail e0 + 8 T
        const bool tl = act && j < rem;
        double sa = 0.0, sb = 0.0, ss = 0.0, ta = 0.0, tb = 0.0, ts = 0.0;
#pragma unroll 4
        for (int t = 0; t < CHEES_LEAF_T; ++t)
            if (act && t < T) {
                const int e = e0 + 8 * t;
                const double xp = rp[e] - mean_prop[e], xq = rq[e] - mean_q[e];
                const double va = xp * xp, vb = xq * xq, vs = xp * rv[e];
                sa = (t == 0) ? va : sa + va;
                sb = (t == 0) ? vb : sb + vb;
                ss = (t == 0) ? vs : ss + vs;
            }
        if (tl) {
            const int e = e0 + 8 * T;
            const double xp = rp[e] - mean_prop[e], xq = rq[e] - mean_q[e];
            ta = xp * xp; tb = xq * xq; ts = xp * rv[e];
        }
        const double ra = chees_leaf_end(sa, ta, T, rem, lane);
        const double rb = chees_leaf_end(sb, tb, T, rem, lane);
        const double rs = chees_leaf_end(ss, ts, T, rem, lane);
        if (act && j == 0) {
            S[base + path] = ra;
            S[base + npaths + path] = rb;
            S[base + 2 * npaths + path] = rs;
        }
    }
    __syncthreads();
    if (active && sub < 3) {
        double *T_ = S + base + sub * npaths;
        for (int l = 0; l < H; ++l)
            for (int p = 0; p < npaths; p += (2 << l))
                if (dep[p] >= H - l) T_[p] = T_[p] + T_[p + (1 << l)];
    }
    __syncthreads();
    if (!inb || sub != 0) return;
    double out = 0.0;
    if (active) {
        const double a = 0.0 + S[base], b = 0.0 + S[base + npaths], s = 0.0 + S[base + 2 * npaths];
        out = (a - b) * s;
    }
    g[c] = out;
}

// ---- sums ------------------------------------------------------------------------------
// all lanes: the balanced tree over neighbouring lanes (2, 4, 8, 16, 32, 64)
__device__ inline double chees_wave_sum(double r, int lane)
{
    r = sum8_f64(r);
#pragma unroll
    for (int l = 0; l < 3; ++l) r = r + xor_level_f64(r, l, lane);
    return r;
}

__global__ void __launch_bounds__(256)
chees_sums_kernel(const double *alpha, const double *g, double *slab, int64_t C, int64_t nch)
{
    const int lane = threadIdx.x & 63;
    const int64_t chunk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (chunk >= nch) return;                       // the whole wave
    const int64_t c = chunk * CHEES_CHUNK + lane;
    const bool inb = c < C;
    const double al = inb ? alpha[c] : 0.0, gg = inb ? g[c] : 0.0;
    const bool fin = chees_finite(gg);
    double t0 = (inb && fin) ? al * gg : 0.0;
    double t1 = (inb && fin) ? al : 0.0;
    double t2 = inb ? 1.0 / al : 0.0;
    double t3 = (inb && !fin) ? 1.0 : 0.0;
    t0 = chees_wave_sum(t0, lane);
    t1 = chees_wave_sum(t1, lane);
    t2 = chees_wave_sum(t2, lane);
    t3 = chees_wave_sum(t3, lane);
    if (lane == 0) {
        double *o = slab + chunk * 4;
        o[0] = t0; o[1] = t1; o[2] = t2; o[3] = t3;
    }
}

__global__ void __launch_bounds__(64)
chees_sums_finish_kernel(const double *slab, double *out, int64_t nch)
{
    if (threadIdx.x >= 4) return;
    double tot = 0.0;
    for (int64_t k = 0; k < nch; ++k) tot = tot + slab[k * 4 + threadIdx.x];
    out[threadIdx.x] = tot;
}

// ---- host ------------------------------------------------------------------------------
struct CheesSpan { const void *p; int64_t elems; const char *name; };

static int32_t chees_shape(int64_t C, int64_t D, const char *what)
{
    if (C < 1 || D < 1) return fail(BINF_E_ARG, "%s: C >= 1 and D >= 1 required", what);
    if (C > 0x7fffffffLL || D > 0x7fffffffLL || C > (1LL << 53) / D)
        return fail(BINF_E_UNSUPPORTED, "%s: too large", what);
    return 0;
}

// nin inputs first, then the outputs: no NULL, no output overlapping anything
static int32_t chees_spans(const CheesSpan *sp, int n, int nin, const char *what)
{
    for (int i = 0; i < n; ++i)
        if (!sp[i].p) return fail(BINF_E_ARG, "%s: null buffer %s", what, sp[i].name);
    for (int i = nin; i < n; ++i)
        for (int k = 0; k < i; ++k)
            if (overlap_f64(sp[i].p, sp[i].elems, sp[k].p, sp[k].elems))
                return fail(BINF_E_ALIAS, "%s: %s overlaps %s", what, sp[i].name, sp[k].name);
    return 0;
}

static int64_t chees_chunks(int64_t C) { return (C + CHEES_CHUNK - 1) / CHEES_CHUNK; }

}  // namespace binf

using namespace binf;

extern "C" int32_t binf_chees_accept_prob_f64(const double *e_before, const double *e_after,
                                              double *alpha, int64_t C, void *stream)
{
    const char *what = "chees_accept_prob";
    const int32_t rc = chees_shape(C, 1, what);
    if (rc) return rc;
    if (!e_before || !e_after || !alpha) return fail(BINF_E_ARG, "%s: null buffer", what);
    if ((alpha != e_before && overlap_f64(alpha, C, e_before, C)) ||
        (alpha != e_after && overlap_f64(alpha, C, e_after, C)))
        return fail(BINF_E_ALIAS, "%s: alpha overlaps an input in part", what);
    chees_accept_prob_kernel<<<dim3((unsigned)((C + 255) / 256)), 256, 0, (hipStream_t)stream>>>(
        e_before, e_after, alpha, C);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what);
    return 0;
}

extern "C" int64_t binf_chees_workspace_bytes(int64_t C, int64_t D)
{
    if (C < 1 || D < 1 || C > 0x7fffffffLL || D > 0x7fffffffLL || C > (1LL << 53) / D) return 0;
    return chees_chunks(C) * (2 * D > 4 ? 2 * D : 4) * 8;
}

extern "C" int32_t binf_chees_means_f64(const double *q, const double *q_prop, const double *alpha,
                                        double *slab, double *mean_q, double *mean_prop, int64_t C,
                                        int64_t D, void *stream)
{
    const char *what = "chees_means";
    int32_t rc = chees_shape(C, D, what);
    if (rc) return rc;
    const int64_t nch = chees_chunks(C);
    const CheesSpan sp[] = {{q, C * D, "q"}, {q_prop, C * D, "q_prop"}, {alpha, C, "alpha"},
                            {slab, 2 * nch * D, "slab"}, {mean_q, D, "mean_q"}, {mean_prop, D, "mean_prop"}};
    rc = chees_spans(sp, 6, 3, what);
    if (rc) return rc;
    if (((uintptr_t)slab) & 7) return fail(BINF_E_ARG, "%s: misaligned slab", what);
    const bool vec2 = D % 2 == 0 && ((((uintptr_t)q) | ((uintptr_t)q_prop)) & 15) == 0;
    const int64_t per = vec2 ? 512 : 256;
    const int64_t ntiles = (D + per - 1) / per;
    if (ntiles > 0x7fffffffLL / nch) return fail(BINF_E_UNSUPPORTED, "%s: too large", what);
    const dim3 grid((unsigned)(nch * ntiles));
    hipStream_t st = (hipStream_t)stream;
    if (vec2) chees_means_kernel<2><<<grid, 256, 0, st>>>(q, q_prop, alpha, slab, C, D, ntiles, nch);
    else      chees_means_kernel<1><<<grid, 256, 0, st>>>(q, q_prop, alpha, slab, C, D, ntiles, nch);
    chees_means_finish_kernel<<<dim3((unsigned)((2 * D + 255) / 256)), 256, 0, st>>>(
        slab, mean_q, mean_prop, C, D, nch);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what);
    return 0;
}

extern "C" int32_t binf_chees_terms_f64(const double *q, const double *q_prop, const double *v,
                                        const double *alpha, const double *mean_q,
                                        const double *mean_prop, double *g, int64_t C, int64_t D,
                                        void *stream)
{
    const char *what = "chees_terms";
    int32_t rc = chees_shape(C, D, what);
    if (rc) return rc;
    if (D > NPY_BUFSIZE) return fail(BINF_E_UNSUPPORTED, "%s: rows beyond %d elements", what, NPY_BUFSIZE);
    const CheesSpan sp[] = {{q, C * D, "q"}, {q_prop, C * D, "q_prop"}, {v, C * D, "v"}, {alpha, C, "alpha"},
                            {mean_q, D, "mean_q"}, {mean_prop, D, "mean_prop"}, {g, C, "g"}};
    rc = chees_spans(sp, 7, 6, what);
    if (rc) return rc;
    CheesGeom geo;
    geo.H = pairwise_tree_height(D);              // at most 7 for D <= NPY_BUFSIZE: dep[128]
    geo.lpc = 8 << (geo.H < 5 ? geo.H : 5);
    const int cpb = 256 / geo.lpc;
    const size_t lds = ((size_t)(cpb * 3) << geo.H) * sizeof(double) + ((size_t)1 << geo.H) * sizeof(int);
    const int64_t blocks = (C + cpb - 1) / cpb;
    chees_terms_kernel<<<dim3((unsigned)blocks), 256, lds, (hipStream_t)stream>>>(
        q, q_prop, v, alpha, mean_q, mean_prop, g, C, (int32_t)D, geo);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what);
    return 0;
}

extern "C" int32_t binf_chees_sums_f64(const double *alpha, const double *g, double *slab,
                                       double *out, int64_t C, void *stream)
{
    const char *what = "chees_sums";
    int32_t rc = chees_shape(C, 1, what);
    if (rc) return rc;
    const int64_t nch = chees_chunks(C);
    const CheesSpan sp[] = {{alpha, C, "alpha"}, {g, C, "g"}, {slab, 4 * nch, "slab"}, {out, 4, "out"}};
    rc = chees_spans(sp, 4, 2, what);
    if (rc) return rc;
    if (((uintptr_t)slab) & 7) return fail(BINF_E_ARG, "%s: misaligned slab", what);
    hipStream_t st = (hipStream_t)stream;
    chees_sums_kernel<<<dim3((unsigned)((nch + 3) / 4)), 256, 0, st>>>(alpha, g, slab, C, nch);
    chees_sums_finish_kernel<<<dim3(1), 64, 0, st>>>(slab, out, nch);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what);
    return 0;
}
