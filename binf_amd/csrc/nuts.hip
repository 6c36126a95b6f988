// No-U-turn sampler: the tree of every chain, built leaf by leaf on the device.
// The contract (the transition, line by line) is in include/binf_hip.h; the host
// restatement is tests/nuts_ref.py.  gfx950, wave64.
//
// One chain per group of G = 8 ... 256 lanes of a 256-thread workgroup (a power of two
// sized to the row), so short rows share a workgroup.  A leaf is three phases:
//   1. ONE pass over r: every dot product the leaf can need -- the kinetic energy, the
//      sub-tree checks against the checkpoints, the whole-tree check of a merge -- summed per
//      pairwise leaf by the leaf's group of 8 lanes from its elements of r held in registers
//      (rowsum.hpp's order: numpy's), formed from the rows as they stand BEFORE the leaf's updates;
//   2. the pairwise trees joined, one lane per dot, in LDS;
//   3. the chain's branch, evaluated by every lane of the chain from the same scalars (same
//      bits: the branch is uniform over the chain's lanes), then ONE pass over the row that
//      does every copy and update the branch asks for, 16 bytes per access where the row
//      length and the bases allow it.
// LDS: the reduction's partial sums only.  No scratch.
#include "rowsum.hpp"
#include "gauss_common.hpp"

namespace binf {

__device__ inline double nuts_expc(double x)
{
    x = (x < -308.0) ? -308.0 : x;
    x = (x > 709.0) ? 709.0 : x;
    return exp_clipped_range(x);
}

template <int VEC>
__device__ inline void nuts_ld(double (&x)[VEC], const double *p, int64_t i)
{
    if (VEC == 2) {
        const double2 t = *reinterpret_cast<const double2 *>(p + i);
        x[0] = t.x;
        x[VEC - 1] = t.y;
    } else {
        x[0] = p[i];
    }
}

template <int VEC>
__device__ inline void nuts_st(double *p, int64_t i, const double (&x)[VEC])
{
    if (VEC == 2) {
        double2 t;
        t.x = x[0];
        t.y = x[VEC - 1];
        *reinterpret_cast<double2 *>(p + i) = t;
    } else {
        p[i] = x[0];
    }
}

struct NutsGeom {
    int32_t lpc;     // lanes per chain (power of two, 8 ... 256)
    int32_t H;       // pairwise tree height of a row
    int32_t ndots;   // dots a chain can need in one call (LDS stride)
};

// what a chain's lanes know about its leaf before the sums
struct NutsPlan {
    bool active;
    int32_t n, j, v, hi, nchk, ndots;
    bool merge;
};

// The end of a pairwise leaf's sum as rowsum.hpp's leaf_sum_f forms it: the 8 lanes' running sums
// joined as ((0+1)+(2+3))+((4+5)+(6+7)), then the leaf's tail elements (len % 8, or all of a leaf
// shorter than 8) added one after the other.  `run` is the lane's sum over its elements 8t + j,
// `tail` its tail element's term (0.0 where it has none).  The 8 lanes of a group call it together.
__device__ inline double nuts_leaf_end(double run, double tail, int T, int rem, int lane)
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

constexpr int NUTS_LEAF_T = PW_BLOCK / 8;      // elements of a full pairwise leaf per lane

// Phases 1 and 2.  Every thread of the workgroup calls it (barriers); afterwards dot k of the
// chain is 0.0 + S[base + (k << H)].
//
// Phase 1 is ONE pass over r: a pairwise leaf of the row (<= 128 elements) belongs to a group of
// 8 lanes, which loads its at most 17 elements per lane of r once, keeps them in registers, and
// forms from them the leaf's sum of EVERY dot the chain needs -- the kinetic energy, then per
// checkpoint level the pair (ck_r . sub, r . sub) from one read of that level's two rows, then
// the merge's pair from one read of rho_tree and of the far edge (rho_sub is read again per pair,
// from cache: in registers beside r it cost a wave per SIMD).  Per dot the additions are
// leaf_sum_f's, in its order.  The loops over levels run to the largest count among
// the wave's chains (a flag masks the rest), so the cross-lane moves see whole groups.
__device__ inline void nuts_dots(const binf_nuts_args &a, const NutsGeom &geo, const NutsPlan &pl,
                                 int64_t c, int sub, double *S, int *dep, int base)
{
    const int H = geo.H, npaths = 1 << H, D = (int)a.D;
    const int lane = threadIdx.x & 63, j = lane & 7;
    if ((int)threadIdx.x < npaths) dep[threadIdx.x] = pairwise_leaf(D, H, threadIdx.x).depth;
    const int64_t row = c * a.D;
    const double *rr = a.r + row, *rsub = a.rho_sub + row, *rtree = a.rho_tree + row;
    const int nsub8 = geo.lpc >> 3, s8 = sub >> 3;
    const bool first = pl.n == 0;
    for (int path = s8; __any(pl.active && path < npaths); path += nsub8) {
        const bool act = pl.active && path < npaths;
        const Leaf L = pairwise_leaf(D, H, act ? path : 0);
        const int T = (L.len >= 8) ? (L.len >> 3) : 0;
        const int rem = (L.len >= 8) ? (L.len & 7) : L.len;
        const int e0 = L.off + j;                      // the lane's element t is e0 + 8 t, its tail e0 + 8 T
        const bool tl = act && j < rem;
        double rv[NUTS_LEAF_T + 1];
#pragma unroll
        for (int t = 0; t < NUTS_LEAF_T; ++t) rv[t] = (act && t < T) ? rr[e0 + 8 * t] : 0.0;
        rv[NUTS_LEAF_T] = tl ? rr[e0 + 8 * T] : 0.0;
        // rho_sub after this leaf, element by element (rho_sub itself is read where a dot needs it)
        auto rs = [&](int t, int e) { return first ? rv[t] : rsub[e] + rv[t]; };
        double *out = S + base + path;
        const bool wr = act && j == 0;
        {   // dot 0: r . r
            double s0 = 0.0;
#pragma unroll
            for (int t = 0; t < NUTS_LEAF_T; ++t)
                if (act && t < T) { const double v = rv[t] * rv[t]; s0 = (t == 0) ? v : s0 + v; }
            const double res = nuts_leaf_end(s0, tl ? rv[NUTS_LEAF_T] * rv[NUTS_LEAF_T] : 0.0, T, rem, lane);
            if (wr) out[0] = res;
        }
        for (int lv = 0; __any(act && lv < pl.nchk); ++lv) {
            const bool la = act && lv < pl.nchk;
            const int64_t off = la ? (c * a.max_depth + (pl.hi - lv)) * a.D : row;
            const double *ckr = a.ck_r + off, *ckrho = a.ck_rho + off;
            double s1 = 0.0, s2 = 0.0, t1 = 0.0, t2 = 0.0;
#pragma unroll
            for (int t = 0; t < NUTS_LEAF_T; ++t)
                if (la && t < T) {
                    const double cv = ckr[e0 + 8 * t];
                    const double sb = (rs(t, e0 + 8 * t) - ckrho[e0 + 8 * t]) + cv;
                    const double v1 = cv * sb, v2 = rv[t] * sb;
                    s1 = (t == 0) ? v1 : s1 + v1;
                    s2 = (t == 0) ? v2 : s2 + v2;
                }
            if (la && tl) {
                const double cv = ckr[e0 + 8 * T];
                const double sb = (rs(NUTS_LEAF_T, e0 + 8 * T) - ckrho[e0 + 8 * T]) + cv;
                t1 = cv * sb; t2 = rv[NUTS_LEAF_T] * sb;
            }
            const double r1 = nuts_leaf_end(s1, t1, T, rem, lane);
            const double r2 = nuts_leaf_end(s2, t2, T, rem, lane);
            if (la && j == 0) { out[(1 + 2 * lv) << H] = r1; out[(2 + 2 * lv) << H] = r2; }
        }
        if (__any(act && pl.merge)) {
            const bool ma = act && pl.merge;
            // the edge in the direction of growth is the leaf itself; the far one is stored
            const double *far = a.edge_r + (pl.v > 0 ? (int64_t)0 : a.C * a.D) + row;
            double s1 = 0.0, s2 = 0.0, t1 = 0.0, t2 = 0.0;
#pragma unroll
            for (int t = 0; t < NUTS_LEAF_T; ++t)
                if (ma && t < T) {
                    const double rt = rtree[e0 + 8 * t] + rs(t, e0 + 8 * t);
                    const double fe = far[e0 + 8 * t];
                    const double v1 = (pl.v > 0 ? fe : rv[t]) * rt, v2 = (pl.v > 0 ? rv[t] : fe) * rt;
                    s1 = (t == 0) ? v1 : s1 + v1;
                    s2 = (t == 0) ? v2 : s2 + v2;
                }
            if (ma && tl) {
                const double rt = rtree[e0 + 8 * T] + rs(NUTS_LEAF_T, e0 + 8 * T);
                const double fe = far[e0 + 8 * T];
                t1 = (pl.v > 0 ? fe : rv[NUTS_LEAF_T]) * rt; t2 = (pl.v > 0 ? rv[NUTS_LEAF_T] : fe) * rt;
            }
            const double r1 = nuts_leaf_end(s1, t1, T, rem, lane);
            const double r2 = nuts_leaf_end(s2, t2, T, rem, lane);
            const int kd = 1 + 2 * pl.nchk;
            if (ma && j == 0) { out[kd << H] = r1; out[(kd + 1) << H] = r2; }
        }
    }
    __syncthreads();
    if (pl.active) {
        for (int k = sub; k < pl.ndots; k += geo.lpc) {
            double *T_ = S + base + (k << H);
            for (int l = 0; l < H; ++l)
                for (int p = 0; p < npaths; p += (2 << l))
                    if (dep[p] >= H - l) T_[p] = T_[p] + T_[p + (1 << l)];
        }
    }
    __syncthreads();
}

template <int VEC>
__global__ void __launch_bounds__(256) nuts_begin_kernel(const binf_nuts_args a, const NutsGeom geo)
{
    extern __shared__ double S[];
    const int lpc = geo.lpc, cpb = 256 / lpc;
    int *dep = reinterpret_cast<int *>(S + ((cpb * geo.ndots) << geo.H));
    const int sub = threadIdx.x & (lpc - 1), cl = threadIdx.x / lpc;
    const int64_t c = (int64_t)blockIdx.x * cpb + cl;
    NutsPlan pl;
    pl.active = c < a.C; pl.n = 0; pl.j = 0; pl.v = 1; pl.hi = 0; pl.nchk = 0; pl.ndots = 1; pl.merge = false;
    const int base = (cl * geo.ndots) << geo.H;
    nuts_dots(a, geo, pl, c, sub, S, dep, base);
    if (!pl.active) return;
    const double K = 0.5 * (0.0 + S[base]);
    const int md = a.max_depth;
    const int64_t nu = 2 * (int64_t)md + ((int64_t)1 << md) - 1;
    const int v = a.u[c * nu] < 0.5 ? 1 : -1;
    const int64_t row = c * a.D, CD = a.C * a.D;
    for (int64_t i = (int64_t)sub * VEC; i < a.D; i += (int64_t)lpc * VEC) {
        double x[VEC];
        nuts_ld<VEC>(x, a.q + row, i);
        nuts_st<VEC>(a.edge_q + row, i, x);
        nuts_st<VEC>(a.edge_q + CD + row, i, x);
        nuts_st<VEC>(a.prop + row, i, x);
        nuts_ld<VEC>(x, a.r + row, i);
        nuts_st<VEC>(a.edge_r + row, i, x);
        nuts_st<VEC>(a.edge_r + CD + row, i, x);
        nuts_st<VEC>(a.rho_tree + row, i, x);
        nuts_ld<VEC>(x, a.g + row, i);
        nuts_st<VEC>(a.edge_g + row, i, x);
        nuts_st<VEC>(a.edge_g + CD + row, i, x);
    }
    if (sub == 0) {
        const double H = K - a.logp[c];
        a.H0[c] = H; a.href[c] = H; a.w_tree[c] = 1.0; a.w_sub[c] = 0.0; a.acc[c] = 0.0;
        a.accept_stat[c] = 0.0;
        a.j[c] = 0; a.n_sub[c] = 0; a.n_leap[c] = 0; a.v[c] = v; a.status[c] = BINF_NUTS_RUN;
        a.tree_depth[c] = 0; a.moved[c] = 0; a.diverging[c] = 0;
        a.dt_dir[c] = (double)v * a.eps[c];
    }
}

template <int VEC>
__global__ void __launch_bounds__(256) nuts_leaf_kernel(const binf_nuts_args a, const NutsGeom geo)
{
    extern __shared__ double S[];
    const int lpc = geo.lpc, cpb = 256 / lpc;
    int *dep = reinterpret_cast<int *>(S + ((cpb * geo.ndots) << geo.H));
    const int sub = threadIdx.x & (lpc - 1), cl = threadIdx.x / lpc;
    const int64_t c = (int64_t)blockIdx.x * cpb + cl;
    const int md = a.max_depth;
    NutsPlan pl;
    pl.active = c < a.C && a.status[c] == BINF_NUTS_RUN;
    pl.n = 0; pl.j = 0; pl.v = 1; pl.hi = 0; pl.nchk = 0; pl.ndots = 0; pl.merge = false;
    if (pl.active) {
        pl.n = a.n_sub[c]; pl.j = a.j[c]; pl.v = a.v[c];
        pl.hi = __popc((unsigned)pl.n >> 1);
        pl.nchk = (pl.n & 1) ? __ffs(~pl.n) - 1 : 0;           // trailing ones of n
        pl.merge = pl.n + 1 == (1 << pl.j);
        pl.ndots = 1 + 2 * pl.nchk + (pl.merge ? 2 : 0);
    }
    // Every per-chain scalar that lane 0 of the chain rewrites at the end of the kernel is read
    // HERE, before the barriers of nuts_dots: a chain of 128 or 256 lanes spans several waves,
    // and those barriers are what orders every wave's reads before lane 0's stores.  Nothing
    // the kernel writes is read again after them except by the lane that wrote it.
    int n_leap = 0;
    double logp = 0.0, H0 = 0.0, acc = 0.0, href = 0.0, w_sub = 0.0, w_tree = 0.0;
    if (pl.active) {
        n_leap = a.n_leap[c] + 1;
        logp = a.logp[c]; H0 = a.H0[c];
        acc = a.acc[c]; href = a.href[c]; w_sub = a.w_sub[c]; w_tree = a.w_tree[c];
    }
    const int base = (cl * geo.ndots) << geo.H;
    nuts_dots(a, geo, pl, c, sub, S, dep, base);
    if (!pl.active) return;
    const int H_ = geo.H;
    auto dot = [&](int k) { return 0.0 + S[base + (k << H_)]; };

    // ---- the chain's branch: every lane, the same scalars, the same bits ----------------
    const int64_t nu = 2 * (int64_t)md + ((int64_t)1 << md) - 1;
    const double *u = a.u + c * nu;
    const int n = pl.n, v = pl.v;
    const double H = 0.5 * dot(0) - logp;
    const double delta = H - H0;
    int j = pl.j, status = BINF_NUTS_RUN, vnew = v, n_sub = n + 1;
    bool sel_cand = false, sel_prop = false, merged = false;
    const bool div = !(delta <= a.max_delta);
    if (div) {
        status = BINF_NUTS_DIV;
    } else {
        const double ea = nuts_expc(-delta);
        acc = acc + (ea < 1.0 ? ea : 1.0);
        double wl;
        if (H < href) {
            const double s = nuts_expc(H - href);
            w_sub = w_sub * s; w_tree = w_tree * s; href = H; wl = 1.0;
        } else {
            wl = nuts_expc(href - H);
        }
        w_sub = w_sub + wl;
        sel_cand = u[2 * md + n_leap - 1] * w_sub < wl;
        bool turn = false;
        for (int t = 0; t < pl.nchk; ++t)
            turn = turn || dot(1 + 2 * t) <= 0.0 || dot(2 + 2 * t) <= 0.0;
        if (turn) {
            status = BINF_NUTS_SUBTURN;
        } else if (pl.merge) {
            merged = true;
            sel_prop = u[md + j] * w_tree < w_sub;
            w_tree = w_tree + w_sub;
            j += 1;
            const int kd = 1 + 2 * pl.nchk;
            if (dot(kd) <= 0.0 || dot(kd + 1) <= 0.0) status = BINF_NUTS_TURN;
            else if (j == md) status = BINF_NUTS_MAXD;
            else { vnew = u[j] < 0.5 ? 1 : -1; w_sub = 0.0; n_sub = 0; }
        }
    }
    const bool finish = status != BINF_NUTS_RUN;

    // ---- one pass over the row ------------------------------------------------------------
    const int64_t row = c * a.D, CD = a.C * a.D;
    const int64_t ck = (c * md + pl.hi) * a.D;
    const int64_t e_own = (v > 0 ? CD : 0) + row, e_new = (vnew > 0 ? CD : 0) + row;
    const bool even = (n & 1) == 0, first = n == 0;
    for (int64_t i = (int64_t)sub * VEC; i < a.D; i += (int64_t)lpc * VEC) {
        double pv[VEC];
        if (div) {
            nuts_ld<VEC>(pv, a.prop + row, i);
            nuts_st<VEC>(a.q_out + row, i, pv);
            continue;
        }
        double qv[VEC], rv[VEC], rs[VEC], cv[VEC];
        nuts_ld<VEC>(qv, a.q + row, i);
        nuts_ld<VEC>(rv, a.r + row, i);
        if (first) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) rs[e] = rv[e];
        } else {
            nuts_ld<VEC>(rs, a.rho_sub + row, i);
#pragma unroll
            for (int e = 0; e < VEC; ++e) rs[e] = rs[e] + rv[e];
        }
        nuts_st<VEC>(a.rho_sub + row, i, rs);
        if (sel_cand) nuts_st<VEC>(a.cand + row, i, qv);
        if (even) {
            nuts_st<VEC>(a.ck_r + ck, i, rv);
            nuts_st<VEC>(a.ck_rho + ck, i, rs);
        }
        if (status == BINF_NUTS_SUBTURN) {
            nuts_ld<VEC>(pv, a.prop + row, i);
            nuts_st<VEC>(a.q_out + row, i, pv);
        } else if (merged) {
            if (sel_prop) {
                if (sel_cand) {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) pv[e] = qv[e];
                } else {
                    nuts_ld<VEC>(pv, a.cand + row, i);
                }
                nuts_st<VEC>(a.prop + row, i, pv);
            } else if (finish) {
                nuts_ld<VEC>(pv, a.prop + row, i);
            }
            nuts_ld<VEC>(cv, a.rho_tree + row, i);
#pragma unroll
            for (int e = 0; e < VEC; ++e) cv[e] = cv[e] + rs[e];
            nuts_st<VEC>(a.rho_tree + row, i, cv);
            nuts_ld<VEC>(cv, a.g + row, i);
            nuts_st<VEC>(a.edge_q + e_own, i, qv);
            nuts_st<VEC>(a.edge_r + e_own, i, rv);
            nuts_st<VEC>(a.edge_g + e_own, i, cv);
            if (finish) {
                nuts_st<VEC>(a.q_out + row, i, pv);
            } else if (vnew != v) {
                nuts_ld<VEC>(cv, a.edge_q + e_new, i);
                nuts_st<VEC>(a.q + row, i, cv);
                nuts_ld<VEC>(cv, a.edge_r + e_new, i);
                nuts_st<VEC>(a.r + row, i, cv);
                nuts_ld<VEC>(cv, a.edge_g + e_new, i);
                nuts_st<VEC>(a.g + row, i, cv);
            }
        }
    }
    if (sub == 0) {
        a.n_leap[c] = n_leap;
        a.status[c] = status;
        if (!div) {
            a.acc[c] = acc; a.href[c] = href; a.w_sub[c] = w_sub; a.w_tree[c] = w_tree;
            a.n_sub[c] = n_sub; a.j[c] = j; a.v[c] = vnew;
            if (sel_prop) a.moved[c] = 1;
        }
        if (finish) {
            const bool mv = sel_prop || a.moved[c] != 0;
            a.tree_depth[c] = j;
            a.accept_stat[c] = acc / (double)n_leap;
            a.dt_dir[c] = 0.0;
            a.diverging[c] = div ? 1 : 0;
            if (div) a.n_divergent[c] += 1;
            if (mv) a.n_accepted[c] += 1;
        } else {
            a.dt_dir[c] = (double)vnew * a.eps[c];
        }
    }
}

// chains still growing: one workgroup, every thread its strided share, an LDS tree
__global__ void __launch_bounds__(256) nuts_pending_kernel(const int32_t *status, int64_t C, int64_t *count)
{
    __shared__ long long part[256];
    long long mine = 0;
    for (int64_t i = threadIdx.x; i < C; i += 256) mine += status[i] == BINF_NUTS_RUN ? 1 : 0;
    part[threadIdx.x] = mine;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) count[0] = part[0];
}

struct AdaptArgs {
    double *eps;
    const double *accept_stat;
    double *hbar, *logeps, *logeps_bar, *mu;
    double target, w1, k1, eta;
    int64_t C;
    int32_t action;
};

// ACTION is a template parameter: one straight-line kernel per action, no switch on a kernel
// argument around the stores
template <int ACTION>
__global__ void __launch_bounds__(256) nuts_adapt_kernel(const AdaptArgs a)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= a.C) return;
    if (ACTION == 0) {
        const double hbar = (1.0 - a.w1) * a.hbar[c] + a.w1 * (a.target - a.accept_stat[c]);
        const double le = a.mu[c] - a.k1 * hbar;
        const double bar = a.eta * le + (1.0 - a.eta) * a.logeps_bar[c];
        const double e = exp(le);
        a.hbar[c] = hbar;
        a.logeps[c] = le;
        a.logeps_bar[c] = bar;
        a.eps[c] = e;
    } else if (ACTION == 1) {
        const double m = log(10.0 * a.eps[c]);
        a.mu[c] = m;
        a.hbar[c] = 0.0;
        a.logeps_bar[c] = 0.0;
    } else {
        const double e = exp(a.logeps_bar[c]);
        a.eps[c] = e;
    }
}

struct NutsSpan { const void *p; int64_t bytes; const char *name; };

static int32_t nuts_check(const binf_nuts_args *a, const char *what)
{
    if (!a) return fail(BINF_E_ARG, "%s: null argument block", what);
    if (a->struct_size != sizeof(binf_nuts_args))
        return fail(BINF_E_ARG, "%s: struct_size %llu, expected %llu", what,
                    (unsigned long long)a->struct_size, (unsigned long long)sizeof(binf_nuts_args));
    if (a->C < 0 || a->D < 1) return fail(BINF_E_ARG, "%s: C >= 0 and D >= 1 required", what);
    if (a->max_depth < 1 || a->max_depth > BINF_NUTS_MAX_DEPTH)
        return fail(BINF_E_ARG, "%s: max_depth %d outside 1 ... %d", what, a->max_depth, BINF_NUTS_MAX_DEPTH);
    if (a->D > NPY_BUFSIZE)
        return fail(BINF_E_UNSUPPORTED, "%s: rows beyond %d elements", what, NPY_BUFSIZE);
    if (a->C > 0x7fffffffLL) return fail(BINF_E_UNSUPPORTED, "%s: too many chains", what);
    const int64_t C = a->C, CD = a->C * a->D, md = a->max_depth;
    const int64_t S = 2 * md + ((int64_t)1 << md) - 1;
    const NutsSpan sp[] = {
        {a->q, CD * 8, "q"}, {a->r, CD * 8, "r"}, {a->g, CD * 8, "g"},
        {a->edge_q, 2 * CD * 8, "edge_q"}, {a->edge_r, 2 * CD * 8, "edge_r"}, {a->edge_g, 2 * CD * 8, "edge_g"},
        {a->cand, CD * 8, "cand"}, {a->prop, CD * 8, "prop"}, {a->q_out, CD * 8, "q_out"},
        {a->rho_sub, CD * 8, "rho_sub"}, {a->rho_tree, CD * 8, "rho_tree"},
        {a->ck_r, CD * md * 8, "ck_r"}, {a->ck_rho, CD * md * 8, "ck_rho"},
        {a->logp, C * 8, "logp"}, {a->eps, C * 8, "eps"}, {a->dt_dir, C * 8, "dt_dir"}, {a->H0, C * 8, "H0"},
        {a->href, C * 8, "href"}, {a->w_sub, C * 8, "w_sub"}, {a->w_tree, C * 8, "w_tree"}, {a->acc, C * 8, "acc"},
        {a->accept_stat, C * 8, "accept_stat"}, {a->u, C * S * 8, "u"},
        {a->j, C * 4, "j"}, {a->n_sub, C * 4, "n_sub"}, {a->n_leap, C * 4, "n_leap"}, {a->v, C * 4, "v"},
        {a->status, C * 4, "status"}, {a->tree_depth, C * 4, "tree_depth"},
        {a->moved, C, "moved"}, {a->diverging, C, "diverging"},
        {a->n_accepted, C * 8, "n_accepted"}, {a->n_divergent, C * 8, "n_divergent"}};
    const int ns = (int)(sizeof(sp) / sizeof(sp[0]));
    if (C == 0) return 0;
    for (int i = 0; i < ns; ++i)
        if (!sp[i].p) return fail(BINF_E_ARG, "%s: null buffer %s", what, sp[i].name);
    for (int i = 0; i < ns; ++i)
        for (int k = i + 1; k < ns; ++k) {
            const char *x = (const char *)sp[i].p, *y = (const char *)sp[k].p;
            if (x < y + sp[k].bytes && y < x + sp[i].bytes)
                return fail(BINF_E_ALIAS, "%s: %s overlaps %s", what, sp[i].name, sp[k].name);
        }
    return 0;
}

static bool nuts_vec2(const binf_nuts_args *a)
{
    const uintptr_t all = (uintptr_t)a->q | (uintptr_t)a->r | (uintptr_t)a->g | (uintptr_t)a->edge_q |
        (uintptr_t)a->edge_r | (uintptr_t)a->edge_g | (uintptr_t)a->cand | (uintptr_t)a->prop |
        (uintptr_t)a->q_out | (uintptr_t)a->rho_sub | (uintptr_t)a->rho_tree | (uintptr_t)a->ck_r |
        (uintptr_t)a->ck_rho;
    return a->D % 2 == 0 && (all & 15) == 0;
}

static int32_t nuts_launch(const binf_nuts_args *a, void *stream, bool leaf, const char *what)
{
    const int32_t rc = nuts_check(a, what);
    if (rc) return rc;
    if (a->C == 0) return 0;
    const bool vec2 = nuts_vec2(a);
    NutsGeom geo;
    int lpc = 8;
    while (lpc < 256 && (int64_t)lpc * (vec2 ? 2 : 1) < a->D) lpc <<= 1;
    geo.lpc = lpc;
    geo.H = pairwise_tree_height(a->D);          // at most 7 for D <= NPY_BUFSIZE: 128 leaf sums, dep[128]
    geo.ndots = leaf ? 2 * a->max_depth + 3 : 1;
    const int cpb = 256 / lpc;
    const size_t lds = ((size_t)(cpb * geo.ndots) << geo.H) * sizeof(double) + 128 * sizeof(int);
    const int64_t blocks = (a->C + cpb - 1) / cpb;
    const dim3 grid((unsigned)blocks);
    hipStream_t st = (hipStream_t)stream;
    if (leaf) {
        if (vec2) nuts_leaf_kernel<2><<<grid, 256, lds, st>>>(*a, geo);
        else      nuts_leaf_kernel<1><<<grid, 256, lds, st>>>(*a, geo);
    } else {
        if (vec2) nuts_begin_kernel<2><<<grid, 256, lds, st>>>(*a, geo);
        else      nuts_begin_kernel<1><<<grid, 256, lds, st>>>(*a, geo);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what);
    return 0;
}

}  // namespace binf

using namespace binf;

extern "C" int32_t binf_nuts_begin_f64(const binf_nuts_args *args, void *stream)
{
    return nuts_launch(args, stream, false, "nuts_begin");
}

extern "C" int32_t binf_nuts_leaf_f64(const binf_nuts_args *args, void *stream)
{
    return nuts_launch(args, stream, true, "nuts_leaf");
}

extern "C" int32_t binf_nuts_pending(const int32_t *status, int64_t C, int64_t *count, void *stream)
{
    if (C < 0) return fail(BINF_E_ARG, "nuts_pending: negative size");
    if (!count || (!status && C > 0)) return fail(BINF_E_ARG, "nuts_pending: null buffer");
    nuts_pending_kernel<<<dim3(1), 256, 0, (hipStream_t)stream>>>(status, C, count);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "nuts_pending");
    return 0;
}

extern "C" int32_t binf_nuts_adapt_step_f64(double *eps, const double *accept_stat, double *hbar,
                                            double *logeps, double *logeps_bar, double *mu,
                                            double target, double w1, double k1, double eta,
                                            int32_t action, int64_t C, void *stream)
{
    if (C < 0) return fail(BINF_E_ARG, "nuts_adapt_step: negative size");
    if (action < 0 || action > 2) return fail(BINF_E_ARG, "nuts_adapt_step: unknown action %d", action);
    if (C == 0) return 0;
    if (!eps || !hbar || !logeps || !logeps_bar || !mu || (action == 0 && !accept_stat))
        return fail(BINF_E_ARG, "nuts_adapt_step: null buffer");
    if (C > 0x7fffffffLL * 256) return fail(BINF_E_UNSUPPORTED, "nuts_adapt_step: too many chains");
    AdaptArgs a;
    a.eps = eps; a.accept_stat = accept_stat; a.hbar = hbar; a.logeps = logeps; a.logeps_bar = logeps_bar;
    a.mu = mu; a.target = target; a.w1 = w1; a.k1 = k1; a.eta = eta; a.C = C; a.action = action;
    const dim3 grid((unsigned)((C + 255) / 256));
    hipStream_t st = (hipStream_t)stream;
    if (action == 0)      nuts_adapt_kernel<0><<<grid, 256, 0, st>>>(a);
    else if (action == 1) nuts_adapt_kernel<1><<<grid, 256, 0, st>>>(a);
    else                  nuts_adapt_kernel<2><<<grid, 256, 0, st>>>(a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "nuts_adapt_step");
    return 0;
}
