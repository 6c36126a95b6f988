// Free-energy differences between neighbouring slots of a tempered ladder: the work
// record of a swap round and Bennett's acceptance ratio (BAR) over a record of rounds.
// Build-defined: the reference has the hook a replica exchange scheme drives
// (binf/samplers/hmc.py:171-176 last_draw_stats) and no estimator of its own.
//
// WORK RECORD.  A swap round evaluates lp_own[c] = log p_c(x_c) and lp_sw[c] =
// log p_c(x_partner(c)) (replica.hip).  binf_replica_work_f64 writes one [C] row
//     w[c] = lp_sw[c] - lp_own[partner(c)]        paired chains (one subtraction)
//     w[c] = quiet NaN                            unpaired chains
// so for the pair (r, r + 1) of a ladder, with i the chain of slot r,
//     u = w[i]     = log p_r(x) - log p_{r+1}(x)   at x ~ p_{r+1}
//     v = w[i + 1] = log p_{r+1}(y) - log p_r(y)   at y ~ p_r.
// Pair (r, r + 1) is active exactly in the rounds whose parity is r & 1: row t of a record
// whose row 0 is round `first_round` holds it iff ((first_round + t) & 1) == (r & 1).
//
// ESTIMATOR.  One independent problem per (group g of ladders, pair r): n samples u and n
// samples v, sample s = k * Lg + l being row t0 + 2 k, ladder g * Lg + l (Lg ladders per
// group).  Samples are cut into chunks of BINF_FE_CHUNK counted from the start of the
// problem; a 256-thread workgroup per chunk reduces it (thread j takes samples j, j + 256,
// ... in order; the wave's butterfly of common.hpp, a balanced tree over neighbouring
// lanes; the four waves in order through LDS) and stores the partials in a slab; a
// finishing kernel adds a problem's chunks in ascending order and moves the problem's
// root bracket.  Plain stores and launch boundaries only: the outputs are a pure function
// of the samples, whatever the grid, the row stride, G or the group's place in the batch.
//
//   pass 1   per chunk and direction: max m, sum exp(x - m), min over finite, #invalid
//   finish 1 M = max m, total = sum_chunks S_c exp(m_c - M):
//            delta_fwd = (M_u + log total_u) - log n, delta_rev = -((M_v + log total_v) - log n),
//            bracket lo = min(min u, -max v), hi = max(max u, -min v), first iterate
//            (delta_fwd + delta_rev) / 2 if inside the bracket, else its midpoint
//   iterate  per chunk: sum sigma(u - D), sum sigma(v + D), sum sigma (1 - sigma) of both
//   finish   g = sum_v - sum_u (increasing in D), S = sum sigma (1 - sigma) = g':
//            g < 0 moves lo to D, g > 0 moves hi; the Newton step D - g / S is taken if it
//            lies strictly inside the bracket and is at most half the previous step, else
//            the bracket is bisected; the problem closes when g == 0 or D stops changing.
//            A run of Newton steps halves the step each time and a run of bisections
//            the bracket, but a bisection resets the "step before" to half the bracket,
//            so the two can interleave: what GUARANTEES the end is the cap FE_MAX_ITER
//            (status NOT_CONVERGED), far above the handful of passes real data take.
//            A problem that closes with S == 0 (every sigma under- or overflowed: g is
//            flat 0 around the iterate) has no determined root: status NO_OVERLAP.
// The logistic, fixed: t = exp(-|z|); sigma = z >= 0 ? 1 / (1 + t) : t / (1 + t);
// sigma (1 - sigma) = t / ((1 + t) (1 + t)).  -inf is a sample of weight 0 (sigma = 0,
// outside the bracket); +inf / NaN in a paired position are counted and void the problem.
// FP64 throughout, exp / log of the device library (within 1 ulp).  gfx950, wave64.
#include "replica_pairing.hpp"

#include <math.h>

namespace binf {

constexpr int FE_CHUNK = BINF_FE_CHUNK;
constexpr int FE_THREADS = 256;
constexpr int FE_PER = FE_CHUNK / FE_THREADS;
constexpr int FE_MAX_ITER = 2200;       // the halvings of ONE run across a double's range
static_assert(FE_CHUNK % FE_THREADS == 0, "chunk = whole strides of the workgroup");

// ---- work record -------------------------------------------------------------------
__global__ void __launch_bounds__(256)
replica_work_kernel(const double *lp_own, const double *lp_sw, double *w, int64_t C, int64_t R,
                    int32_t parity)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const int64_t i = replica_pair_lower(c, R, parity);
    double v = __longlong_as_double(0x7ff8000000000000LL);
    if (i >= 0) v = lp_sw[c] - lp_own[i == c ? c + 1 : i];
    w[c] = v;
}

// ---- estimator ---------------------------------------------------------------------
struct FeGeom {
    const double *w;
    int64_t stride_t;
    int64_t T, C, R, first_round;
    int64_t Lg;             // ladders per group
    int64_t maxch;          // chunks of the largest problem (slab rows per problem)
    double *state;          // [P][4]: delta, lo, hi, previous step
    double *slab1;          // [P][maxch][8]
    double *slab2;          // [P][maxch][3]
    int32_t *open;          // [P]
    int32_t *iters;         // [P]
    int32_t *any_open;      // [1]
    double *delta, *delta_fwd, *delta_rev, *info;
    int64_t *n, *n_invalid;
    int32_t *status;
};

struct FeProblem {
    int64_t g, r, t0, n, nch;
};

__device__ inline FeProblem fe_problem(const FeGeom &a, int64_t p)
{
    FeProblem q;
    q.g = p / (a.R - 1);
    q.r = p % (a.R - 1);
    q.t0 = ((q.r & 1) - (a.first_round & 1)) & 1;
    const int64_t rows = a.T > q.t0 ? (a.T - q.t0 + 1) / 2 : 0;
    q.n = rows * a.Lg;
    q.nch = (q.n + FE_CHUNK - 1) / FE_CHUNK;
    return q;
}

// the chunk's samples of this thread, in its order; positions past the problem's end read
// as -inf, the sample of weight 0
__device__ inline void fe_load(const FeGeom &a, const FeProblem &q, int64_t chunk,
                               double (&u)[FE_PER], double (&v)[FE_PER])
{
    const double ninf = -INFINITY;
    int64_t s = chunk * FE_CHUNK + threadIdx.x;
    int64_t k = s / a.Lg, l = s % a.Lg;
    const int64_t dk = FE_THREADS / a.Lg, dl = FE_THREADS % a.Lg;
    const double *base = a.w + q.t0 * a.stride_t + q.g * a.Lg * a.R + q.r;
#pragma unroll
    for (int i = 0; i < FE_PER; ++i) {
        u[i] = ninf;
        v[i] = ninf;
        if (s < q.n) {
            const double *ptr = base + 2 * k * a.stride_t + l * a.R;
            u[i] = ptr[0];
            v[i] = ptr[1];
        }
        s += FE_THREADS;
        k += dk;
        l += dl;
        if (l >= a.Lg) { l -= a.Lg; k += 1; }
    }
}

struct OpSum { __device__ static double op(double x, double y) { return x + y; } };
struct OpMax { __device__ static double op(double x, double y) { return fmax(x, y); } };
struct OpMin { __device__ static double op(double x, double y) { return fmin(x, y); } };

// all lanes: the balanced tree over neighbouring lanes (2, 4, 8, 16, 32, 64)
template <class OP>
__device__ inline double fe_wave(double r, int lane)
{
    r = OP::op(r, xor1_f64(r));
    r = OP::op(r, xor2_f64(r));
    r = OP::op(r, other_quad_f64(r));
#pragma unroll
    for (int l = 0; l < 3; ++l) r = OP::op(r, xor_level_f64(r, l, lane));
    return r;
}

// all threads: ((w0 . w1) . w2) . w3 over the four waves' trees
template <class OP>
__device__ inline double fe_block(double r, double *sh)
{
    const int lane = threadIdx.x & 63;
    r = fe_wave<OP>(r, lane);
    __syncthreads();
    if (lane == 0) sh[threadIdx.x >> 6] = r;
    __syncthreads();
    return OP::op(OP::op(OP::op(sh[0], sh[1]), sh[2]), sh[3]);
}

__device__ inline bool fe_invalid(double x) { return !(x <= 1.7976931348623157e308); }

__global__ void __launch_bounds__(FE_THREADS) fe_pass1_kernel(const FeGeom a)
{
    __shared__ double sh[4];
    const int64_t p = blockIdx.x / a.maxch, chunk = blockIdx.x % a.maxch;
    const FeProblem q = fe_problem(a, p);
    if (chunk >= q.nch) return;
    double x[2][FE_PER];
    fe_load(a, q, chunk, x[0], x[1]);
    double *out = a.slab1 + (p * a.maxch + chunk) * 8;
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        double mx = -INFINITY, mn = INFINITY, bad = 0.0;
#pragma unroll
        for (int i = 0; i < FE_PER; ++i) {
            double e = x[d][i];
            if (fe_invalid(e)) { bad = bad + 1.0; e = -INFINITY; }
            x[d][i] = e;
            mx = fmax(mx, e);
            if (e > -INFINITY) mn = fmin(mn, e);
        }
        mx = fe_block<OpMax>(mx, sh);
        mn = fe_block<OpMin>(mn, sh);
        bad = fe_block<OpSum>(bad, sh);
        double acc = 0.0;
        if (mx > -INFINITY) {
#pragma unroll
            for (int i = 0; i < FE_PER; ++i) acc = acc + exp(x[d][i] - mx);
        }
        acc = fe_block<OpSum>(acc, sh);
        if (threadIdx.x == 0) {
            out[4 * d + 0] = mx;
            out[4 * d + 1] = acc;
            out[4 * d + 2] = mn;
            out[4 * d + 3] = bad;
        }
    }
}

__device__ inline void fe_logistic(double z, double &sig, double &dsig)
{
    const double t = exp(-fabs(z));
    const double d = 1.0 + t;
    sig = z >= 0.0 ? 1.0 / d : t / d;
    dsig = t / (d * d);
}

__global__ void __launch_bounds__(FE_THREADS) fe_iter_kernel(const FeGeom a)
{
    __shared__ double sh[4];
    const int64_t p = blockIdx.x / a.maxch, chunk = blockIdx.x % a.maxch;
    if (!a.open[p]) return;
    const FeProblem q = fe_problem(a, p);
    if (chunk >= q.nch) return;
    const double D = a.state[p * 4];
    double u[FE_PER], v[FE_PER];
    fe_load(a, q, chunk, u, v);
    double su = 0.0, sv = 0.0, sd = 0.0;
#pragma unroll
    for (int i = 0; i < FE_PER; ++i) {
        double s0, d0, s1, d1;
        fe_logistic(u[i] - D, s0, d0);
        fe_logistic(v[i] + D, s1, d1);
        su = su + s0;
        sv = sv + s1;
        sd = (sd + d0) + d1;
    }
    su = fe_block<OpSum>(su, sh);
    sv = fe_block<OpSum>(sv, sh);
    sd = fe_block<OpSum>(sd, sh);
    if (threadIdx.x == 0) {
        double *out = a.slab2 + (p * a.maxch + chunk) * 3;
        out[0] = su;
        out[1] = sv;
        out[2] = sd;
    }
}

// Finishing kernels: a 64-thread workgroup per problem stages 64 chunks' partials at a
// time in LDS; thread 0 walks them in ascending order.
template <int K, class F>
__device__ inline void fe_walk(const double *slab, int64_t nch, double (*sh)[64], const F &f)
{
    for (int64_t c0 = 0; c0 < nch; c0 += 64) {
        const int64_t c = c0 + threadIdx.x;
        __syncthreads();
        if (c < nch) {
#pragma unroll
            for (int k = 0; k < K; ++k) sh[k][threadIdx.x] = slab[c * K + k];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int m = nch - c0 < 64 ? (int)(nch - c0) : 64;
            for (int j = 0; j < m; ++j) f(j);
        }
    }
}

__device__ inline void fe_close(const FeGeom &a, int64_t p, double delta, double info,
                                int32_t status)
{
    a.delta[p] = delta;
    a.info[p] = info;
    a.status[p] = status;
    a.open[p] = 0;
}

__global__ void __launch_bounds__(64) fe_finish1_kernel(const FeGeom a)
{
    __shared__ double sh[8][64];
    const int64_t p = blockIdx.x;
    const FeProblem q = fe_problem(a, p);
    const double *slab = a.slab1 + p * a.maxch * 8;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    double M[2] = {-INFINITY, -INFINITY}, mn[2] = {INFINITY, INFINITY}, bad[2] = {0.0, 0.0};
    fe_walk<8>(slab, q.nch, sh, [&](int j) {
        for (int d = 0; d < 2; ++d) {
            M[d] = fmax(M[d], sh[4 * d][j]);
            mn[d] = fmin(mn[d], sh[4 * d + 2][j]);
            bad[d] = bad[d] + sh[4 * d + 3][j];
        }
    });
    double tot[2] = {0.0, 0.0};
    fe_walk<8>(slab, q.nch, sh, [&](int j) {
        for (int d = 0; d < 2; ++d) {
            const double m = sh[4 * d][j];
            if (m > -INFINITY) tot[d] = tot[d] + sh[4 * d + 1][j] * exp(m - M[d]);
        }
    });
    if (threadIdx.x != 0) return;
    a.iters[p] = 0;
    a.n[p] = q.n;
    a.n_invalid[p] = (int64_t)(bad[0] + bad[1]);
    if (q.n == 0 || bad[0] + bad[1] > 0.0) {
        a.delta_fwd[p] = qnan;
        a.delta_rev[p] = qnan;
        fe_close(a, p, qnan, qnan, q.n == 0 ? BINF_FE_EMPTY : BINF_FE_INVALID);
        return;
    }
    const double logn = log((double)q.n);
    const double fwd = M[0] > -INFINITY ? (M[0] + log(tot[0])) - logn : -INFINITY;
    const double rev = M[1] > -INFINITY ? -((M[1] + log(tot[1])) - logn) : INFINITY;
    a.delta_fwd[p] = fwd;
    a.delta_rev[p] = rev;
    if (!(M[0] > -INFINITY) && !(M[1] > -INFINITY)) { fe_close(a, p, qnan, qnan, BINF_FE_NO_FINITE); return; }
    if (!(M[0] > -INFINITY)) { fe_close(a, p, -INFINITY, 0.0, BINF_FE_ONE_SIDED); return; }
    if (!(M[1] > -INFINITY)) { fe_close(a, p, INFINITY, 0.0, BINF_FE_ONE_SIDED); return; }
    const double lo = fmin(mn[0], -M[1]), hi = fmax(M[0], -mn[1]);
    double D = 0.5 * fwd + 0.5 * rev;
    if (!(D >= lo && D <= hi)) D = 0.5 * lo + 0.5 * hi;
    double *st = a.state + p * 4;
    st[0] = D;
    st[1] = lo;
    st[2] = hi;
    st[3] = hi - lo;
    a.open[p] = 1;
    a.status[p] = BINF_FE_NOT_CONVERGED;       // until the problem closes
    a.delta[p] = D;
    a.info[p] = qnan;
}

__global__ void __launch_bounds__(64) fe_finish_iter_kernel(const FeGeom a)
{
    __shared__ double sh[3][64];
    const int64_t p = blockIdx.x;
    if (!a.open[p]) return;
    const FeProblem q = fe_problem(a, p);
    double A = 0.0, B = 0.0, S = 0.0;
    fe_walk<3>(a.slab2 + p * a.maxch * 3, q.nch, sh, [&](int j) {
        A = A + sh[0][j];
        B = B + sh[1][j];
        S = S + sh[2][j];
    });
    if (threadIdx.x != 0) return;
    double *st = a.state + p * 4;
    const double D = st[0];
    double lo = st[1], hi = st[2];
    const double g = B - A;
    const int32_t it = a.iters[p] + 1;
    a.iters[p] = it;
    const int32_t closed = S > 0.0 ? BINF_FE_OK : BINF_FE_NO_OVERLAP;
    if (g == 0.0) { fe_close(a, p, D, S, closed); return; }
    if (g < 0.0) lo = D; else hi = D;
    const double step = g / S;
    const double cand = D - step;
    double Dn, dx;
    if (cand > lo && cand < hi && fabs(2.0 * g) <= fabs(st[3] * S)) {
        Dn = cand;
        dx = fabs(step);
    } else {
        dx = 0.5 * hi - 0.5 * lo;
        Dn = fmin(lo + dx, hi);
    }
    if (Dn == D) { fe_close(a, p, D, S, closed); return; }
    if (it >= FE_MAX_ITER) { fe_close(a, p, D, S, BINF_FE_NOT_CONVERGED); return; }
    st[0] = Dn;
    st[1] = lo;
    st[2] = hi;
    st[3] = dx;
    a.delta[p] = Dn;
    a.info[p] = S;
    *a.any_open = 1;        // the same value from every open problem: a plain store
}

struct FeLayout {
    int64_t P, maxch, state, slab1, slab2, open, iters, flag, bytes;
};

// false: the shape is refused (G does not divide the ladders, sizes out of range)
static bool fe_layout(int64_t T, int64_t C, int64_t R, int64_t G, FeLayout &L)
{
    if (T < 0 || C < 0 || R < 1 || G < 1 || C % R != 0 || (C / R) % G != 0) return false;
    if (T > 0x7fffffffLL || C > 0x7fffffffLL) return false;
    const int64_t Lg = C / R / G;
    const int64_t n = ((T + 1) / 2) * Lg;           // the larger parity class
    L.P = G * (R - 1);
    L.maxch = (n + FE_CHUNK - 1) / FE_CHUNK;
    if (L.P > 0x7fffffffLL || (L.maxch > 0 && L.P > 0x7fffffffLL / L.maxch)) return false;
    int64_t off = 0;
    L.state = off; off += L.P * 4 * 8;
    L.slab1 = off; off += L.P * L.maxch * 8 * 8;
    L.slab2 = off; off += L.P * L.maxch * 3 * 8;
    L.open = off;  off += (L.P * 4 + 7) / 8 * 8;
    L.iters = off; off += (L.P * 4 + 7) / 8 * 8;
    L.flag = off;  off += 8;
    L.bytes = off;
    return true;
}

}  // namespace binf

using namespace binf;

extern "C" int32_t binf_replica_work_f64(const double *lp_own, const double *lp_swapped,
                                         double *w_out, int64_t C, int64_t R, int32_t parity,
                                         void *stream)
{
    const char *what = "replica_work";
    if (C < 0) return fail(BINF_E_ARG, "%s: negative size", what);
    if (R < 1) return fail(BINF_E_ARG, "%s: R >= 1 required", what);
    if (C % R != 0) return fail(BINF_E_ARG, "%s: C is not a multiple of R", what);
    if (parity != 0 && parity != 1) return fail(BINF_E_ARG, "%s: parity %d outside {0, 1}", what, parity);
    if (C == 0) return 0;
    if (!lp_own || !lp_swapped || !w_out) return fail(BINF_E_ARG, "%s: null buffer", what);
    if (overlap_f64(w_out, C, lp_own, C) || overlap_f64(w_out, C, lp_swapped, C))
        return fail(BINF_E_ALIAS, "%s: w_out overlaps an input (a partner's entry is read "
                    "after its own chain may have been written)", what);
    const int64_t blocks = (C + 255) / 256;
    if (blocks > 0x7fffffffLL) return fail(BINF_E_UNSUPPORTED, "%s: too many chains", what);
    replica_work_kernel<<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(
        lp_own, lp_swapped, w_out, C, R, parity);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what);
    return 0;
}

extern "C" int32_t binf_free_energy_chunk(void) { return FE_CHUNK; }

extern "C" int64_t binf_free_energy_bar_workspace_bytes(int64_t T, int64_t C, int64_t R, int64_t G)
{
    FeLayout L;
    if (!fe_layout(T, C, R, G, L)) return 0;
    return L.bytes;
}

extern "C" int32_t binf_free_energy_bar_f64(const double *work, int64_t stride_t, int64_t T,
                                            int64_t C, int64_t R, int64_t first_round, int64_t G,
                                            double *delta, double *delta_fwd, double *delta_rev,
                                            double *info, int64_t *n, int64_t *n_invalid,
                                            int32_t *status, void *workspace,
                                            int64_t workspace_bytes, void *stream)
{
    const char *what = "free_energy_bar";
    if (T < 0 || C < 0) return fail(BINF_E_ARG, "%s: negative size", what);
    if (R < 1) return fail(BINF_E_ARG, "%s: R >= 1 required", what);
    if (C % R != 0) return fail(BINF_E_ARG, "%s: C is not a multiple of R", what);
    if (G < 1 || (C / R) % G != 0)
        return fail(BINF_E_ARG, "%s: G must be >= 1 and divide the number of ladders", what);
    if (first_round < 0) return fail(BINF_E_ARG, "%s: negative first_round", what);
    if (stride_t < 0 || (T > 1 && stride_t < C))
        return fail(BINF_E_ARG, "%s: rows of %lld overlap at a row stride of %lld", what,
                    (long long)C, (long long)stride_t);
    FeLayout L;
    if (!fe_layout(T, C, R, G, L) || stride_t > (1LL << 40))
        return fail(BINF_E_UNSUPPORTED, "%s: record or batch too large", what);
    if (L.P == 0) return 0;                             // R == 1: nothing to estimate
    if (!delta || !delta_fwd || !delta_rev || !info || !n || !n_invalid || !status)
        return fail(BINF_E_ARG, "%s: null output", what);
    if (!workspace || workspace_bytes < L.bytes || (((uintptr_t)workspace) & 7))
        return fail(BINF_E_ARG, "%s: workspace NULL, misaligned or smaller than %lld bytes", what,
                    (long long)L.bytes);
    if (L.maxch > 0 && !work) return fail(BINF_E_ARG, "%s: null record", what);
    char *ws = (char *)workspace;
    FeGeom a;
    a.w = work; a.stride_t = stride_t; a.T = T; a.C = C; a.R = R; a.first_round = first_round;
    a.Lg = C / R / G; a.maxch = L.maxch;
    a.state = (double *)(ws + L.state); a.slab1 = (double *)(ws + L.slab1);
    a.slab2 = (double *)(ws + L.slab2); a.open = (int32_t *)(ws + L.open);
    a.iters = (int32_t *)(ws + L.iters); a.any_open = (int32_t *)(ws + L.flag);
    a.delta = delta; a.delta_fwd = delta_fwd; a.delta_rev = delta_rev; a.info = info;
    a.n = n; a.n_invalid = n_invalid; a.status = status;
    const hipStream_t st = (hipStream_t)stream;
    const unsigned chunks = (unsigned)(L.P * L.maxch), probs = (unsigned)L.P;
    if (chunks) fe_pass1_kernel<<<dim3(chunks), FE_THREADS, 0, st>>>(a);
    fe_finish1_kernel<<<dim3(probs), 64, 0, st>>>(a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what);
    if (!chunks) return 0;                              // every problem is empty and closed
    // the host drives the iterations and reads one flag back between batches of them
    for (int done = 0, batch = 6; done <= FE_MAX_ITER; done += batch, batch = 4) {
        for (int i = 0; i < batch; ++i) {
            if (i == batch - 1) BINF_HIP_CHECK(hipMemsetAsync(a.any_open, 0, 4, st));
            fe_iter_kernel<<<dim3(chunks), FE_THREADS, 0, st>>>(a);
            fe_finish_iter_kernel<<<dim3(probs), 64, 0, st>>>(a);
        }
        e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, what);
        int32_t any = 0;
        BINF_HIP_CHECK(hipMemcpyAsync(&any, a.any_open, 4, hipMemcpyDeviceToHost, st));
        BINF_HIP_CHECK(hipStreamSynchronize(st));
        if (!any) break;
    }
    return 0;
}
