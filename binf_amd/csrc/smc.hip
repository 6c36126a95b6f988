// Tempered sequential Monte Carlo over populations of chains: the reweighting with its
// root search for the next temperature, systematic resampling, the row gather.
// Build-defined: the reference runs one chain at one temperature (binf/samplers/hmc.py)
// and has no population method of its own.
//
// C = G * P chains; population g is the chains [g * P, (g + 1) * P).  A 256-thread
// workgroup serves one population in the temper and in the resample kernel, so nothing a
// population computes depends on G or on its place in the batch.
//
// TEMPER.  e_i = l_i - m (m the largest finite l) is written once -- to LDS for P <= 8192,
// else to the w output, which the last pass overwrites -- and every pass reads it back:
// thread j owns the particles j, j + 256, ... in all passes, so no pass needs a barrier
// for the data, only the two of the sum.  A pass evaluates S1 = sum w, S2 = sum w^2 at one
// step d; up to 1 + n_bisect + 1 passes.  Every thread holds the same sums (same bits), so
// the bisection runs in uniform control flow without a broadcast.
//
// RESAMPLE.  Thread j owns the contiguous particles [j L, (j + 1) L), L = ceil(P / 256):
// a running sum per segment, a serial walk over the 256 segment totals by thread 0, and
// cs_i = E_j + r_i.  Both cs and the targets t_k ascend, so a segment's outputs are one
// contiguous run of k: the thread finds its first k by bisection on the function t_k (no
// array of prefix sums is ever stored) and walks its particles once more, emitting k while
// t_k < cs_i.  One dominant weight makes one thread write all P outputs: the cost of the
// method's worst case, not of the common one (the temper step holds ESS at rho P).
//
// GATHER.  A chain's row is moved by LPC = 8 .. 256 threads, sized to the row, with 16-byte
// accesses where both rows are 16-byte aligned, as replica.hip moves a partner's row; the
// source row is ancestor[c].  One read and one write of a row per chain: HBM-bound.
// FP64 throughout, exp / log of the device library (within 1 ulp).  gfx950, wave64.
#include "common.hpp"
#include "philox_draws.hpp"

#include <math.h>

namespace binf {

constexpr int SMC_THREADS = 256;
constexpr int64_t SMC_LDS_P = 8192;         // e_i in LDS up to here (64 KiB)

// all lanes: the balanced tree over neighbouring lanes (2, 4, 8, 16, 32, 64)
__device__ inline double smc_wave_sum(double r, int lane)
{
    r = r + xor1_f64(r);
    r = r + xor2_f64(r);
    r = r + other_quad_f64(r);
#pragma unroll
    for (int l = 0; l < 3; ++l) r = r + xor_level_f64(r, l, lane);
    return r;
}

__device__ inline double smc_wave_max(double r, int lane)
{
    r = fmax(r, xor1_f64(r));
    r = fmax(r, xor2_f64(r));
    r = fmax(r, other_quad_f64(r));
#pragma unroll
    for (int l = 0; l < 3; ++l) r = fmax(r, xor_level_f64(r, l, lane));
    return r;
}

// all 256 threads: ((w0 + w1) + w2) + w3 of two sums at once; sh holds 8 doubles
__device__ inline void smc_block_sum2(double &a, double &b, double *sh)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    a = smc_wave_sum(a, lane);
    b = smc_wave_sum(b, lane);
    __syncthreads();
    if (lane == 0) { sh[wave] = a; sh[4 + wave] = b; }
    __syncthreads();
    a = ((sh[0] + sh[1]) + sh[2]) + sh[3];
    b = ((sh[4] + sh[5]) + sh[6]) + sh[7];
}

struct SmcTemperArgs {
    const double *ll;
    double *beta, *delta, *beta_chain, *w, *log_z_inc, *ess;
    int64_t *n_invalid;
    int32_t *status;
    int64_t P;
    double rho;
    int32_t n_bisect;
};

template <bool LDS>
__global__ void __launch_bounds__(SMC_THREADS) smc_temper_kernel(const SmcTemperArgs a)
{
    extern __shared__ double smc_e[];
    __shared__ double sh[8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t g = blockIdx.x, P = a.P;
    const double *ll = a.ll + g * P;
    double *w = a.w + g * P;
    double *bc = a.beta_chain + g * P;
    double *e = LDS ? smc_e : w;

    // classify: the largest finite l, the NaN, the +inf
    double mx = -INFINITY, nnan = 0.0, npinf = 0.0;
    for (int64_t i = tid; i < P; i += SMC_THREADS) {
        const double v = ll[i];
        if (v != v) nnan = nnan + 1.0;
        else if (v == INFINITY) npinf = npinf + 1.0;
        else mx = fmax(mx, v);
    }
    mx = smc_wave_max(mx, lane);
    __syncthreads();
    if (lane == 0) sh[wave] = mx;
    __syncthreads();
    mx = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
    smc_block_sum2(nnan, npinf, sh);

    const double beta = a.beta[g];
    int32_t status = BINF_SMC_OK;
    if (!(beta < 1.0)) status = BINF_SMC_FINISHED;
    else if (npinf > 0.0) status = BINF_SMC_INVALID;
    else if (!(mx > -INFINITY)) status = BINF_SMC_NO_FINITE;
    if (status != BINF_SMC_OK) {
        for (int64_t i = tid; i < P; i += SMC_THREADS) { w[i] = 1.0; bc[i] = beta; }
        if (tid == 0) {
            a.delta[g] = 0.0;
            a.beta[g] = beta;
            a.log_z_inc[g] = 0.0;
            a.ess[g] = (double)P;
            a.n_invalid[g] = (int64_t)nnan;
            a.status[g] = status;
        }
        return;
    }

    for (int64_t i = tid; i < P; i += SMC_THREADS) {
        const double v = ll[i];
        e[i] = (v == v && v > -INFINITY) ? v - mx : -INFINITY;
    }
    // S1, S2 at the step d, the same bits in every thread; STORE: the weights go to w
    auto pass = [&](double d, double &s1, double &s2, bool store) {
        s1 = 0.0;
        s2 = 0.0;
        for (int64_t i = tid; i < P; i += SMC_THREADS) {
            const double ei = e[i];
            const double wi = ei > -INFINITY ? exp(d * ei) : 0.0;
            s1 = s1 + wi;
            s2 = s2 + wi * wi;
            if (store) w[i] = wi;
        }
        smc_block_sum2(s1, s2, sh);
    };
    const double need = a.rho * (double)P;
    const double hi0 = 1.0 - beta;
    double s1, s2, delta, beta_new;
    pass(hi0, s1, s2, false);
    if ((s1 * s1) / s2 >= need) {
        delta = hi0;
        beta_new = 1.0;
    } else {
        double lo = 0.0, hi = hi0;
        for (int k = 0; k < a.n_bisect; ++k) {
            const double mid = 0.5 * (lo + hi);
            pass(mid, s1, s2, false);
            if ((s1 * s1) / s2 >= need) lo = mid; else hi = mid;
        }
        delta = lo;
        if (lo == 0.0) { delta = hi; status = BINF_SMC_STALLED; }
        beta_new = beta + delta;
    }
    pass(delta, s1, s2, true);
    for (int64_t i = tid; i < P; i += SMC_THREADS) bc[i] = beta_new;
    if (tid == 0) {
        a.delta[g] = delta;
        a.beta[g] = beta_new;
        a.log_z_inc[g] = delta * mx + (log(s1) - log((double)P));
        a.ess[g] = (s1 * s1) / s2;
        a.n_invalid[g] = (int64_t)nnan;
        a.status[g] = status;
    }
}

struct SmcResampleArgs {
    const double *w;
    const double *u;            // null: generated
    const int32_t *status;      // null: every population resamples
    int64_t *ancestor, *n_unique;
    int64_t P;
    int64_t chain_offset;
    uint64_t seed, offset;
};

__device__ inline double smc_target(int64_t k, double u, double fP, double total)
{
    return (((double)k + u) / fP) * total;
}

// the first k in [0, P] with t_k >= bound (P: none)
__device__ inline int64_t smc_first_target(double bound, int64_t P, double u, double fP, double total)
{
    int64_t lo = 0, hi = P;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (smc_target(mid, u, fP, total) >= bound) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__global__ void __launch_bounds__(SMC_THREADS) smc_resample_kernel(const SmcResampleArgs a)
{
    __shared__ double shT[SMC_THREADS];         // segment totals, then their exclusive sums
    __shared__ int64_t shL[SMC_THREADS];        // a segment's last particle of positive weight
    __shared__ double sh_total;
    __shared__ int64_t sh_last;
    __shared__ unsigned long long sh_count;
    const int tid = threadIdx.x;
    const int64_t g = blockIdx.x, P = a.P, base = g * P;
    const double *w = a.w + base;
    int64_t *anc = a.ancestor + base;
    const int64_t L = (P + SMC_THREADS - 1) / SMC_THREADS;
    const int64_t i0 = (int64_t)tid * L < P ? (int64_t)tid * L : P;
    const int64_t i1 = i0 + L < P ? i0 + L : P;

    double r = 0.0;
    int64_t last = -1;
    for (int64_t i = i0; i < i1; ++i) {
        const double wi = w[i];
        r = i == i0 ? wi : r + wi;
        if (wi > 0.0) last = i;
    }
    shT[tid] = r;
    shL[tid] = last;
    if (tid == 0) sh_count = 0;
    __syncthreads();
    if (tid == 0) {
        double E = 0.0;
        int64_t lp = -1;
        for (int j = 0; j < SMC_THREADS; ++j) {
            const double T = shT[j];
            shT[j] = E;
            E = E + T;
            if (shL[j] > lp) lp = shL[j];
        }
        sh_total = E;
        sh_last = lp;
    }
    __syncthreads();
    const double total = sh_total;
    const double u = a.u ? a.u[g] : uniform_elem(a.chain_offset + base, a.seed, a.offset);
    const int32_t st = a.status ? a.status[g] : BINF_SMC_OK;
    const bool pass_through = st == BINF_SMC_FINISHED || st == BINF_SMC_INVALID || st == BINF_SMC_NO_FINITE;
    if (pass_through || !(total > 0.0 && total < INFINITY) || !(u >= 0.0 && u < 1.0)) {
        for (int64_t k = tid; k < P; k += SMC_THREADS) anc[k] = base + k;
        if (tid == 0) a.n_unique[g] = P;
        return;
    }
    const double fP = (double)P;
    if (i0 < i1) {
        const double E = shT[tid];
        int64_t k = smc_first_target(E, P, u, fP, total);
        for (int64_t i = i0; i < i1 && k < P; ++i) {
            const double wi = w[i];
            r = i == i0 ? wi : r + wi;
            const double cs = E + r;
            while (k < P && smc_target(k, u, fP, total) < cs) anc[k++] = base + i;
        }
    }
    // targets no prefix sum exceeds: the last particle of positive weight
    const int64_t kf = smc_first_target(total, P, u, fP, total);
    const int64_t lp = base + sh_last;
    for (int64_t k = kf + tid; k < P; k += SMC_THREADS) anc[k] = lp;
    __syncthreads();
    unsigned long long n = 0;
    for (int64_t k = tid; k < P; k += SMC_THREADS) n += (k == 0 || anc[k] != anc[k - 1]) ? 1 : 0;
    if (n) atomicAdd(&sh_count, n);
    __syncthreads();
    if (tid == 0) a.n_unique[g] = (int64_t)sh_count;
}

struct SmcGatherArgs {
    const double *x;
    const int64_t *ancestor;
    double *out;
    const double *side_in;
    double *side_out;
    int64_t C, D;
    int32_t n_side;
    int32_t lpc;                // threads per chain (power of two, 8..256)
};

__global__ void __launch_bounds__(256) smc_gather_kernel(const SmcGatherArgs a)
{
    const int lpc = a.lpc;
    const int sub = threadIdx.x & (lpc - 1);
    const int64_t c = (int64_t)blockIdx.x * (256 / lpc) + threadIdx.x / lpc;
    if (c >= a.C) return;
    const int64_t D = a.D;
    const int64_t s = a.ancestor[c];
    const bool ok = s >= 0 && s < a.C;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    double *dst = a.out + c * D;
    if (ok) {
        const double *src = a.x + s * D;
        if (((((uintptr_t)src) | ((uintptr_t)dst)) & 15) == 0) {
            const int64_t even = D & ~(int64_t)1;
            for (int64_t i = (int64_t)sub * 2; i < even; i += (int64_t)lpc * 2)
                *reinterpret_cast<double2 *>(dst + i) = *reinterpret_cast<const double2 *>(src + i);
            if ((D & 1) && sub == 0) dst[D - 1] = src[D - 1];
        } else {
            for (int64_t i = sub; i < D; i += lpc) dst[i] = src[i];
        }
    } else {
        for (int64_t i = sub; i < D; i += lpc) dst[i] = qnan;
    }
    if (sub == 0) {
        for (int k = 0; k < a.n_side; ++k)
            a.side_out[k * a.C + c] = ok ? a.side_in[k * a.C + s] : qnan;
    }
}

static int32_t smc_shape(const char *what, int64_t C, int64_t P, int64_t G)
{
    if (C < 0 || P < 0 || G < 0) return fail(BINF_E_ARG, "%s: negative size", what);
    if (P < 1 || P > BINF_SMC_MAX_P)
        return fail(BINF_E_UNSUPPORTED, "%s: P = %lld outside 1 ... %d", what, (long long)P, BINF_SMC_MAX_P);
    if (G > 0x7fffffffLL) return fail(BINF_E_UNSUPPORTED, "%s: too many populations", what);
    if (G * P != C) return fail(BINF_E_ARG, "%s: C is not G * P", what);
    return 0;
}

}  // namespace binf

using namespace binf;

extern "C" int32_t binf_smc_temper_f64(const double *ll, double *beta, int64_t C, int64_t P,
                                       int64_t G, double ess_fraction, int32_t n_bisect,
                                       double *delta, double *beta_chain, double *w,
                                       double *log_z_inc, double *ess, int64_t *n_invalid,
                                       int32_t *status, void *stream)
{
    const char *what = "smc_temper";
    const int32_t rc = smc_shape(what, C, P, G);
    if (rc) return rc;
    if (!(ess_fraction > 0.0 && ess_fraction <= 1.0))
        return fail(BINF_E_ARG, "%s: ess_fraction %g outside (0, 1]", what, ess_fraction);
    if (n_bisect < 1 || n_bisect > 128) return fail(BINF_E_ARG, "%s: n_bisect %d outside 1 ... 128", what, n_bisect);
    if (C == 0) return 0;
    if (!ll || !beta || !delta || !beta_chain || !w || !log_z_inc || !ess || !n_invalid || !status)
        return fail(BINF_E_ARG, "%s: null buffer", what);
    if (overlap_f64(w, C, ll, C) || overlap_f64(beta_chain, C, ll, C) || overlap_f64(beta_chain, C, w, C))
        return fail(BINF_E_ALIAS, "%s: w, beta_chain and ll must not overlap (w is the kernel's "
                    "scratch while ll is still read)", what);
    SmcTemperArgs a;
    a.ll = ll; a.beta = beta; a.delta = delta; a.beta_chain = beta_chain; a.w = w;
    a.log_z_inc = log_z_inc; a.ess = ess; a.n_invalid = n_invalid; a.status = status;
    a.P = P; a.rho = ess_fraction; a.n_bisect = n_bisect;
    if (P <= SMC_LDS_P)
        smc_temper_kernel<true><<<dim3((unsigned)G), SMC_THREADS, (size_t)P * 8, (hipStream_t)stream>>>(a);
    else
        smc_temper_kernel<false><<<dim3((unsigned)G), SMC_THREADS, 0, (hipStream_t)stream>>>(a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what);
    return 0;
}

extern "C" int32_t binf_smc_resample_f64(const double *w, const double *u, const int32_t *status,
                                         int64_t C, int64_t P, int64_t G, uint64_t seed,
                                         uint64_t offset, int64_t chain_offset, int64_t *ancestor,
                                         int64_t *n_unique, void *stream)
{
    const char *what = "smc_resample";
    const int32_t rc = smc_shape(what, C, P, G);
    if (rc) return rc;
    if (chain_offset < 0) return fail(BINF_E_ARG, "%s: negative chain_offset", what);
    if (C == 0) return 0;
    if (!w || !ancestor || !n_unique) return fail(BINF_E_ARG, "%s: null buffer", what);
    if (overlap_f64(ancestor, C, w, C))
        return fail(BINF_E_ALIAS, "%s: ancestor overlaps w", what);
    SmcResampleArgs a;
    a.w = w; a.u = u; a.status = status; a.ancestor = ancestor; a.n_unique = n_unique;
    a.P = P; a.chain_offset = chain_offset; a.seed = seed; a.offset = offset;
    smc_resample_kernel<<<dim3((unsigned)G), SMC_THREADS, 0, (hipStream_t)stream>>>(a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what);
    return 0;
}

extern "C" int32_t binf_smc_gather_f64(const double *x, const int64_t *ancestor, double *out,
                                       const double *side_in, double *side_out, int32_t n_side,
                                       int64_t C, int64_t D, void *stream)
{
    const char *what = "smc_gather";
    if (C < 0 || D < 0) return fail(BINF_E_ARG, "%s: negative size", what);
    if (n_side < 0 || n_side > 4) return fail(BINF_E_ARG, "%s: n_side %d outside 0 ... 4", what, n_side);
    if (C == 0) return 0;
    if (!ancestor) return fail(BINF_E_ARG, "%s: null ancestor", what);
    if (D > 0 && (!x || !out)) return fail(BINF_E_ARG, "%s: null buffer", what);
    if (n_side > 0 && (!side_in || !side_out)) return fail(BINF_E_ARG, "%s: null side buffer", what);
    if (D > 0 && C > 0x7fffffffffffffffLL / 8 / D) return fail(BINF_E_ARG, "%s: C*D overflows", what);
    const int64_t nS = (int64_t)n_side * C;
    if (D > 0 && overlap_f64(out, C * D, x, C * D))
        return fail(BINF_E_ALIAS, "%s: out overlaps x (an ancestor's row is read after its own "
                    "chain may have been written)", what);
    if (overlap_f64(side_out, nS, side_in, nS))
        return fail(BINF_E_ALIAS, "%s: side_out overlaps side_in", what);
    if (overlap_f64(ancestor, C, side_out, nS) || (D > 0 && overlap_f64(ancestor, C, out, C * D)) ||
        (D > 0 && overlap_f64(side_out, nS, out, C * D)))
        return fail(BINF_E_ALIAS, "%s: an output overlaps the ancestors or the other output", what);
    if (D == 0 && n_side == 0) return 0;
    SmcGatherArgs a;
    a.x = x; a.ancestor = ancestor; a.out = out; a.side_in = side_in; a.side_out = side_out;
    a.C = C; a.D = D; a.n_side = n_side;
    const bool vec2 = D % 2 == 0 && ((((uintptr_t)x) | ((uintptr_t)out)) & 15) == 0;
    const int64_t per_thread = vec2 ? 2 : 1;
    int lpc = 8;
    while (lpc < 256 && (int64_t)lpc * per_thread < D) lpc <<= 1;
    a.lpc = lpc;
    const int64_t blocks = (C + 256 / lpc - 1) / (256 / lpc);
    if (blocks > 0x7fffffffLL) return fail(BINF_E_UNSUPPORTED, "%s: too many chains", what);
    smc_gather_kernel<<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what);
    return 0;
}
