// The count term of the negative-binomial error model (glm_term.hpp): the part of its log
// density that holds phi = exp(lam) and the data but no linear predictor,
//
//   sum_n sum_{j < y_n} log(phi + j)  =  sum_{j = 0}^{ymax - 1} T_j log(phi + j),
//
// with the integer tail counts T_j = #{n : y_n > j}, computed once on the host and handed
// over as doubles (exact: T_j <= N < 2^31).  No lgamma on the device and none of the
// cancellation of lgamma(y + phi) - lgamma(phi) at large phi.  gfx950 (MI355X), wave64.
//
// Both orders are functions of the table alone (ymax, the distinct values), never of C:
//
// log_norm_chain[c] = (sum_j T_j log(phi_c + j)) + log_norm.  One workgroup of 256 threads
//   per chain.  Thread t sums the terms fl(T_j * log(fl(phi + j))) of j = t, t + 256, ...
//   ascending from 0.0; the 64 sums of a wave are joined by the butterfly x = x + x[lane ^ o],
//   o = 1, 2, 4, 8, 16, 32; the four wave sums as (0 + 1) + (2 + 3); log_norm last.  ymax = 0:
//   log_norm itself.
//
// prefix[s][k] = sum_{j < v_k} log(phi_s + j) at the distinct values v_0 < v_1 < ... of ys.
//   One thread per row s walks j = 0, 1, ... ascending from 0.0, adding fl(log(fl(phi + j))),
//   and writes the running sum when j reaches v_k: every entry is a prefix of ONE sequence.
//
// phi = exp(lam) with lam clamped to the regular range, as every kernel of the family has it;
// a lam outside the range: log_norm_chain = -inf, the prefix row as at the nearer end (the
// record's -inf is the pointwise kernel's).
#include "common.hpp"
#include "glm_term.hpp"

#include <math.h>

namespace binf {

constexpr int64_t NEGBIN_MAX_COUNT = 1LL << 20;

__global__ void __launch_bounds__(256)
negbin_chain_term_kernel(const double *lam, const double *tail, int32_t ymax, double log_norm,
                         double *out)
{
    __shared__ double sw[4];
    const int64_t c = blockIdx.x;
    const int tid = threadIdx.x;
    const double l = lam[c];
    const double phi = exp(negbin_lam(l));
    double acc = 0.0;
    for (int j = tid; j < ymax; j += 256) {
        const double x = phi + (double)j;
        const double lg = log(x);
        acc = acc + tail[j] * lg;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) acc = acc + shfl_xor_f64(acc, o);
    if ((tid & 63) == 0) sw[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        const double s = ((sw[0] + sw[1]) + (sw[2] + sw[3])) + log_norm;
        out[c] = negbin_regular(l) ? s : -INFINITY;
    }
}

__global__ void __launch_bounds__(256)
negbin_prefix_kernel(const double *lam, const double *values, double *out, int64_t S, int64_t J)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= S) return;
    const double phi = exp(negbin_lam(lam[s]));
    double acc = 0.0;
    int64_t j = 0;
    for (int64_t k = 0; k < J; ++k) {
        double v = values[k];
        if (!(v <= (double)NEGBIN_MAX_COUNT)) v = (double)NEGBIN_MAX_COUNT;   // bounded walk
        for (; (double)j < v; ++j) {
            const double x = phi + (double)j;
            acc = acc + log(x);
        }
        out[s * J + k] = acc;
    }
}

}  // namespace binf

using namespace binf;

extern "C" int32_t binf_negbin_count_term_f64(const double *log_dispersion,
                                              const double *tail_counts, int64_t ymax,
                                              double log_norm, double *out_chain,
                                              const double *values, int64_t J,
                                              double *out_prefix, int64_t C, void *stream)
{
    const char *what = "negbin_count_term";
    if (C < 0 || ymax < 0 || J < 0) return fail(BINF_E_ARG, "%s: need C>=0, ymax>=0, J>=0", what);
    if (!out_chain && !out_prefix) return fail(BINF_E_ARG, "%s: no output", what);
    if (ymax > NEGBIN_MAX_COUNT)
        return fail(BINF_E_UNSUPPORTED, "%s: counts above 2^20 (ymax=%lld) are not covered", what,
                    (long long)ymax);
    if (C > 0x7fffffffLL || J > NEGBIN_MAX_COUNT + 1)
        return fail(BINF_E_UNSUPPORTED, "%s: too large", what);
    if (C == 0) return 0;
    if (!log_dispersion) return fail(BINF_E_ARG, "%s: null buffer", what);
    if (out_chain && ymax > 0 && !tail_counts) return fail(BINF_E_ARG, "%s: null tail counts", what);
    if (out_prefix && (J < 1 || !values)) return fail(BINF_E_ARG, "%s: a prefix needs J>=1 values", what);
    if (overlap_f64(out_chain, C, log_dispersion, C) || overlap_f64(out_chain, C, tail_counts, ymax) ||
        overlap_f64(out_chain, C, values, J) || overlap_f64(out_prefix, C * J, log_dispersion, C) ||
        overlap_f64(out_prefix, C * J, tail_counts, ymax) || overlap_f64(out_prefix, C * J, values, J))
        return fail(BINF_E_ALIAS, "%s: an output overlaps an input", what);
    if (overlap_f64(out_chain, C, out_prefix, C * J))
        return fail(BINF_E_ALIAS, "%s: the outputs overlap", what);
    hipStream_t st = (hipStream_t)stream;
    if (out_chain) {
        negbin_chain_term_kernel<<<dim3((unsigned)C), 256, 0, st>>>(
            log_dispersion, tail_counts, (int32_t)ymax, log_norm, out_chain);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, "negbin_count_term launch");
    }
    if (out_prefix) {
        negbin_prefix_kernel<<<dim3((unsigned)((C + 255) / 256)), 256, 0, st>>>(
            log_dispersion, values, out_prefix, C, J);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, "negbin_count_term prefix launch");
    }
    return 0;
}
