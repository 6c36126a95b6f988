// Generic per-step tier: the pieces of HMCSampler.sample() as separate
// chain-batched kernels, for posteriors whose gradient is evaluated by other
// code (any AbstractBinfPDF-shaped plug-in).  gfx950, wave64.
//
// Reference lines replaced: binf/samplers/hmc.py:116-123 (kick / drift: the
// identity entry points of the one element-wise kernel, leapfrog_ew.hpp),
// :148,150 (energy reductions), :151-164 (accept, adapt, select) and the
// TestHO gradient binf/pdf/__init__.py:191.
#include "rowsum.hpp"
#include "gauss_common.hpp"
#include "leapfrog_ew.hpp"

namespace binf {

// ---------------------------------------------------------------------------
// row reductions in numpy's pairwise order (machinery: rowsum.hpp)
// ---------------------------------------------------------------------------
enum { OP_SUM = 0, OP_SUMSQ = 1, OP_SUMSQ_SHIFT = 2, OP_SUMSQ_DIFF = 3, OP_SUMSQ_DIFF_DIV = 4 };

struct RedArgs {
    const double *x;
    const double *y;     // OP_SUMSQ_DIFF*: per-column vector subtracted first
    const double *w;     // OP_SUMSQ_DIFF_DIV: per-column divisor of the square
    double shift;
    int64_t D;
};

template <int OP>
struct RedElem {
    const double *row;
    const double *y;
    const double *w;
    double shift;
    __device__ inline double operator()(int i) const
    {
        const double x = row[i];
        if (OP == OP_SUM) return x;
        if (OP == OP_SUMSQ) return x * x;
        const double d = (OP == OP_SUMSQ_SHIFT) ? x - shift : x - y[i];
        if (OP == OP_SUMSQ_DIFF_DIV) return d * d / w[i];
        return d * d;
    }
};

template <int OP>
struct RedMake {
    __device__ static inline RedElem<OP> make(const RedArgs &a, int64_t row)
    {
        return RedElem<OP>{a.x + row * a.D, a.y, a.w, a.shift};
    }
};

// ---------------------------------------------------------------------------
// the TestHO gradient k * (x - x0) (pdf/__init__.py:191): the leapfrog kernel's flat grid
// and 16-byte accesses (leapfrog_ew.hpp), one input and one output
// ---------------------------------------------------------------------------
template <int VEC>
__global__ void __launch_bounds__(256)
gauss_grad_kernel(const double *x, double *out, double k, double x0, int64_t n)
{
    const int64_t span = (int64_t)256 * VEC * EW_UNR;            // elements per workgroup pass
    for (int64_t b0 = (int64_t)blockIdx.x * span; b0 < n; b0 += (int64_t)gridDim.x * span) {
        double xv[EW_UNR][VEC];
        int64_t idx[EW_UNR];
#pragma unroll
        for (int r = 0; r < EW_UNR; ++r) {
            idx[r] = b0 + ((int64_t)r * 256 + threadIdx.x) * VEC;
            if (idx[r] < n) ew_load<VEC>(xv[r], x, idx[r]);
        }
#pragma unroll
        for (int r = 0; r < EW_UNR; ++r) {
            if (idx[r] >= n) continue;
#pragma unroll
            for (int v = 0; v < VEC; ++v) xv[r][v] = k * (xv[r][v] - x0);
            ew_store<VEC>(out, idx[r], xv[r]);
        }
    }
}

// ---------------------------------------------------------------------------
// Metropolis accept, step-size adaption, select           hmc.py:151-164,188-191
//
// A chain is served by LPC = 8 .. 256 threads of a workgroup (a power of two
// sized to the row), so short rows (the polynomial model's K = 33 coefficients)
// share a workgroup; every thread of the group evaluates the same accept test
// (same inputs, same bits) and copies its part of the selected row with 16-byte
// accesses where alignment allows.
// ---------------------------------------------------------------------------
struct AcceptArgs {
    const double *q_prop;
    const double *q_old;
    const double *e_before;
    const double *e_after;
    const double *u;
    double *q_out;
    uint8_t *accepted;
    int64_t *n_accepted;
    double *dt_chain;
    double uprate;
    double downrate;
    int64_t C;
    int64_t D;
    int32_t adapt;
    int32_t lpc;        // threads per chain (power of two, 8..256)
};

template <int VEC>
__global__ void __launch_bounds__(256) accept_select_kernel(const AcceptArgs a)
{
    const int lpc = a.lpc;
    const int sub = threadIdx.x & (lpc - 1);
    const int64_t c = (int64_t)blockIdx.x * (256 / lpc) + threadIdx.x / lpc;
    if (c >= a.C) return;
    const bool acc = metropolis_accept(a.u[c], -(a.e_after[c] - a.e_before[c]));
    const double *src = (acc ? a.q_prop : a.q_old) + c * a.D;
    double *dst = a.q_out + c * a.D;
    if (dst != src) {
        for (int64_t i = (int64_t)sub * VEC; i < a.D; i += (int64_t)lpc * VEC) {
            double r[VEC];
            ew_load<VEC>(r, src, i);
            ew_store<VEC>(dst, i, r);
        }
    }
    if (sub == 0) {
        a.accepted[c] = acc ? 1 : 0;
        if (a.n_accepted && acc) a.n_accepted[c] += 1;
        if (a.adapt) {
            const double dt = a.dt_chain[c];
            a.dt_chain[c] = acc ? dt * a.uprate : dt * a.downrate;
        }
    }
}

// csb.numeric.exp: exp(clip(x, -308, 709))
__global__ void __launch_bounds__(256)
clipped_exp_kernel(const double *x, double *out, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * 256) {
        double v = x[i];
        v = (v < -308.0) ? -308.0 : v;
        v = (v > 709.0) ? 709.0 : v;
        out[i] = exp_clipped_range(v);
    }
}

// accept_decide (gauss_common.hpp) elementwise: what makes its three answers testable
__global__ void __launch_bounds__(256)
accept_decide_kernel(const double *u, const double *x, const double *delta, int32_t *out, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * 256)
        out[i] = accept_decide(u[i], x[i], delta[i]);
}

}  // namespace binf

using namespace binf;

extern "C" int32_t binf_accept_decide_f64(const double *u, const double *x, const double *delta,
                                          int32_t *out, int64_t n, void *stream)
{
    if (n < 0) return fail(BINF_E_ARG, "accept_decide: negative size");
    if (n == 0) return 0;
    if (!u || !x || !delta || !out) return fail(BINF_E_ARG, "accept_decide: null buffer");
    int64_t blocks = (n + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    accept_decide_kernel<<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(u, x, delta, out, n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "accept_decide launch");
    return 0;
}

extern "C" int32_t binf_clipped_exp_f64(const double *x, double *out, int64_t n,
                                        void *stream)
{
    if (n < 0) return fail(BINF_E_ARG, "clipped_exp: negative size");
    if (n == 0) return 0;
    if (!x || !out) return fail(BINF_E_ARG, "clipped_exp: null buffer");
    int64_t blocks = (n + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    clipped_exp_kernel<<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(x, out, n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "clipped_exp launch");
    return 0;
}

extern "C" int32_t binf_row_sum_f64(const double *x, double *out, int64_t C,
                                    int64_t D, int32_t op, double shift,
                                    double scale, void *stream)
{
    if (C < 0 || D < 0) return fail(BINF_E_ARG, "row_sum: negative size");
    if (op < 0 || op > 2) return fail(BINF_E_ARG, "row_sum: unknown op %d", op);
    if (C == 0) return 0;
    if ((!x && D > 0) || !out) return fail(BINF_E_ARG, "row_sum: null buffer");
    RedArgs a;
    a.x = x; a.y = nullptr; a.w = nullptr; a.shift = shift; a.D = D;
    hipStream_t st = (hipStream_t)stream;
    switch (op) {
    case OP_SUM: return row_reduce_launch<RedMake<OP_SUM>, RedArgs>(a, C, D, scale, out, st, false, "row_sum");
    case OP_SUMSQ: return row_reduce_launch<RedMake<OP_SUMSQ>, RedArgs>(a, C, D, scale, out, st, false, "row_sum");
    default: return row_reduce_launch<RedMake<OP_SUMSQ_SHIFT>, RedArgs>(a, C, D, scale, out, st, false, "row_sum");
    }
}

// E[c] = -log_prob[c] + 0.5 * np.sum(p[c]**2) (hmc.py:143,148,150) in one launch:
// the kinetic row sum with the subtraction as its epilogue.  (-lp) + k and k - lp
// are the same IEEE operation, so the bits equal the three-launch form.
extern "C" int32_t binf_hmc_energy_f64(const double *p, const double *log_prob, double *out,
                                       int64_t C, int64_t D, void *stream)
{
    if (C < 0 || D < 0) return fail(BINF_E_ARG, "hmc_energy: negative size");
    if (C == 0) return 0;
    if ((!p && D > 0) || !log_prob || !out) return fail(BINF_E_ARG, "hmc_energy: null buffer");
    RedArgs a;
    a.x = p; a.y = nullptr; a.w = nullptr; a.shift = 0.0; a.D = D;
    GaussFinish fin;
    fin.on = 2; fin.tau = 1.0; fin.tau_chain = nullptr; fin.n_data = 0.0; fin.minus = log_prob;
    return row_reduce_launch<RedMake<OP_SUMSQ>, RedArgs>(a, C, D, 0.5, out, (hipStream_t)stream, false,
                                                        "hmc_energy", &fin);
}

extern "C" int32_t binf_row_sumsq_diff_f64(const double *x, const double *y,
                                           const double *w, double *out,
                                           int64_t C, int64_t D, double scale,
                                           void *stream)
{
    if (C < 0 || D < 0) return fail(BINF_E_ARG, "row_sumsq_diff: negative size");
    if (C == 0) return 0;
    if (((!x || !y) && D > 0) || !out) return fail(BINF_E_ARG, "row_sumsq_diff: null buffer");
    RedArgs a;
    a.x = x; a.y = y; a.w = w; a.shift = 0.0; a.D = D;
    if (w)
        return row_reduce_launch<RedMake<OP_SUMSQ_DIFF_DIV>, RedArgs>(a, C, D, scale, out, (hipStream_t)stream, false, "row_sumsq_diff");
    return row_reduce_launch<RedMake<OP_SUMSQ_DIFF>, RedArgs>(a, C, D, scale, out, (hipStream_t)stream, false, "row_sumsq_diff");
}

// The identity entry points check sizes, mode and null buffers only: unlike their metric
// twins (leapfrog_check) they refuse no aliasing.
static int32_t ew_check(int64_t C, int64_t D, int32_t mode, bool any_null, const char *what)
{
    if (C < 0 || D < 0) return fail(BINF_E_ARG, "%s: negative size", what);
    if (mode != BINF_MODE_EXACT && mode != BINF_MODE_FMA)
        return fail(BINF_E_ARG, "%s: unknown mode %d", what, mode);
    if (C == 0 || D == 0) return 0;
    if (any_null) return fail(BINF_E_ARG, "%s: null buffer", what);
    if (C > 0x7fffffffffffffffLL / D) return fail(BINF_E_ARG, "%s: C*D overflows", what);
    return 0;
}

template <int KIND>
static int32_t identity_launch(double *q, double *p, const double *g, double timestep,
                               const double *dt_chain, int32_t half, int64_t C, int64_t D,
                               int32_t mode, void *stream, const char *what)
{
    const int32_t rc = ew_check(C, D, mode, (KIND != LF_KICK && !q) || !p || (KIND != LF_DRIFT && !g), what);
    if (rc != 0 || C == 0 || D == 0) return rc;
    const LeapfrogEwArgs a{q, p, g, timestep, dt_chain, C * D, D};
    LeapfrogEwExtra<KIND, false> x;
    if constexpr (KIND == LF_KICK) x.half = half ? 1 : 0;
    return leapfrog_ew_launch<KIND, false>(a, x, mode, stream, what);
}

extern "C" int32_t binf_leapfrog_kick_f64(double *p, const double *grad,
                                          double timestep, const double *dt_chain,
                                          int32_t half, int64_t C, int64_t D,
                                          int32_t mode, void *stream)
{
    return identity_launch<LF_KICK>(nullptr, p, grad, timestep, dt_chain, half, C, D, mode, stream,
                                    "leapfrog_kick");
}

extern "C" int32_t binf_leapfrog_drift_f64(double *q, const double *p,
                                           double timestep, const double *dt_chain,
                                           int64_t C, int64_t D, int32_t mode,
                                           void *stream)
{
    return identity_launch<LF_DRIFT>(q, const_cast<double *>(p), nullptr, timestep, dt_chain, 0, C, D,
                                     mode, stream, "leapfrog_drift");
}

extern "C" int32_t binf_leapfrog_kick_drift_f64(double *q, double *p, const double *grad,
                                                double timestep, const double *dt_chain,
                                                int64_t C, int64_t D, int32_t mode,
                                                void *stream)
{
    return identity_launch<LF_KICK_DRIFT>(q, p, grad, timestep, dt_chain, 0, C, D, mode, stream,
                                          "leapfrog_kick_drift");
}

extern "C" int32_t binf_gauss_grad_f64(const double *x, double *out, double k,
                                       double x0, int64_t C, int64_t D,
                                       void *stream)
{
    const char *what = "gauss_grad";
    const int32_t rc = ew_check(C, D, BINF_MODE_EXACT, !out || !x, what);
    if (rc != 0 || C == 0 || D == 0) return rc;
    const int64_t n = C * D;
    hipStream_t st = (hipStream_t)stream;
    if (D % 2 == 0 && ew_aligned16(out, x))
        gauss_grad_kernel<2><<<dim3(ew_blocks(n, 2)), 256, 0, st>>>(x, out, k, x0, n);
    else
        gauss_grad_kernel<1><<<dim3(ew_blocks(n, 1)), 256, 0, st>>>(x, out, k, x0, n);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what);
    return 0;
}

extern "C" int32_t binf_accept_select_f64(const double *q_prop, const double *q_old,
                                          const double *e_before, const double *e_after,
                                          const double *u, double *q_out,
                                          uint8_t *accepted, int64_t *n_accepted,
                                          double *dt_chain,
                                          int32_t adapt, double uprate, double downrate,
                                          int64_t C, int64_t D, void *stream)
{
    if (C < 0 || D < 0) return fail(BINF_E_ARG, "accept_select: negative size");
    if (C == 0) return 0;
    if (!q_prop || !q_old || !e_before || !e_after || !u || !q_out || !accepted)
        return fail(BINF_E_ARG, "accept_select: null buffer");
    if (adapt && !dt_chain) return fail(BINF_E_ARG, "accept_select: adapt needs dt_chain");
    AcceptArgs a;
    a.q_prop = q_prop; a.q_old = q_old; a.e_before = e_before; a.e_after = e_after;
    a.u = u; a.q_out = q_out; a.accepted = accepted; a.n_accepted = n_accepted; a.dt_chain = dt_chain;
    a.uprate = uprate; a.downrate = downrate; a.C = C; a.D = D; a.adapt = adapt;
    const bool vec2 = D % 2 == 0 && ew_aligned16(q_prop, q_old, q_out);
    const int64_t per_thread = vec2 ? 2 : 1;
    int lpc = 8;
    while (lpc < 256 && (int64_t)lpc * per_thread < D) lpc <<= 1;
    a.lpc = lpc;
    const int64_t blocks = (C + 256 / lpc - 1) / (256 / lpc);
    if (blocks > 0x7fffffffLL) return fail(BINF_E_UNSUPPORTED, "accept_select: too many chains");
    if (vec2) accept_select_kernel<2><<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(a);
    else      accept_select_kernel<1><<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "accept_select launch");
    return 0;
}
