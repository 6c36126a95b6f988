// The per-point term of the two generalised-linear error models, written once: used by
// every kernel of glm.hip (the element-wise record, the fused log-prob, the fused
// gradient and with it the leapfrog) and restated line for line in tests/glm_ref.py.
//
//   eta = mock + offset_n                         (offset 0.0 when absent)
//
// Sign convention of GaussianErrorModel._evaluate_gradient: ll is the log-density term
// WITHOUT its data-only constant, g the derivative of MINUS ll with respect to the mock
// datum.  Every operation is rounded on its own (-ffp-contract=off; common.hpp).
//
// binomial-logit, y successes of m trials (m = 1.0 when absent):
//   t  = exp(-|eta|)
//   sp = max(eta, 0) + log1p(t)                   softplus, finite for every finite eta
//   ll = y * eta - m * sp
//   s  = eta >= 0 ? 1 / (1 + t) : t / (1 + t)     the fixed logistic of free_energy.hip
//   g  = m * s - y
// Poisson-log:
//   e  = exp(eta)
//   ll = y * eta - e                              -inf once exp overflows (eta > 709.78)
//   g  = e - y                                    +inf there; never NaN for y >= 0
//                                                 (while y * eta itself is a double)
#pragma once

#include <math.h>

namespace binf {

template <int FAMILY>
__device__ inline double glm_eta(double mock, double offset) { return mock + offset; }

template <int FAMILY, bool WANT_LL, bool WANT_G>
__device__ inline void glm_term(double eta, double y, double m, double &ll, double &g)
{
    if constexpr (FAMILY == BINF_GLM_BINOMIAL_LOGIT) {
        const double t = exp(-fabs(eta));
        if constexpr (WANT_LL) {
            const double sp = fmax(eta, 0.0) + log1p(t);
            ll = y * eta - m * sp;
        }
        if constexpr (WANT_G) {
            const double d = 1.0 + t;
            const double s = eta >= 0.0 ? 1.0 / d : t / d;
            g = m * s - y;
        }
    } else {
        const double e = exp(eta);
        if constexpr (WANT_LL) ll = y * eta - e;
        if constexpr (WANT_G) g = e - y;
    }
}

}  // namespace binf
