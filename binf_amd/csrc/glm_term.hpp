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
// negative-binomial-log (NB2: mean exp(eta), variance mean + mean^2 / phi), given the
// chain's lam = log(phi) and phi:
//   z  = eta - lam
//   m  = y + phi
//   then the binomial-logit lines at (z, y, m): ll = y * z - (y + phi) * softplus(z),
//   g = (y + phi) * logistic(z) - y.  What is left of the log density,
//   sum_{j<y} log(phi + j) - lgamma(y + 1), holds no eta: the count term of negbin.hip
//   and the caller's constant.
// The kernels hand the term a lam inside [BINF_NEGBIN_LAM_MIN, BINF_NEGBIN_LAM_MAX]
// (negbin_lam below), where phi = exp(lam) is a normal double: g is finite for every
// finite eta, ll is while (y + phi) * softplus(z) is a double (-inf beyond: phi near
// e**709 with z > 0); never NaN.
#pragma once

#include <math.h>

#ifndef BINF_GLM_NEGBIN_LOG
#define BINF_GLM_NEGBIN_LOG 2
#endif

namespace binf {

// The regular range of lam = log(phi): exp(-708) = 3.3e-308 is a normal double,
// exp(709) = 8.2e307 a finite one.  A chain whose lam lies outside it (NaN included)
// has log-prob -inf; its term is evaluated at the nearer end of the range, so that no
// NaN arises and its gradient is that of the end.
constexpr double BINF_NEGBIN_LAM_MIN = -708.0;
constexpr double BINF_NEGBIN_LAM_MAX = 709.0;

__host__ __device__ inline bool negbin_regular(double lam)
{
    return lam >= BINF_NEGBIN_LAM_MIN && lam <= BINF_NEGBIN_LAM_MAX;
}

__host__ __device__ inline double negbin_lam(double lam)
{
    return lam >= BINF_NEGBIN_LAM_MIN ? (lam <= BINF_NEGBIN_LAM_MAX ? lam : BINF_NEGBIN_LAM_MAX)
                                      : BINF_NEGBIN_LAM_MIN;
}

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

// the term of FAMILY with the chain's (lam, phi) at hand: read by the negative binomial
// alone, whose two own operations are each rounded before the binomial lines
template <int FAMILY, bool WANT_LL, bool WANT_G>
__device__ inline void glm_term_chain(double eta, double y, double m, double lam, double phi,
                                      double &ll, double &g)
{
    if constexpr (FAMILY == BINF_GLM_NEGBIN_LOG) {
        const double z = eta - lam;
        const double mm = y + phi;
        glm_term<BINF_GLM_BINOMIAL_LOGIT, WANT_LL, WANT_G>(z, y, mm, ll, g);
    } else {
        glm_term<FAMILY, WANT_LL, WANT_G>(eta, y, m, ll, g);
    }
}

}  // namespace binf
