// The per-point term of the Gaussian error model, shared by the kernels that evaluate it
// sample by sample: predict.hip (the posterior-predictive density of a grid) and loo.hip
// (the pointwise log-likelihood record).  One order of operations for both, so that a
// record built from binf_gauss_pointwise_loglik_f64 holds the very terms the predictive
// density sums.
#pragma once

namespace binf {

// max that keeps a NaN once it has seen one (np.max propagates NaN)
__device__ inline double nan_max(double m, double f) { return (f > m || f != f) ? f : m; }

__device__ inline double predictive_term(double m, double y, double prec, double hlp,
                                         double half_log_2pi)
{
    const double d = m - y;
    return (-0.5 * (d * d)) * prec + hlp - half_log_2pi;
}

}  // namespace binf
