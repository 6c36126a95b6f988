// Per-thread arithmetic of the convergence diagnostics (diagnostics.hip), host + device so
// that the loops can be run against a plain restatement on the host as well.  Every
// multiply and add is rounded separately (common.hpp turns contraction off).
#pragma once
#include <stdint.h>

#ifndef BINF_HD
#ifdef __HIPCC__
#define BINF_HD __host__ __device__
#else
#define BINF_HD
#endif
#endif

namespace binf {

constexpr int DIAG_LT = 16;        // lags per thread: the register window of the autocovariance
constexpr int DIAG_CHAIN_BLOCK = 64;   // split chains per block of the cross-chain sums

// One pass over the n draws x[t * st], t < n, of a split chain and dimension:
//   K0 = x[0], d_t = x[t] - K0, s1 = sum d_t, s2 = sum d_t * d_t (from 0.0, in t order)
//   mean = K0 + s1 / n,  m2 = s2 - (s1 * s1) / n
struct DiagMoments {
    double k0, s1, s2;
    BINF_HD inline void start(double first) { k0 = first; s1 = 0.0; s2 = 0.0; }
    BINF_HD inline void add(double x)
    {
        const double d = x - k0;
        s1 = s1 + d;
        s2 = s2 + d * d;
    }
    BINF_HD inline double mean(double n) const { return k0 + s1 / n; }
    BINF_HD inline double m2(double n) const { return s2 - (s1 * s1) / n; }
};

// acc[j] = sum_{i < n - k} c_i * c_{i+k}, k = k0 + j, c_i = x[i * st] - mean, each lag's sum
// from 0.0 in i order.  The loop advances DIAG_LT draws at a time with the next 2 * DIAG_LT
// centred draws of the lagged side in registers, so each load feeds DIAG_LT multiply-adds.
// While every product of a step exists for every lag of the tile the step is straight-line
// code; the last two or three steps test each product (i + k < n: uniform over a wave, so a
// scalar branch; a product that does not exist is skipped, never multiplied by zero -- a NaN
// or inf beside it must not leak).  Every load of a step is issued before its first use and
// none depends on a test: an index at or beyond draw n is clamped to n - 1 (read, not used).
// Lags with k >= n stay 0.0.  Never reads x at or beyond draw n.
BINF_HD inline void diag_autocov_lags(const double *x, int64_t st, int64_t n, double mean,
                                      int64_t k0, double acc[DIAG_LT])
{
    constexpr int LT = DIAG_LT;
    const int64_t last = n - 1;
    auto at = [&](int64_t t) { return x[(t < last ? t : last) * st] - mean; };
#pragma unroll
    for (int j = 0; j < LT; ++j) acc[j] = 0.0;
    double w[2 * LT];
#pragma unroll
    for (int j = 0; j < LT; ++j) w[j] = at(k0 + j);
    for (int64_t i0 = 0; i0 + k0 < n; i0 += LT) {
#pragma unroll
        for (int j = 0; j < LT; ++j) w[LT + j] = at(i0 + k0 + LT + j);
        if (i0 + k0 + 2 * LT - 2 < n) {
#pragma unroll
            for (int u = 0; u < LT; ++u) {
                const double cu = at(i0 + u);
#pragma unroll
                for (int j = 0; j < LT; ++j) acc[j] = acc[j] + cu * w[u + j];
            }
        } else {
#pragma unroll
            for (int u = 0; u < LT; ++u) {
                const double cu = at(i0 + u);
#pragma unroll
                for (int j = 0; j < LT; ++j)
                    if (i0 + u + k0 + j < n) acc[j] = acc[j] + cu * w[u + j];
            }
        }
#pragma unroll
        for (int j = 0; j < LT; ++j) w[j] = w[LT + j];
    }
}

}  // namespace binf
