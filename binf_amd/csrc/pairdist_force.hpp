// Pair-distance model, force side: what every force scheme shares -- the restraint weight of
// a pair, the arguments of a fused leapfrog, and the integrator arithmetic (ONE copy: "the
// fused leapfrog is bit-identical to the per-step tier" is a property of pair_kick below).
// Included by pairdist.hip alone, before the scheme headers.
#pragma once
#include "common.hpp"

namespace binf {

// Restraint weight of one pair: w = (d - y) / d = 1 - y / d with d = |x_i - x_j|.
// IEEE sqrt + IEEE divide cost ~55 FP64 instructions per pair; instead
// 1/d = rsqrt(d^2) from the hardware seed (v_rsq_f64, ~24 good bits) polished
// by ONE Newton step, then one FMA.  The step leaves -1.5 e0^2 of the seed's
// error e0: measured on MI355X, 1/d is within 3.5e-15 relative (2^-48.0, seed
// ~2^-24.3), not the ~1e-15 once stated here (a second step measured 1.1e-15
// vs 6e-15 worst force error against numpy and 6 % more time).
// Used by BOTH force kernels, so the fused leapfrog and the per-step tier stay
// bit-identical to each other; against 50-digit arithmetic every force
// component is held to tau (EPS_W sum_j |y/d| |dx| + (n + 2) u sum_j |w| |dx|),
// EPS_W = 1.5 * 2^-48 + 10u (tests/test_gpu_pairdist_exact.py).
__device__ inline double pair_weight(double d0, double d1, double d2, double y)
{
    const double s = (d0 * d0 + d1 * d1) + d2 * d2;
    double r = __builtin_amdgcn_rsq(s);
    r = r * __builtin_fma(-0.5 * s * r, r, 1.5);
    return __builtin_fma(-y, r, 1.0);
}

__device__ inline double wave_rol1(double v)     // lane l takes lane (l + 1) mod 64's value
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(lo, lo, 0x134, 0xf, 0xf, false);   // old = src: no zeroing mov
    hi = __builtin_amdgcn_update_dpp(hi, hi, 0x134, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

struct PairLeapArgs {
    double *q;               // [C x 3n] in/out
    const double *q_from;    // [C x 3n] start positions when they are not to be read from q, or null
    double *p;               // [C x 3n] in/out
    const double *ymat;      // [n x n]
    const double *ypk;       // sym kernels: the targets in lane order (sym_pack_targets_kernel), or null
    const double *tau_chain; // [C] or null
    const double *dt_chain;  // [C] or null
    double tau;
    double timestep;
    double prior_k;
    double prior_x0;
    int32_t has_prior;
    int32_t prior_first;     // prior term added before the likelihood term
    int32_t nsteps;
    int32_t n_beads;
    int64_t n_chains;        // sym kernels: a workgroup walks chains blockIdx.x, + gridDim.x, ...
};

// One chain of a fused leapfrog: where it reads its start positions (qs), where its
// positions and momenta live, its precision and its time step.
struct PairChain {
    double *qc;
    const double *qs;
    double *pc;
    double tau, dt, hdt;
};

__device__ inline PairChain pair_chain(const PairLeapArgs &a, int64_t c)
{
    const int64_t o = c * 3 * (int64_t)a.n_beads;
    PairChain ch;
    ch.qc = a.q + o;
    ch.qs = (a.q_from ? a.q_from : a.q) + o;
    ch.pc = a.p + o;
    ch.tau = a.tau_chain ? a.tau_chain[c] : a.tau;
    ch.dt = a.dt_chain ? a.dt_chain[c] : a.timestep;
    ch.hdt = 0.5 * ch.dt;
    return ch;
}

// One component of the posterior's gradient: the likelihood's term tau * f and the prior's
// k (q - x0) added in the Posterior's order (component terms in sorted-name order), as the
// per-step tier does it.
__device__ __attribute__((always_inline)) inline double
pair_grad1(const PairLeapArgs &a, double f, double q, double tau)
{
    const double gl = tau * f;
    double g = gl;
    if (a.has_prior) {
        const double gp = a.prior_k * (q - a.prior_x0);
        g = a.prior_first ? gp + gl : gl + gp;
    }
    return g;
}

template <bool FMA>                              // p - step * g
__device__ __attribute__((always_inline)) inline double pair_kick1(double g, double p, double step)
{
    return FMA ? __builtin_fma(-step, g, p) : p - step * g;
}

template <bool FMA>                              // q + p * dt
__device__ __attribute__((always_inline)) inline double pair_drift1(double q, double p, double dt)
{
    return FMA ? __builtin_fma(p, dt, q) : q + p * dt;
}

// One component of a bead's kick from its force f and, when `drift`, of the drift that follows.
// (Per component and by reference on purpose: a form that takes the three components as arrays
// costs the sym kernels, which live at their 128-VGPR bound, up to 48 bytes of scratch per lane.)
template <bool FMA>
__device__ __attribute__((always_inline)) inline void
pair_kick(const PairLeapArgs &a, double f, double &q, double &p, double tau, double step, double dt, bool drift)
{
    p = pair_kick1<FMA>(pair_grad1(a, f, q, tau), p, step);
    if (drift) q = pair_drift1<FMA>(q, p, dt);
}

// out[3 bead + axis] = tau_c * f[axis]: the gradient of the per-step tier
__device__ __attribute__((always_inline)) inline void
store_scaled_force(double *o, double tc, double f0, double f1, double f2)
{
    o[0] = tc * f0;
    o[1] = tc * f1;
    o[2] = tc * f2;
}

}  // namespace binf

