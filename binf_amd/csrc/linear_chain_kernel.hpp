// A linear forward model's posterior (mock = theta . A, Gaussian errors), one chain
// per lane GROUP, any number of Gibbs sweeps per launch: the sibling of
// poly_chain_kernel.hpp for a user's design matrix A [K x N].  One kernel template
// serves
//
//   binf_hmc_sample_linear_f64        one HMCSampler.sample() (hmc_linear.hip):
//                                     GIBBS = false, n = 1, draws and the constant
//                                     log-prob terms supplied by the caller;
//   binf_gibbs_linear_sample_n_f64    n sweeps of the Gibbs loop (gibbs_linear.hip),
//                                     binf/samplers/gibbs.py:146-149 around
//                                       coefficients: HMCSampler.sample (hmc.py:136-164)
//                                                     or RWMCSampler.sample
//                                                     (binf/example/samplers.py:78-92)
//                                       precision:    GammaSampler.sample
//                                                     (binf/example/samplers.py:27-51)
//                                     on a Likelihood of a linear forward model
//                                     (binf/model/forwardmodels.py:23-33,
//                                     binf/pdf/likelihoods.py:141-155), with the state
//                                     of a chain in registers between the sweeps.
//
// Everything but the per-datum model is the polynomial kernel's (the draws, the accept
// clip, adaption, the Gamma draw, records); the argument block, np_sum_k and the host path
// of the entry points are shared (chain_common.hpp): PolyChainArgs with `xs` = the design
// matrix, row-major [K x N].
//
// Mapping: the DATA are spread over the G = 8 * 2^H lanes of a chain in numpy's
// pairwise-tree order (H = tree height of N; lane (leaf g, accumulator j) owns data
// points off_g + 8 t + j, t = 0, 1, ... = "rounds"); theta / p / the force are
// replicated in the registers of the chain's lanes.  Each datum carries a COLUMN of A:
// the workgroup stages the image
//     sa[k][t][slot]  (k < KMAX, t < rounds padded to a multiple of 4, slot < G)
//     sy[t][slot]
// once in dynamic LDS -- the lanes of a group read consecutive doubles, the groups of
// a wave read the same address (a broadcast), so every ds_read_b64 is conflict-free.
// Rows k >= K, rounds past a lane's data and slots past a leaf hold exact zeros.  The
// image is (KMAX + 1) * rounds * G doubles: 136 KiB of the 160 KiB LDS at K = 16,
// N = 1024 (one workgroup per CU there), 16 KiB at K = 9, N = 200.  A is ALWAYS read
// from LDS; there is no L1/L2 path.
//
// Arithmetic contract (all orders are functions of (K, N) alone -- never of the batch,
// a chain's position in it, or chain_offset):
//   mock    v = A[0][n] * theta[0]; v = fma(A[k][n], theta[k], v) for k = 1 .. KMAX-1:
//           ONE fixed chain, the same in the energy and in the force, in both leapfrog
//           modes (rows K .. KMAX-1 are zeros against theta = 0: exact no-ops; KMAX is
//           K rounded up to a multiple of 4).  The reference forms mock with BLAS, whose
//           order is not reproducible: AGAINST THE REFERENCE the energies are held to the
//           rounding bound of a K-term dot product (tests/linear_bounds.py), not to bits.
//           Against this contract, restated on the host (tests/chain_contract.py), states,
//           flags, counters and energies are held BIT FOR BIT
//           (tests/test_gpu_chain_contract.py; the energies under one of the three doubles
//           nearest log tau, the device library's log being within one ulp).
//   chi^2   the squared residuals summed in numpy's pairwise order: per-lane running
//           sums in numpy's accumulator order + the xor-shuffle tree of
//           chain_sum_finish -- np.sum((mock - ys)**2) of the mock above, bit for bit;
//   prior, kinetic energy   np.sum's order over K elements (np_sum_k);
//   force   per column ONE read serves the forward product and the back-contraction:
//           g[k] = fma(A[k][n], (v - y_n) * tau, g[k]) over the lane's data in round
//           order, then an xor-butterfly over the chain's lanes (a + b == b + a: every
//           lane ends with the same bits, the replicas never diverge).
//   n sweeps in one launch run the very instructions of n single launches.
//   A non-finite coefficient poisons its own chain only (every shuffle stays inside
//   the chain's lane group): its energies are NaN, its move is rejected, its state kept.
//
// Budget (from the guide's figures, not measured for this kernel): ds_read_b64 moves
// 256 B/clk/CU = 32 doubles, the FP64 pipe does 64 lane-FMAs/clk/CU; a column element
// read once feeds two FMAs, so the two roughly balance.  Reading the column twice
// would make LDS the bound.
// gfx950, wave64.
#pragma once
#include "chain_common.hpp"

namespace binf {

// rounds of the LDS image: tcount padded to a multiple of 4 (the widest interleave)
inline int32_t linear_chain_rounds(int32_t tcount) { return (tcount + 3) & ~3; }

inline size_t linear_chain_lds_bytes(int kmax, int32_t tcount, int32_t H)
{
    return (size_t)(kmax + 1) * (size_t)linear_chain_rounds(tcount) * (size_t)(8 << H) *
           sizeof(double);
}

template <int KMAX, bool FMA, bool GIBBS, int MOVE>
__global__ void __launch_bounds__(256) linear_chain_kernel(const PolyChainArgs a)
{
    // rounds in flight: their mock chains are independent (latency), a column element
    // is held until its back-contraction (registers)
    constexpr int R = KMAX <= 8 ? 4 : 2;
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int K = a.K, N = a.N, H = a.H;
    const int lg = 3 + H;
    const int G = 1 << lg;
    const int slot = lane & (G - 1);
    const int chainbase = lane - slot;
    const int j = slot & 7;
    const Leaf Lf = pairwise_leaf(N, H, slot >> 3);
    const int n = Lf.len;
    const int T = (n >= 8) ? (n >> 3) : 0;
    const int rem = (n >= 8) ? (n & 7) : n;
    const int TC = a.tcount;
    const int TP = (TC + 3) & ~3;
    const int64_t raw = (wave << (6 - lg)) + (lane >> lg);
    const bool valid = raw < a.C;
    const int64_t c = valid ? raw : a.C - 1;

    // the columns of A and the data of every lane slot, staged once per workgroup
    extern __shared__ double lds[];
    double *const sa = lds;                       // [KMAX][TP][G]
    double *const sy = lds + KMAX * TP * G;       // [TP][G]
    __shared__ double zx[GIBBS ? ZIG_C + 1 : 1], zr[GIBBS ? ZIG_C : 1];
    for (int i = threadIdx.x; i < TP * G; i += 256) {
        const int t = i >> lg, sl = i & (G - 1);
        const Leaf L2 = pairwise_leaf(N, H, sl >> 3);
        const int e = 8 * t + (sl & 7);
        const bool m = e < L2.len;
        const int64_t d = L2.off + e;
        sy[i] = m ? a.ys[d] : 0.0;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) sa[k * TP * G + i] = (m && k < K) ? a.xs[(int64_t)k * N + d] : 0.0;
    }
    if (GIBBS && MOVE == POLY_MOVE_HMC && !a.p0 && a.zig) {
        for (int k = threadIdx.x; k <= ZIG_C; k += 256) zx[k] = ZIG_X[k];
        for (int k = threadIdx.x; k < ZIG_C; k += 256) zr[k] = ZIG_RATIO[k];
    }
    __syncthreads();
    // a redundant path of a ragged tree recomputes its leaf for the energy tree but
    // must not count it twice in the force: its force weight is zero
    const double fcanon = Lf.canonical ? 1.0 : 0.0;
    double th[KMAX], p[KMAX], g[KMAX], old[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) th[k] = (k < K) ? a.theta0[c * K + k] : 0.0;
    double tau = a.tau0 ? a.tau0[c] : a.tau;
    double dt = a.dt_chain ? a.dt_chain[c] : a.timestep;

    // rounds t0 .. t0 + R - 1 of this lane: the columns and the mock data (the fixed
    // chain of the contract)
    auto mock_rounds = [&](int t0, double (&col)[KMAX][R], double (&v)[R]) {
        const double *base = sa + t0 * G + slot;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
#pragma unroll
            for (int u = 0; u < R; ++u) col[k][u] = base[(k * TP + u) * G];
        }
#pragma unroll
        for (int u = 0; u < R; ++u) v[u] = col[0][u] * th[0];
#pragma unroll
        for (int k = 1; k < KMAX; ++k) {
#pragma unroll
            for (int u = 0; u < R; ++u) v[u] = __builtin_fma(col[k][u], th[k], v[u]);
        }
    };
    // np.sum((mock - ys)**2)
    auto chi2_of = [&]() {
        LaneSum s = {0.0, 0.0};
        for (int t0 = 0; t0 < TC; t0 += R) {
            double col[KMAX][R], v[R];
            mock_rounds(t0, col, v);
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const double d = v[u] - sy[(t0 + u) * G + slot];
                lane_sum_add<false>(s, d * d, t0 + u, T);
            }
        }
        return 1.0 * chain_sum_finish<false, 0>(s, T, rem, lane, H, Lf.depth);
    };
    // log posterior of theta given tau: the component terms added one after the other in
    // the Posterior's order (posteriors.py:147-151, sorted component names)
    auto log_prob = [&](double chi2, double logZ, bool have_pre, double cpre, bool have_post,
                        double cpost) {
        const double lik = -0.5 * chi2 * tau + logZ;              // likelihoods.py:141-146
        double pri = 0.0;
        if (a.prior_means) {
            auto term = [&](int k) {
                const double d = th[k] - ((k < K) ? a.prior_means[k] : 0.0);
                return d * d / ((k < K) ? a.prior_vars[k] : 1.0);  // priors.py:52-54
            };
            pri = -0.5 * np_sum_k<KMAX>(term, K);
        }
        double total = 0.0;
        bool have = false;
        auto add = [&](double t) {
            total = have ? total + t : t;
            have = true;
        };
        if (have_pre) add(cpre);
        if (a.prior_means && a.prior_first) add(pri);
        add(lik);
        if (a.prior_means && !a.prior_first) add(pri);
        if (have_post) add(cpost);
        return total;
    };
    auto kinetic = [&]() {                                        // hmc.py:148,150
        auto sq = [&](int k) { return p[k] * p[k]; };
        return 0.5 * np_sum_k<KMAX>(sq, K);
    };
    // force[k] = tau * sum_n (mock_n - y_n) A[k][n]              likelihoods.py:148-155
    // tauf = tau for a chain's canonical lanes, 0 on a redundant path of a ragged tree;
    // a round past the lane's data has weight 0 (its column and datum are zeros)
    auto force = [&](double tauf) {
#pragma unroll
        for (int k = 0; k < KMAX; ++k) g[k] = 0.0;
        for (int t0 = 0; t0 < TC; t0 += R) {
            double col[KMAX][R], v[R], r[R];
            mock_rounds(t0, col, v);
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const double m = (8 * (t0 + u) + j < n) ? tauf : 0.0;
                r[u] = (v[u] - sy[(t0 + u) * G + slot]) * m;
            }
            // every g[k] receives its terms in the order t = 0, 1, 2, ...
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
#pragma unroll
                for (int u = 0; u < R; ++u) g[k] = __builtin_fma(col[k][u], r[u], g[k]);
            }
        }
        // all-reduce over the chain's lanes, level by level for all coefficients at once
#pragma unroll
        for (int k = 0; k < KMAX; ++k) g[k] = g[k] + xor1_f64(g[k]);
#pragma unroll
        for (int k = 0; k < KMAX; ++k) g[k] = g[k] + xor2_f64(g[k]);
#pragma unroll
        for (int k = 0; k < KMAX; ++k) g[k] = g[k] + other_quad_f64(g[k]);
        if (lg > 3) {
#pragma unroll
            for (int k = 0; k < KMAX; ++k) g[k] = g[k] + xor8_f64(g[k]);
            if (lg > 4) {
#pragma unroll
                for (int k = 0; k < KMAX; ++k) g[k] = g[k] + xor16_f64(g[k], lane);
            }
            if (lg > 5) {
#pragma unroll
                for (int k = 0; k < KMAX; ++k) g[k] = g[k] + xor32_f64(g[k], lane);
            }
        }
#pragma unroll
        for (int k = 0; k < KMAX; ++k) g[k] = (k < K) ? g[k] : 0.0;
    };
    // K draws of a chain from a paired Philox stream: lane (slot & 7) of the chain computes
    // block (e0 >> 1) + (slot & 7) -- global elements 2b, 2b + 1 -- and the chain's lanes
    // pick element e0 + k from the lane that holds it
    auto gather_pairs = [&](int64_t e0, double va, double vb) {
        const int odd = (int)(e0 & 1);
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            const int s = k + odd;
            const double sel = (s & 1) ? vb : va;
            const double v = shfl_f64(sel, chainbase + ((s >> 1) & 7));
            p[k] = (k < K) ? v : 0.0;
        }
    };

    double chi2 = chi2_of();            // of the current state; carried from sweep to sweep
    int32_t nacc = 0;
    const int64_t gc = a.chain_offset + c;      // global chain index (generated draws)
    const int nsweeps = GIBBS ? a.n : 1;
    for (int i = 0; i < nsweeps; ++i) {
        const double logZ = (double)N * 0.5 * log(tau);           // errormodels: N/2 log tau
        bool have_pre, have_post;
        double cpre = 0.0, cpost = 0.0;
        if (GIBBS) {
            const double gp = a.gp_shape_m1 * log(tau) - tau * a.gp_rate;   // priors.py:23-25
            have_pre = a.gp_where == 1;
            have_post = a.gp_where == 2;
            cpre = cpost = gp;
        } else {
            have_pre = a.lp_pre != nullptr;
            have_post = a.lp_post != nullptr;
            cpre = have_pre ? a.lp_pre[c] : 0.0;
            cpost = have_post ? a.lp_post[c] : 0.0;
        }
        // ---- the draws of this sweep ----------------------------------------------------
        const int64_t ic = (int64_t)i * a.C + c;
        if (a.p0) {
#pragma unroll
            for (int k = 0; k < KMAX; ++k) p[k] = (k < K) ? a.p0[ic * K + k] : 0.0;
        } else if (GIBBS) {
            const int64_t e0 = gc * K;
            const int64_t b = (e0 >> 1) + (slot & 7);
            const uint64_t off = a.off_m + (uint64_t)i * a.stride_m;
            double va, vb;
            if (MOVE == POLY_MOVE_HMC) {                          // hmc.py:146
                if (a.zig) zig_normal_pair(b, a.seed_m, off, zx, zr, va, vb);
                else       normals2(b, a.seed_m, off, va, vb);
            } else {                                              // samplers.py:80-81
                const double low = -a.stepsize;
                const double scale = a.stepsize - low;
                uniforms2(b, a.seed_m, off, va, vb);
                va = low + scale * va;
                vb = low + scale * vb;
            }
            gather_pairs(e0, va, vb);
        }
        double uu;
        if (a.u) uu = a.u[ic];
        else uu = GIBBS ? uniform_elem(gc, a.seed_u, a.off_u + (uint64_t)i * a.stride_u) : 0.0;

        // ---- the move of the coefficients ------------------------------------------------
        bool acc;
        double chi2_new, e_before = 0.0, e_after = 0.0;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) old[k] = th[k];
        if (MOVE == POLY_MOVE_HMC) {
            e_before = -log_prob(chi2, logZ, have_pre, cpre, have_post, cpost) + kinetic();  // hmc.py:148
            const double hdt = 0.5 * dt;
            const double tauf = tau * fcanon;
            // hmc.py:116-123 as ONE loop around the force: half kick, (nsteps - 1) x [drift,
            // kick], drift, half kick
            for (int l = 0; l <= a.nsteps; ++l) {
                force(tauf);
                const double kdt = (l == 0 || l == a.nsteps) ? hdt : dt;
#pragma unroll
                for (int k = 0; k < KMAX; ++k) p[k] = kick<FMA>(p[k], kdt, g[k]);
                if (l < a.nsteps) {
#pragma unroll
                    for (int k = 0; k < KMAX; ++k) th[k] = drift<FMA>(th[k], p[k], dt);
                }
            }
            chi2_new = chi2_of();
            e_after = -log_prob(chi2_new, logZ, have_pre, cpre, have_post, cpost) + kinetic();  // hmc.py:150
            acc = metropolis_accept(uu, -(e_after - e_before));          // hmc.py:151
        } else {
            // E_old = -log_prob(state), proposal = state + change, E_new (samplers.py:78-84);
            // -(E_new - E_old) == lp_new - lp_old bit for bit (rwmc.hip)
            const double lp_old = log_prob(chi2, logZ, have_pre, cpre, have_post, cpost);
#pragma unroll
            for (int k = 0; k < KMAX; ++k) th[k] = (k < K) ? th[k] + p[k] : 0.0;
            chi2_new = chi2_of();
            const double lp_new = log_prob(chi2_new, logZ, have_pre, cpre, have_post, cpost);
            acc = uu < np_exp(lp_new - lp_old);                          // samplers.py:86
        }
        if (GIBBS) {
            // the chain's lanes hold replicas: slot 0 decides (it is the lane whose results
            // a single launch writes out)
            acc = __shfl((int)acc, chainbase, 64) != 0;
        }
#pragma unroll
        for (int k = 0; k < KMAX; ++k) th[k] = acc ? th[k] : old[k];
        chi2 = acc ? chi2_new : chi2;
        nacc += acc ? 1 : 0;
        if (MOVE == POLY_MOVE_HMC && i < a.n_adapt)
            dt = acc ? dt * a.uprate : dt * a.downrate;                   // hmc.py:188-191

        // ---- the conjugate draw of the precision (samplers.py:27-51) -----------------------
        if (GIBBS && !a.keep_tau) {
            // likelihood.log_prob(coefficients, precision=1.0): the error model's epilogue
            // at tau = 1
            const double lp1 = -0.5 * chi2 * 1.0 + (double)N * 0.5 * log(1.0);
            const double rate = -lp1 + a.g_rate;
            const double gv = a.g ? a.g[ic]
                                  : gamma_elem<false>(gc, a.g_shape, a.seed_g,      // shape >= 1
                                                      a.off_g + (uint64_t)i * a.stride_g);
            tau = gv / rate;
            tau = shfl_f64(tau, chainbase);
        }
        if (valid && slot == 0) {
            if (a.accepted) a.accepted[ic] = acc ? 1 : 0;
            if (a.e_before) a.e_before[ic] = e_before;
            if (a.e_after) a.e_after[ic] = e_after;
            if (GIBBS && (i + 1) % a.thin == 0) {
                const int64_t r = (int64_t)((i + 1) / a.thin - 1) * a.C + c;
                if (a.rec_theta) {
#pragma unroll
                    for (int k = 0; k < KMAX; ++k)
                        if (k < K) a.rec_theta[r * K + k] = th[k];
                }
                if (a.rec_tau) a.rec_tau[r] = tau;
            }
        }
    }
    if (!valid || slot != 0) return;
    // theta_out may be theta0 itself: a chain then keeps or replaces its own row
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
        if (k < K) a.theta_out[c * K + k] = th[k];
    if (GIBBS && a.tau_out) a.tau_out[c] = tau;
    if (a.n_accepted && nacc) a.n_accepted[c] += nacc;
    if (a.n_adapt > 0 && a.dt_chain) a.dt_chain[c] = dt;
}

// ---- host side ---------------------------------------------------------------------------
inline int linear_chain_kmax(int32_t K) { return (K + 3) & ~3; }

template <class Kern>
inline hipError_t linear_chain_launch(Kern kern, int kmax, const PolyChainArgs &a, hipStream_t st)
{
    return chain_launch(kern, a, linear_chain_lds_bytes(kmax, a.tcount, a.H), st);
}

}  // namespace binf
