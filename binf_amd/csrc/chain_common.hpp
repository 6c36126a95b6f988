// What the chain-resident kernels of every model kind share (poly_chain_kernel.hpp: the
// example's polynomial; linear_chain_kernel.hpp: a user's design matrix): the argument
// block, the small device helpers, and the host path of the entry points --
//
//   binf_hmc_sample_poly_f64, binf_hmc_sample_linear_f64          one HMCSampler.sample();
//   binf_gibbs_poly_sample_n_f64, binf_gibbs_linear_sample_n_f64  n sweeps of the Gibbs loop
//
// -- shape limits, rounds per leaf, grid and launch, every refusal before a launch and the
// fill of the argument block.  A kind keeps its KMAX ladder, its LDS size, its limit on the
// number of chains and the words that name its kernels in a refusal.
//
// The sweep itself is written out in each kernel: as ONE device function around a model
// policy it compiled to other machine code (the shared body is optimised once on its own
// and once more inside the kernel), which cost the K = 8 random-walk instantiations their
// second wave per SIMD and 43-58 % at 65536 chains (profiles/r09_c_chain_resources.md, r09_c_chain_speed.md).
// gfx950, wave64.
#pragma once
#include "gauss_common.hpp"
#include "philox_draws.hpp"

namespace binf {

struct PolyChainArgs {
    const double *theta0;      // [C x K]
    const double *tau0;        // [C] or null (then `tau`)
    double tau;
    double *theta_out;         // [C x K]; may be theta0
    double *tau_out;           // [C] (GIBBS) or null
    double *rec_theta;         // [n / thin x C x K] or null
    double *rec_tau;           // [n / thin x C] or null
    uint8_t *accepted;         // [n x C] or null
    int64_t *n_accepted;       // [C] or null
    double *e_before;          // [n x C] or null (HMC move)
    double *e_after;           // [n x C] or null
    const double *xs;          // [N] abscissae (polynomial) / [K x N] design matrix (linear)
    const double *ys;          // [N]
    const double *prior_means; // [K] or null: Gaussian prior on theta (energy only)
    const double *prior_vars;  // [K]
    const double *lp_pre;      // !GIBBS: [C] or null, theta-independent terms added first
    const double *lp_post;     // !GIBBS: ... added last
    const double *p0;          // [n x C x K] momenta (HMC) / proposal steps (RWMC); null: generated
    const double *u;           // [n x C] acceptance draws; null: generated
    const double *g;           // [n x C] Gamma(shape, 1) variates; null: generated
    double *dt_chain;          // [C] or null
    double timestep;
    double uprate;
    double downrate;
    double stepsize;           // RWMC half-width
    double gp_shape_m1;        // GIBBS: the GammaPrior term of the coefficient conditional,
    double gp_rate;            //        (shape - 1) log tau - tau rate (priors.py:23-25)
    double g_shape;            // GIBBS: shape of the conjugate draw (samplers.py:27-32)
    double g_rate;             //        prior rate added to 0.5 chi^2 (samplers.py:34-41)
    int64_t C;
    int64_t chain_offset;      // global index of chain 0 of this launch (generated draws)
    uint64_t seed_m, off_m, stride_m;   // momentum / proposal stream: sweep i at off_m + i stride_m
    uint64_t seed_u, off_u, stride_u;   // acceptance draws
    uint64_t seed_g, off_g, stride_g;   // gamma variates
    int32_t K;
    int32_t N;
    int32_t H;                 // pairwise tree height of N
    int32_t tcount;            // rounds of 8 data points per leaf: ceil(longest leaf / 8)
    int32_t nsteps;
    int32_t n;                 // sweeps (GIBBS) / 1
    int32_t thin;
    int32_t n_adapt;           // the first n_adapt HMC transitions adapt the timestep
    int32_t prior_first;       // the Gaussian prior term precedes the likelihood term
    int32_t gp_where;          // GIBBS: 0 no GammaPrior term, 1 before the theta terms, 2 after
    int32_t zig;               // generated momenta: 1 ziggurat, 0 Box-Muller (rng.hip streams)
    int32_t keep_tau;          // GIBBS: no precision draw (n moves under a fixed precision)
};

constexpr int POLY_MOVE_HMC = 0;
constexpr int POLY_MOVE_RWMC = 1;

// np.sum over K <= KMAX register values (every lane for itself)
template <int KMAX, class F>
__device__ inline double np_sum_k(F f, int K)
{
    double res;
    if (KMAX < 8 || K < 8) {
        res = -0.0;
#pragma unroll
        for (int i = 0; i < (KMAX < 7 ? KMAX : 7); ++i) {
            const double n = res + f(i);
            res = (i < K) ? n : res;
        }
    } else {
        double r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = f(j);
        const int k8 = K & ~7;
#pragma unroll
        for (int i = 8; i < KMAX; ++i) {
            const double n = r[i & 7] + f(i);
            r[i & 7] = (i < k8) ? n : r[i & 7];
        }
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
#pragma unroll
        for (int i = 8; i < KMAX; ++i) {
            const double n = res + f(i);
            res = (i >= k8 && i < K) ? n : res;
        }
    }
    return 0.0 + res;
}

// both outputs of block i of the ziggurat normal stream (rng.hip): elements 2i, 2i + 1
__device__ inline void zig_normal_pair(int64_t i, uint64_t seed, uint64_t offset, const double *zx,
                                       const double *zr, double &a, double &b)
{
    const Philox4 r = zig_block(i, seed, offset, 0);
    int layer;
    double u;
    zig_split(r.v[0], r.v[1], layer, u);
    a = (fabs(u) < zr[layer]) ? u * zx[layer] : zig_slow(r.v[0], r.v[1], zx, zr, i, seed, offset, 0);
    zig_split(r.v[2], r.v[3], layer, u);
    b = (fabs(u) < zr[layer]) ? u * zx[layer] : zig_slow(r.v[2], r.v[3], zx, zr, i, seed, offset, 1);
}

// ---- host side: what the entry points of both kinds share ------------------------------
constexpr int CHAIN_MAX_K = 16;
constexpr int CHAIN_MAX_N = 1024;
constexpr int CHAIN_MAX_H = 3;

// do the chain-resident kernels cover this shape?
inline bool chain_supported(int64_t K, int64_t N)
{
    return K >= 1 && K <= CHAIN_MAX_K && N >= 0 && N <= CHAIN_MAX_N &&
           pairwise_tree_height(N) <= CHAIN_MAX_H;
}

// rounds of 8 data points of the longest leaf (at least one)
inline int32_t poly_chain_tcount(int32_t N, int32_t H)
{
    int32_t longest = 0;
    for (int32_t g = 0; g < (1 << H); ++g) {
        const Leaf L = pairwise_leaf(N, H, g);
        if (L.len > longest) longest = L.len;
    }
    const int32_t tc = (longest + 7) / 8;
    return tc < 1 ? 1 : tc;
}

// grid from (C, H), `lds` bytes of dynamic LDS (raised above the default limit where a
// kernel needs more) and launch
template <class Kern>
inline hipError_t chain_launch(Kern kern, const PolyChainArgs &a, size_t lds, hipStream_t st)
{
    const int64_t chains_per_wave = 64 >> (3 + a.H);
    const int64_t waves = (a.C + chains_per_wave - 1) / chains_per_wave;
    const dim3 grid((unsigned)((waves + 3) / 4));
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void *)kern,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)lds);
        if (e != hipSuccess) return e;
    }
    kern<<<grid, 256, lds, st>>>(a);
    return hipGetLastError();
}

// what a check answers besides a refusal (< 0) and "nothing to do" (0)
constexpr int32_t CHAIN_GO = 1;

// the two Gibbs argument blocks are field for field the same, but for the name of this one
inline const double *chain_design(const binf_gibbs_poly_args &g) { return g.xs; }
inline const double *chain_design(const binf_gibbs_linear_args &g) { return g.design; }

// every refusal of binf_gibbs_{poly,linear}_sample_n_f64, before any launch
template <class G>
inline int32_t chain_check_gibbs(const char *what, const G *g)
{
    if (!g) return fail(BINF_E_ARG, "%s: null argument block", what);
    if (g->struct_size != sizeof(G))
        return fail(BINF_E_ARG, "%s: struct_size %llu, this library expects %llu", what,
                    (unsigned long long)g->struct_size, (unsigned long long)sizeof(G));
    const int64_t C = g->C, K = g->K, N = g->N;
    if (C < 0 || K < 1 || N < 0 || g->n < 1 || g->thin < 1 || g->chain_offset < 0 || g->n_adapt < 0)
        return fail(BINF_E_ARG, "%s: need C>=0, K>=1, N>=0, n>=1, thin>=1, chain_offset>=0", what);
    if (g->move != BINF_MOVE_HMC && g->move != BINF_MOVE_RWMC)
        return fail(BINF_E_ARG, "%s: unknown move %d", what, g->move);
    if (g->mode != BINF_MODE_EXACT && g->mode != BINF_MODE_FMA)
        return fail(BINF_E_ARG, "%s: unknown mode %d", what, g->mode);
    if (g->move == BINF_MOVE_HMC && g->nsteps < 1)
        return fail(BINF_E_ARG, "%s: nsteps >= 1 required", what);
    if (g->gp_where < 0 || g->gp_where > 2)
        return fail(BINF_E_ARG, "%s: gp_where must be 0, 1 or 2", what);
    if (!g->keep_precision && !(g->gamma_shape > 0.0))
        return fail(BINF_E_ARG, "%s: gamma_shape must be > 0", what);
    if (!g->keep_precision && !g->g && g->gamma_shape < 1.0)
        return fail(BINF_E_UNSUPPORTED, "%s: generated gamma variates need gamma_shape >= 1 (got %g): supply g or sweep one at a time", what, g->gamma_shape);
    if (!chain_supported(K, N))
        return fail(BINF_E_UNSUPPORTED, "%s: K=%lld > 16 or n_data=%lld > 1024 (or a pairwise tree deeper than 3) not covered (sweep with the per-step tier)", what, (long long)K, (long long)N);
    if (C == 0) return 0;
    if (!g->coefficients || !g->precision || !g->coefficients_out || !g->precision_out ||
        (N > 0 && (!chain_design(*g) || !g->ys)))
        return fail(BINF_E_ARG, "%s: null buffer", what);
    if ((g->prior_means == nullptr) != (g->prior_vars == nullptr))
        return fail(BINF_E_ARG, "%s: prior_means and prior_vars go together", what);
    if (g->n_adapt > 0 && !g->dt_chain)
        return fail(BINF_E_ARG, "%s: adaption needs dt_chain", what);
    if (g->move == BINF_MOVE_HMC && !g->p0 && g->zig &&
        ((g->off_m + (uint64_t)(g->n - 1) * g->stride_m) >> 48))
        return fail(BINF_E_ARG, "%s: ziggurat stream offsets must stay < 2^48", what);
    const int64_t waves_needed = (C + 7) / 8;
    if (waves_needed / 4 > 0x7ffffff0LL) return fail(BINF_E_UNSUPPORTED, "%s: too many chains", what);
    if ((g->coefficients_out != g->coefficients && overlap_f64(g->coefficients_out, C * K, g->coefficients, C * K)) ||
        (g->precision_out != g->precision && overlap_f64(g->precision_out, C, g->precision, C)) ||
        overlap_f64(g->coefficients_out, C * K, g->precision, C) || overlap_f64(g->precision_out, C, g->coefficients, C * K))
        return fail(BINF_E_ALIAS, "%s: outputs may be exactly their inputs, not a partial overlap", what);
    return CHAIN_GO;
}

template <class G>
inline PolyChainArgs chain_fill_gibbs(const G &g)
{
    PolyChainArgs a = {};
    a.theta0 = g.coefficients; a.tau0 = g.precision; a.theta_out = g.coefficients_out;
    a.tau_out = g.precision_out; a.rec_theta = g.rec_coefficients; a.rec_tau = g.rec_precision;
    a.accepted = g.accepted; a.n_accepted = g.n_accepted; a.e_before = g.e_before;
    a.e_after = g.e_after; a.xs = chain_design(g); a.ys = g.ys; a.prior_means = g.prior_means;
    a.prior_vars = g.prior_vars; a.p0 = g.p0; a.u = g.u; a.g = g.g; a.dt_chain = g.dt_chain;
    a.timestep = g.timestep; a.uprate = g.uprate; a.downrate = g.downrate;
    a.stepsize = g.stepsize; a.gp_shape_m1 = g.gp_shape - 1.0; a.gp_rate = g.gp_rate;
    a.g_shape = g.gamma_shape; a.g_rate = g.gamma_rate; a.C = g.C; a.chain_offset = g.chain_offset;
    a.seed_m = g.seed_m; a.off_m = g.off_m; a.stride_m = g.stride_m;
    a.seed_u = g.seed_u; a.off_u = g.off_u; a.stride_u = g.stride_u;
    a.seed_g = g.seed_g; a.off_g = g.off_g; a.stride_g = g.stride_g;
    a.K = (int32_t)g.K; a.N = (int32_t)g.N; a.H = pairwise_tree_height(g.N);
    a.tcount = poly_chain_tcount(a.N, a.H);
    a.nsteps = g.nsteps; a.n = g.n; a.thin = g.thin;
    a.n_adapt = g.move == BINF_MOVE_HMC ? g.n_adapt : 0;
    a.prior_first = g.prior_first ? 1 : 0; a.gp_where = g.gp_where; a.zig = g.zig ? 1 : 0;
    a.keep_tau = g.keep_precision ? 1 : 0;
    return a;
}

// the arguments of binf_hmc_sample_{poly,linear}_f64, in their order
struct ChainHmcCall {
    const double *q0, *p0, *u;
    double *q_out;
    uint8_t *accepted;
    int64_t *n_accepted;
    double *e_before, *e_after;
    const double *xs, *ys;     // xs: the abscissae / the design matrix
    double precision;
    const double *precision_chain, *prior_means, *prior_vars;
    int32_t prior_first;
    const double *lp_pre, *lp_post;
    double timestep;
    double *dt_chain;
    int64_t C, K, N;
    int32_t nsteps, adapt;
    double uprate, downrate;
    int32_t mode;              // BINF_MODE_LANE_PER_CHAIN taken out into the next field
    bool lane_per_chain;       // polynomial only
};

// every refusal of a single transition, before any launch.  `covered_by` names the kernels
// in the refusal of a shape, `max_chains` is the kind's limit.
inline int32_t chain_check_hmc(const char *what, const ChainHmcCall &h, const char *covered_by,
                               int64_t max_chains)
{
    const int64_t C = h.C, K = h.K, N = h.N;
    if (C < 0 || K < 1 || N < 0 || h.nsteps < 1)
        return fail(BINF_E_ARG, "%s: need C>=0, K>=1, N>=0, nsteps>=1", what);
    if (h.mode != BINF_MODE_EXACT && h.mode != BINF_MODE_FMA)
        return fail(BINF_E_ARG, "%s: unknown mode %d", what, h.mode);
    if (!chain_supported(K, N))
        return fail(BINF_E_UNSUPPORTED, "%s: K=%lld > 16 or n_data=%lld > 1024 (or a pairwise tree deeper than 3) not covered by %s (use the per-step tier)", what, (long long)K, (long long)N, covered_by);
    if (h.lane_per_chain && N > 128)
        return fail(BINF_E_UNSUPPORTED, "%s: one lane per chain covers n_data <= 128, not %lld", what, (long long)N);
    if (C == 0) return 0;
    if (!h.q0 || !h.p0 || !h.u || !h.q_out || !h.accepted || (N > 0 && (!h.xs || !h.ys)))
        return fail(BINF_E_ARG, "%s: null buffer", what);
    if ((h.prior_means == nullptr) != (h.prior_vars == nullptr))
        return fail(BINF_E_ARG, "%s: prior_means and prior_vars go together", what);
    if (h.adapt && !h.dt_chain)
        return fail(BINF_E_ARG, "%s: adaption needs dt_chain", what);
    if (C > max_chains)
        return fail(BINF_E_UNSUPPORTED, "%s: too many chains", what);
    if ((h.q_out != h.q0 && overlap_f64(h.q_out, C * K, h.q0, C * K)) || overlap_f64(h.q_out, C * K, h.p0, C * K))
        return fail(BINF_E_ALIAS, "%s: q_out overlaps q0/p0 (only q_out == q0 is allowed)", what);
    return CHAIN_GO;
}

inline PolyChainArgs chain_fill_hmc(const ChainHmcCall &h)
{
    PolyChainArgs a = {};
    a.theta0 = h.q0; a.tau0 = h.precision_chain; a.tau = h.precision; a.theta_out = h.q_out;
    a.accepted = h.accepted; a.n_accepted = h.n_accepted; a.e_before = h.e_before;
    a.e_after = h.e_after; a.xs = h.xs; a.ys = h.ys; a.prior_means = h.prior_means;
    a.prior_vars = h.prior_vars; a.lp_pre = h.lp_pre; a.lp_post = h.lp_post; a.p0 = h.p0;
    a.u = h.u; a.dt_chain = h.dt_chain; a.timestep = h.timestep; a.uprate = h.uprate;
    a.downrate = h.downrate; a.C = h.C; a.K = (int32_t)h.K; a.N = (int32_t)h.N;
    a.H = pairwise_tree_height(h.N);
    a.tcount = poly_chain_tcount(a.N, a.H);
    a.nsteps = h.nsteps; a.n = 1; a.thin = 1; a.n_adapt = h.adapt ? 1 : 0;
    a.prior_first = h.prior_first ? 1 : 0;
    return a;
}

}  // namespace binf
