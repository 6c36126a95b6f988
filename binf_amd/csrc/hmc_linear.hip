// Fused HMC transition on the posterior of a linear forward model (mock = theta . A,
// Gaussian errors; K <= 16 coefficients, n_data <= 1024), one lane GROUP per chain:
// the single-transition instantiations of linear_chain_kernel.hpp (mapping, LDS image
// of A, summation orders and reference lines are documented there), and the query
// that tells a caller which shapes the resident kernels cover.  Contract:
// include/binf_hip.h, binf_hmc_sample_linear_f64.
#include "linear_chain_kernel.hpp"

namespace binf {

template <int KMAX>
static hipError_t launch_linear_hmc_k(const PolyChainArgs &a, bool fma, hipStream_t st)
{
    if (fma) return linear_chain_launch(linear_chain_kernel<KMAX, true, false, POLY_MOVE_HMC>, KMAX, a, st);
    return linear_chain_launch(linear_chain_kernel<KMAX, false, false, POLY_MOVE_HMC>, KMAX, a, st);
}

}  // namespace binf

using namespace binf;

extern "C" int32_t binf_linear_resident_supported(int64_t K, int64_t N)
{
    return linear_chain_supported(K, N) ? 1 : 0;
}

extern "C" int32_t binf_hmc_sample_linear_f64(
    const double *q0, const double *p0, const double *u, double *q_out,
    uint8_t *accepted, int64_t *n_accepted, double *e_before, double *e_after,
    const double *design, const double *ys, double precision,
    const double *precision_chain, const double *prior_means,
    const double *prior_vars, int32_t prior_first, const double *lp_pre,
    const double *lp_post, double timestep, double *dt_chain, int64_t C,
    int64_t K, int64_t N, int32_t nsteps, int32_t adapt, double uprate,
    double downrate, int32_t mode, void *stream)
{
    if (C < 0 || K < 1 || N < 0 || nsteps < 1)
        return fail(BINF_E_ARG, "hmc_sample_linear: need C>=0, K>=1, N>=0, nsteps>=1");
    if (mode != BINF_MODE_EXACT && mode != BINF_MODE_FMA)
        return fail(BINF_E_ARG, "hmc_sample_linear: unknown mode %d", mode);
    if (!linear_chain_supported(K, N))
        return fail(BINF_E_UNSUPPORTED, "hmc_sample_linear: K=%lld > 16 or n_data=%lld > 1024 (or a pairwise tree deeper than 3) not covered by the resident kernel (use the per-step tier)", (long long)K, (long long)N);
    if (C == 0) return 0;
    if (!q0 || !p0 || !u || !q_out || !accepted || (N > 0 && (!design || !ys)))
        return fail(BINF_E_ARG, "hmc_sample_linear: null buffer");
    if ((prior_means == nullptr) != (prior_vars == nullptr))
        return fail(BINF_E_ARG, "hmc_sample_linear: prior_means and prior_vars go together");
    if (adapt && !dt_chain)
        return fail(BINF_E_ARG, "hmc_sample_linear: adaption needs dt_chain");
    if (C > 0x7fffffffLL * 8)
        return fail(BINF_E_UNSUPPORTED, "hmc_sample_linear: too many chains");
    const int64_t bytes = C * K * (int64_t)sizeof(double);
    const char *qo = (const char *)q_out, *pi = (const char *)p0, *qi = (const char *)q0;
    if ((qo != qi && qo < qi + bytes && qi < qo + bytes) || (qo < pi + bytes && pi < qo + bytes))
        return fail(BINF_E_ALIAS, "hmc_sample_linear: q_out overlaps q0/p0 (only q_out == q0 is allowed)");
    PolyChainArgs a = {};
    a.theta0 = q0; a.tau0 = precision_chain; a.tau = precision; a.theta_out = q_out;
    a.accepted = accepted; a.n_accepted = n_accepted; a.e_before = e_before;
    a.e_after = e_after; a.xs = design; a.ys = ys; a.prior_means = prior_means;
    a.prior_vars = prior_vars; a.lp_pre = lp_pre; a.lp_post = lp_post; a.p0 = p0;
    a.u = u; a.dt_chain = dt_chain; a.timestep = timestep; a.uprate = uprate;
    a.downrate = downrate; a.C = C; a.K = (int32_t)K; a.N = (int32_t)N;
    a.H = pairwise_tree_height(N);
    a.tcount = poly_chain_tcount(a.N, a.H);
    a.nsteps = nsteps; a.n = 1; a.thin = 1; a.n_adapt = adapt ? 1 : 0;
    a.prior_first = prior_first ? 1 : 0;
    const bool fma = (mode == BINF_MODE_FMA);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    switch (linear_chain_kmax(a.K)) {
    case 4:  e = launch_linear_hmc_k<4>(a, fma, st); break;
    case 8:  e = launch_linear_hmc_k<8>(a, fma, st); break;
    case 12: e = launch_linear_hmc_k<12>(a, fma, st); break;
    default: e = launch_linear_hmc_k<16>(a, fma, st); break;
    }
    if (e != hipSuccess) return hip_fail(e, "linear_chain_kernel launch");
    return 0;
}
