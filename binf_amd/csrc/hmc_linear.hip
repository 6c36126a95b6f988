// Fused HMC transition on the posterior of a linear forward model (mock = theta . A,
// Gaussian errors; K <= 16 coefficients, n_data <= 1024), one lane GROUP per chain:
// the single-transition instantiations of linear_chain_kernel.hpp, and the query that
// tells a caller which shapes the resident kernels cover.  Contract:
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
    return chain_supported(K, N) ? 1 : 0;
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
    const ChainHmcCall h = {q0, p0, u, q_out, accepted, n_accepted, e_before, e_after, design, ys,
                            precision, precision_chain, prior_means, prior_vars, prior_first, lp_pre,
                            lp_post, timestep, dt_chain, C, K, N, nsteps, adapt, uprate, downrate,
                            mode, false};
    const int32_t rc = chain_check_hmc("hmc_sample_linear", h, "the resident kernel", 0x7fffffffLL * 8);
    if (rc != CHAIN_GO) return rc;
    const PolyChainArgs a = chain_fill_hmc(h);
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
