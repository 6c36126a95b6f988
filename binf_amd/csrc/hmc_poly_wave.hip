// Fused HMC transition on the example's polynomial posterior, one lane GROUP per
// chain (n_data <= 1024, K <= 16 coefficients): the single-transition instantiations
// of poly_chain_kernel.hpp.  Same entry point as the one-lane-per-chain kernel of
// hmc_poly.hip (binf_hmc_sample_poly_f64), which checks the call; the per-step tier
// with its MFMA gradient takes over where chains x data is large.
#include "poly_chain_kernel.hpp"

namespace binf {

template <int KMAX>
static hipError_t launch_poly_wave_k(const PolyChainArgs &a, bool fma, hipStream_t st)
{
    if (fma) return chain_launch(poly_chain_kernel<KMAX, true, false, POLY_MOVE_HMC>, a, 0, st);
    return chain_launch(poly_chain_kernel<KMAX, false, false, POLY_MOVE_HMC>, a, 0, st);
}

int32_t launch_poly_wave(const PolyChainArgs &a, bool fma, hipStream_t st)
{
    hipError_t e;
    if (a.K <= 4)      e = launch_poly_wave_k<4>(a, fma, st);
    else if (a.K <= 8) e = launch_poly_wave_k<8>(a, fma, st);
    else               e = launch_poly_wave_k<16>(a, fma, st);
    if (e != hipSuccess) return hip_fail(e, "poly_chain_kernel launch");
    return 0;
}

}  // namespace binf
