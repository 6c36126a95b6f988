// n sweeps of the example's Gibbs loop (example_script.py:33-34 around
// binf/samplers/gibbs.py:136-151) in one launch: the multi-sweep instantiations of
// poly_chain_kernel.hpp.  Contract: include/binf_hip.h, binf_gibbs_poly_sample_n_f64.
#include "poly_chain_kernel.hpp"

namespace binf {

template <int KMAX>
static hipError_t launch_gibbs_k(const PolyChainArgs &a, int move, bool fma, hipStream_t st)
{
    if (move == POLY_MOVE_RWMC)
        return chain_launch(poly_chain_kernel<KMAX, false, true, POLY_MOVE_RWMC>, a, 0, st);
    if (fma)
        return chain_launch(poly_chain_kernel<KMAX, true, true, POLY_MOVE_HMC>, a, 0, st);
    return chain_launch(poly_chain_kernel<KMAX, false, true, POLY_MOVE_HMC>, a, 0, st);
}

}  // namespace binf

using namespace binf;

extern "C" int32_t binf_gibbs_poly_sample_n_f64(const binf_gibbs_poly_args *g, void *stream)
{
    const int32_t rc = chain_check_gibbs("gibbs_poly", g);
    if (rc != CHAIN_GO) return rc;
    const PolyChainArgs a = chain_fill_gibbs(*g);
    const bool fma = g->mode == BINF_MODE_FMA;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    if (a.K <= 4)      e = launch_gibbs_k<4>(a, g->move, fma, st);
    else if (a.K <= 8) e = launch_gibbs_k<8>(a, g->move, fma, st);
    else               e = launch_gibbs_k<16>(a, g->move, fma, st);
    if (e != hipSuccess) return hip_fail(e, "gibbs_poly launch");
    return 0;
}
