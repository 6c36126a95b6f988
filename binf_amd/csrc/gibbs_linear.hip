// n sweeps of the Gibbs loop (binf/samplers/gibbs.py:136-151) on a linear forward
// model's posterior in one launch: the multi-sweep instantiations of
// linear_chain_kernel.hpp.  Contract: include/binf_hip.h, binf_gibbs_linear_sample_n_f64.
#include "linear_chain_kernel.hpp"

namespace binf {

template <int KMAX>
static hipError_t launch_gibbs_linear_k(const PolyChainArgs &a, int move, bool fma, hipStream_t st)
{
    if (move == POLY_MOVE_RWMC)
        return linear_chain_launch(linear_chain_kernel<KMAX, false, true, POLY_MOVE_RWMC>, KMAX, a, st);
    if (fma)
        return linear_chain_launch(linear_chain_kernel<KMAX, true, true, POLY_MOVE_HMC>, KMAX, a, st);
    return linear_chain_launch(linear_chain_kernel<KMAX, false, true, POLY_MOVE_HMC>, KMAX, a, st);
}

}  // namespace binf

using namespace binf;

extern "C" int32_t binf_gibbs_linear_sample_n_f64(const binf_gibbs_linear_args *g, void *stream)
{
    const int32_t rc = chain_check_gibbs("gibbs_linear", g);
    if (rc != CHAIN_GO) return rc;
    const PolyChainArgs a = chain_fill_gibbs(*g);
    const bool fma = g->mode == BINF_MODE_FMA;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    switch (linear_chain_kmax(a.K)) {
    case 4:  e = launch_gibbs_linear_k<4>(a, g->move, fma, st); break;
    case 8:  e = launch_gibbs_linear_k<8>(a, g->move, fma, st); break;
    case 12: e = launch_gibbs_linear_k<12>(a, g->move, fma, st); break;
    default: e = launch_gibbs_linear_k<16>(a, g->move, fma, st); break;
    }
    if (e != hipSuccess) return hip_fail(e, "gibbs_linear launch");
    return 0;
}
