// Replica exchange between neighbouring slots of a tempered ladder, chain-batched.
// Build-defined: the reference has the hooks a replica exchange scheme drives
// (binf/samplers/hmc.py:171-176 last_draw_stats, binf/samplers/gibbs.py:117,143-144
// _update_subsampler_states) and no exchange of its own.
//
// C = n_ladders * R chains; chain c is slot r = c % R of ladder c / R.  A round has a
// parity in {0, 1}: slot r is the LOWER member of the pair (r, r + 1) iff r >= parity,
// (r - parity) is even and r + 1 < R; every other chain is its own partner.  For a pair
// (i, j = i + 1), with lp_own[c] = log p_c(x_c) and lp_sw[c] = log p_c(x_partner(c)),
//
//     delta  = (lp_sw[i] + lp_sw[j]) - (lp_own[i] + lp_own[j])     three roundings, this order
//     accept = u < exp(clip(delta, -308, 709))                     metropolis_accept(u, delta)
//
// Two launches around the pdf's evaluation of the exchanged states: the gather kernel
// (out[c] = x[partner(c)]) and the swap kernel (test, row exchange, flags, counters, walker
// ids).  A chain is served by LPC = 8 .. 256 threads of a workgroup, sized to the row as in
// accept_select_kernel; the groups of BOTH members of a pair evaluate the same test on the
// same five doubles -- the same bits -- so no flag passes between groups and nothing needs a
// second launch.  Rows move with 16-byte accesses where the source and the destination row
// are both 16-byte aligned (an odd D misaligns every second row: those take 8-byte accesses).
// One read and one write of a row per chain: HBM-bound.  gfx950, wave64.
#include "gauss_common.hpp"
#include "philox_draws.hpp"
#include "replica_pairing.hpp"

namespace binf {

struct ReplicaArgs {
    const double *x;
    const double *lp_own;
    const double *lp_sw;
    const double *u;            // null: generated
    double *out;
    uint8_t *accepted;
    int64_t *n_attempted;       // null: not counted
    int64_t *n_accepted;        // null: not counted
    int64_t *walker;            // null: not tracked
    int64_t C;
    int64_t D;
    int64_t R;
    int64_t chain_offset;
    uint64_t seed;
    uint64_t offset;
    int32_t parity;
    int32_t lpc;                // threads per chain (power of two, 8..256)
};

__device__ inline void replica_copy_row(double *dst, const double *src, int64_t D, int sub, int lpc)
{
    if (((((uintptr_t)src) | ((uintptr_t)dst)) & 15) == 0) {
        const int64_t even = D & ~(int64_t)1;
        for (int64_t i = (int64_t)sub * 2; i < even; i += (int64_t)lpc * 2)
            *reinterpret_cast<double2 *>(dst + i) = *reinterpret_cast<const double2 *>(src + i);
        if ((D & 1) && sub == 0) dst[D - 1] = src[D - 1];
    } else {
        for (int64_t i = sub; i < D; i += lpc) dst[i] = src[i];
    }
}

template <bool SWAP>
__global__ void __launch_bounds__(256) replica_kernel(const ReplicaArgs a)
{
    const int lpc = a.lpc;
    const int sub = threadIdx.x & (lpc - 1);
    const int64_t c = (int64_t)blockIdx.x * (256 / lpc) + threadIdx.x / lpc;
    if (c >= a.C) return;
    const int64_t i = replica_pair_lower(c, a.R, a.parity);
    const int64_t partner = i < 0 ? c : (i == c ? c + 1 : i);
    bool acc = !SWAP;
    if (SWAP && i >= 0) {
        const double delta = (a.lp_sw[i] + a.lp_sw[i + 1]) - (a.lp_own[i] + a.lp_own[i + 1]);
        const double uu = a.u ? a.u[i] : uniform_elem(a.chain_offset + i, a.seed, a.offset);
        acc = metropolis_accept(uu, delta);
    }
    replica_copy_row(a.out + c * a.D, a.x + (acc ? partner : c) * a.D, a.D, sub, lpc);
    if (SWAP && sub == 0) {
        a.accepted[c] = acc ? 1 : 0;
        if (i == c) {
            // the lower member's group keeps the pair's books (pairs are disjoint)
            if (a.n_attempted) a.n_attempted[c] += 1;
            if (a.n_accepted && acc) a.n_accepted[c] += 1;
            if (a.walker && acc) {
                const int64_t w = a.walker[c];
                a.walker[c] = a.walker[c + 1];
                a.walker[c + 1] = w;
            }
        }
    }
}

static int32_t replica_launch(bool swap, ReplicaArgs &a, void *stream, const char *what)
{
    if (a.C < 0 || a.D < 0) return fail(BINF_E_ARG, "%s: negative size", what);
    if (a.R < 1) return fail(BINF_E_ARG, "%s: R >= 1 required", what);
    if (a.C % a.R != 0) return fail(BINF_E_ARG, "%s: C is not a multiple of R", what);
    if (a.parity != 0 && a.parity != 1) return fail(BINF_E_ARG, "%s: parity %d outside {0, 1}", what, a.parity);
    if (a.chain_offset < 0 || a.chain_offset % a.R != 0)
        return fail(BINF_E_ARG, "%s: chain_offset must be >= 0 and a multiple of R", what);
    if (a.C == 0) return 0;
    if (a.D > 0 && (!a.x || !a.out)) return fail(BINF_E_ARG, "%s: null buffer", what);
    if (swap && (!a.lp_own || !a.lp_sw || !a.accepted)) return fail(BINF_E_ARG, "%s: null buffer", what);
    if (a.D > 0 && a.C > 0x7fffffffffffffffLL / 8 / a.D) return fail(BINF_E_ARG, "%s: C*D overflows", what);
    if (overlap_f64(a.out, a.C * a.D, a.x, a.C * a.D))
        return fail(BINF_E_ALIAS, "%s: out overlaps x (a partner's row is read after its own "
                    "chain may have been written)", what);
    if (!swap && a.D == 0) return 0;
    const bool vec2 = a.D % 2 == 0 && ((((uintptr_t)a.x) | ((uintptr_t)a.out)) & 15) == 0;
    const int64_t per_thread = vec2 ? 2 : 1;
    int lpc = 8;
    while (lpc < 256 && (int64_t)lpc * per_thread < a.D) lpc <<= 1;
    a.lpc = lpc;
    const int64_t blocks = (a.C + 256 / lpc - 1) / (256 / lpc);
    if (blocks > 0x7fffffffLL) return fail(BINF_E_UNSUPPORTED, "%s: too many chains", what);
    if (swap) replica_kernel<true><<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(a);
    else      replica_kernel<false><<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what);
    return 0;
}

}  // namespace binf

using namespace binf;

extern "C" int32_t binf_replica_gather_f64(const double *x, double *out, int64_t C, int64_t D,
                                           int64_t R, int32_t parity, void *stream)
{
    ReplicaArgs a = {};
    a.x = x; a.out = out; a.C = C; a.D = D; a.R = R; a.parity = parity;
    return replica_launch(false, a, stream, "replica_gather");
}

extern "C" int32_t binf_replica_swap_f64(const double *x, const double *lp_own,
                                         const double *lp_swapped, const double *u, double *out,
                                         uint8_t *accepted, int64_t *n_attempted,
                                         int64_t *n_accepted, int64_t *walker, int64_t C, int64_t D,
                                         int64_t R, int32_t parity, uint64_t seed, uint64_t offset,
                                         int64_t chain_offset, void *stream)
{
    ReplicaArgs a = {};
    a.x = x; a.lp_own = lp_own; a.lp_sw = lp_swapped; a.u = u; a.out = out; a.accepted = accepted;
    a.n_attempted = n_attempted; a.n_accepted = n_accepted; a.walker = walker;
    a.C = C; a.D = D; a.R = R; a.parity = parity; a.seed = seed; a.offset = offset;
    a.chain_offset = chain_offset;
    return replica_launch(true, a, stream, "replica_swap");
}
