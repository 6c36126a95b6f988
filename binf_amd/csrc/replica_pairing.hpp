// The pairing of a swap round of a tempered ladder, shared by the exchange kernels
// (replica.hip) and the work record (free_energy.hip).
//
// C = n_ladders * R chains; chain c is slot r = c % R of ladder c / R.  A round has a
// parity in {0, 1}: slot r is the LOWER member of the pair (r, r + 1) iff r >= parity,
// (r - parity) is even and r + 1 < R; every other chain is its own partner.
#pragma once
#include "common.hpp"

namespace binf {

// the lower member of chain c's pair, or -1 for a chain that has no partner this round
__device__ inline int64_t replica_pair_lower(int64_t c, int64_t R, int64_t parity)
{
    // R <= C (the launcher's checks): 32-bit division whenever the chain index fits
    const int64_t r = c <= 0xffffffffLL ? (int64_t)((uint32_t)c % (uint32_t)R) : c % R;
    if (r >= parity && ((r - parity) & 1) == 0 && r + 1 < R) return c;
    if (r - 1 >= parity && ((r - 1 - parity) & 1) == 0) return c - 1;       // r < R: r - 1 + 1 < R
    return -1;
}

}  // namespace binf
