// The strided record of kept draws that the diagnostics (diagnostics.hip) and the rank
// layer (ranks.hip) read, and its host-side validation.
#pragma once
#include "common.hpp"

namespace binf {

struct DiagDraws {
    const double *x;
    int64_t st, sc;             // element strides of t and c (the inner stride is 1)
    int64_t T, C, D;
    int64_t split, n, M;
    int64_t span;               // doubles from x to one past the last draw read
};

inline bool overlap_bytes(const void *a, int64_t a_bytes, const void *b, int64_t b_bytes)
{
    if (!a || !b || a_bytes <= 0 || b_bytes <= 0) return false;
    const char *pa = (const char *)a, *pb = (const char *)b;
    return pa < pb + b_bytes && pb < pa + a_bytes;
}

inline int32_t diag_draws(const char *what, const double *draws, int64_t stride_t, int64_t stride_c,
                          int64_t stride_i, int64_t T, int64_t C, int64_t D, int32_t split,
                          DiagDraws &d)
{
    if (C < 1 || D < 1) return fail(BINF_E_ARG, "%s: C >= 1 and D >= 1 required", what);
    if (split != 1 && split != 2) return fail(BINF_E_ARG, "%s: split %d outside {1, 2}", what, split);
    if (T < 0 || T / split < 2)
        return fail(BINF_E_ARG, "%s: a segment of n = T / split = %lld draws (n >= 2 required)",
                    what, (long long)(T < 0 ? T : T / split));
    if (stride_i != 1) return fail(BINF_E_ARG, "%s: inner stride %lld (1 required)", what, (long long)stride_i);
    if (C == 1) stride_c = D;                       // never applied: any value is admissible
    if (stride_t < 0 || stride_c < 0) return fail(BINF_E_ARG, "%s: negative stride", what);
    if (!draws) return fail(BINF_E_ARG, "%s: null buffer", what);
    const __int128 lim = (__int128)1 << 60;
    const __int128 row_t = (__int128)(C - 1) * stride_c + D;      // one draw of every chain
    const __int128 row_c = (__int128)(T - 1) * stride_t + D;      // every draw of one chain
    const __int128 span = (__int128)(T - 1) * stride_t + (__int128)(C - 1) * stride_c + D;
    if (span > lim || (__int128)2 * C * D > lim)
        return fail(BINF_E_UNSUPPORTED, "%s: draws span more than 2^60 elements", what);
    const bool draw_major = stride_c >= D && (__int128)stride_t >= row_t;
    const bool chain_major = stride_t >= D && (__int128)stride_c >= row_c;
    if (!draw_major && !chain_major)
        return fail(BINF_E_ARG, "%s: overlapping strides (%lld, %lld, 1) for [%lld x %lld x %lld]", what,
                    (long long)stride_t, (long long)stride_c, (long long)T, (long long)C, (long long)D);
    d.x = draws; d.st = stride_t; d.sc = stride_c; d.T = T; d.C = C; d.D = D;
    d.split = split; d.n = T / split; d.M = (int64_t)split * C; d.span = (int64_t)span;
    return 0;
}

}  // namespace binf
