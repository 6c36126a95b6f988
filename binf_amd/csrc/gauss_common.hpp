// Device helpers shared by the fused Gaussian HMC kernels (single-transition
// and persistent multi-transition).  gfx950, wave64.
#pragma once
#include "common.hpp"

namespace binf {

// Arguments of the fused Gaussian HMC kernels (hmc_gauss.hip, hmc_gauss_split.hip)
struct GaussNArgs {
    const double *q0;
    const double *p0;        // [n x C x D]
    const double *u;         // [n x C]
    double *q_out;           // [C x D]
    double *samples;         // [n/thin x C x D] or null
    uint8_t *accepted;       // [n x C] or null
    int64_t *n_accepted;     // [C] or null
    double *e_before;        // [n x C] or null
    double *e_after;         // [n x C] or null
    double *dt_chain;        // [C] or null
    double timestep;
    double k;
    double x0;
    double uprate;
    double downrate;
    int64_t C;
    int32_t D;
    int32_t nsteps;
    int32_t H;
    int32_t n;               // transitions per launch
    int32_t thin;            // record every thin-th state (>= 1)
    int32_t n_adapt;         // the first n_adapt transitions adapt the timestep
    // draws generated in the kernel (hmc_gauss_rng.hip)
    uint64_t rng_seed;
    uint64_t rng_offset;
    int64_t chain_offset;    // global index of this launch's first chain (sharded runs)
    double *p_dump;          // [n x C x D], GAUSS_RNG_DUMP only
    double *u_dump;          // [n x C],     GAUSS_RNG_DUMP only
    // 0.5 * timestep and -0.5 * k, formed on the host (gauss_derived_args): a kernel argument
    // stays in scalar registers, a product formed on the VALU does not.  Last, so that no
    // other field moves: the kernels that do not read them compile as before.
    double half_timestep;
    double c_lp;
    // ONESUM (hmc_gauss_kernel.hpp): dH = c_dh (sum q'^2 - sum q^2), c_dh = k^2 dt^2 / 8, and
    // the factor of its delta, gauss_onesum_factor(nsteps).  Read by the ONESUM kernels only.
    double c_dh;
    double f_dh;
};

// delta of the ONESUM decision: f(L) (2 Eb~ + |x~|), f(L) = (128 + 32 L) 2^-53.
//
// The unit Gaussian (k = 1, x0 = 0), step h = dt with 2^-256 <= h and k h^2 <= 1, one element:
// half kick, L - 1 times (drift, kick), drift, half kick.  Write z = (q, r) for the position and
// the half-step momentum after a kick and J(z) = r^2 + h q r + q^2.  In exact arithmetic
//   * drift-then-kick M: (q, r) -> (q', r - h q'), q' = q + h r, keeps J (expand it);
//   * J(q, p - h q / 2) = I(q, p) = p^2 + (1 - h^2 / 4) q^2: the start is J(z0) = I(q0, p0), and
//     the last drift and half kick F: (q, r) -> (q', r - h q' / 2) give I(F z) = J(z);
//   * so I(q', p') = I(q0, p0), i.e. dH = (q'^2 + p'^2) / 2 - (q0^2 + p0^2) / 2 = (h^2 / 8) (q'^2 - q0^2),
//     and summed over the chain dH = c (Sq' - Sq0), c = k^2 h^2 / 8 -- no momentum in it.
// For |h| <= 1 both forms are norms: (q^2 + r^2) / 2 <= J <= 3 (q^2 + r^2) / 2 and
// 3 (q^2 + p^2) / 4 <= I <= q^2 + p^2.  Roundings, w = 2^-53, n = sqrt(q^2 + r^2) <= sqrt(2 J):
//   * a step in EXACT mode rounds h r, q + ., h q', r - . (4 roundings; FMA mode rounds only the
//     two sums, a subset of the same terms).  |q' error| <= w (1 + w) (h |r| + |q + h r|) <= 2.42 w n;
//     the kick inherits h times that and adds w (1 + w) (h |q'| + |r - h q'|) <= 3.83 w n (1 + 3 w).
//     The step's error vector e has Euclidean length <= 6.7 w n and sqrt(J(e)) <= sqrt(3/2) 6.7 w n
//     <= 11.6 w sqrt(J(z)): computed z' = M z + e with | sqrt J(z') - sqrt J(z) | <= 12 w sqrt J(z);
//   * the first half kick: error <= w (1 + w) (|q0| / 2 + |r|), 2 w sqrt J(z0) in the J norm;
//   * the last drift and half kick, in the I norm (<= Euclidean): 6.2 w sqrt J(z) by the same
//     count, taken as one more step of 12 w.
//   So sqrt I(q', p') = sqrt I(q0, p0) (1 + t), |t| <= (2 + 12 L) w (1 + 12 L w), and with
//   I(q0, p0) <= q0^2 + p0^2, summed: | dH* - X* | <= (4 + 24 L) w Eb* (1 + 13 L w), where dH* and
//   X* = c (Sq' - Sq0) are formed in exact arithmetic from the float64 end points q', p' of the
//   trajectory as the kernels compute it (numpy's p' included) and Eb* is the exact start energy.
//   * numpy's side, as in the derivation above accept_decide below: each energy within g24 of the exact one, the
//     subtraction rounded once: | xe + dH* | <= 25 w (1 + 25 w) (Eb* + Ea*), and Ea* <= Eb* + |dH*|;
//   * this side: the fused sums are within g22 of the exact ones (by depth, whichever elements
//     a lane holds: see above accept_decide), and c Sq <= h^2 E / 4 <= E / 4:
//     5.5 w (Eb* + Ea*); c_dh = ((k h) (k h)) / 8 carries at most 2 roundings, the subtraction
//     and the product one each: 4 w |X*| more.  | x~ + X* | <= 6 w (2 Eb* + |dH*|) + 4 w |X*|;
//   * forming x~ - delta and x~ + delta in accept_decide: w (|x~| + delta) each.
// Sum, with |dH*| and |X*| within (4 + 24 L) w Eb* + 10 w |x~| of |x~| and Eb* <= Eb~ (1 + 25 w):
//   | x~ - xe | <= [ (66 + 24 L) Eb~ + 36 |x~| ] w (1 + 14 L w).
// accept_decide needs | x~ - xe | <= delta / 2 = (f / 2) (2 Eb~ + |x~|): f >= (66 + 24 L) w and
// f >= 72 w do, and f(L) = (128 + 32 L) w leaves a quarter for the second-order terms (L w < 2^-38
// in the domain below), the three roundings of forming delta itself and those of f (none: it is
// an exact double for L < 2^40).  One f serves both modes.
// Overflow and non-finite values make Spb~, Sq~ or x~ infinite or NaN: delta is then no number
// <= 2^-21 or x~ is not finite, and accept_decide sends the transition to the exact sums.
// Subnormal products (h r, h q', the squares, c_dh times the difference) are absolute errors
// of 2^-1075 each: a decision is only taken with delta <= 2^-21, i.e. Eb~ < 2^25 and every |q|,
// |p| < 2^13, where D (2 L + 6) such errors move x~ - xe by less than 2^-1000 -- against
// accept_decide's margin of 2^-40, of which its own derivation uses 2^-49.
// Not for a non-unit Gaussian: with x0 != 0 the roundings of a step scale with |q|, not with
// |q - x0|, and no bound in Eb alone holds.
inline double gauss_onesum_factor(int32_t nsteps)
{
    return 0x1p-46 + (double)nsteps * 0x1p-48;
}

// Where the ONESUM kernel may be launched for a unit Gaussian with a batch-wide step: the
// derivation's condition on the step (k = 1: 2^-256 <= dt and k dt^2 <= 1; false for a NaN), and
// L small enough that a chain of ordinary energy (2 Eb ~ D + D <= 2^12 at D = 1024) can be
// decided at all, f(L) 2^12 <= 2^-21 (accept_decide's cap on delta): L <= 32764.
inline bool gauss_onesum_domain(const GaussNArgs &a)
{
    return a.timestep >= 0x1p-256 && a.k * a.timestep * a.timestep <= 1.0 && a.nsteps >= 1 &&
           gauss_onesum_factor(a.nsteps) * 0x1p12 <= 0x1p-21;
}

// Halving is exact, so these are the bits the kernels used to form themselves.
inline void gauss_derived_args(GaussNArgs &a)
{
    a.half_timestep = 0.5 * a.timestep;
    a.c_lp = -0.5 * a.k;
    a.c_dh = ((a.k * a.timestep) * (a.k * a.timestep)) * 0.125;
    a.f_dh = gauss_onesum_factor(a.nsteps);
}

// How a [C x D] batch maps onto waves (host side; shared by the launchers)
struct GaussPlan {
    int32_t H;        // height of numpy's pairwise tree for length D
    int LW;           // log2(waves per chain)
    int tneed;        // elements per lane
    bool regular;     // all leaves equal, full depth, multiples of 8
    int64_t blocks;   // workgroups of the one-wave-per-chain / wide kernels
};

inline GaussPlan gauss_plan(int64_t C, int64_t D)
{
    GaussPlan p;
    p.H = pairwise_tree_height(D);
    p.LW = p.H > 3 ? p.H - 3 : 0;
    p.tneed = 1;
    p.regular = true;
    int32_t len0 = -1;
    for (int g = 0; g < (1 << p.H); ++g) {
        Leaf L = pairwise_leaf((int32_t)D, p.H, g);
        int tn = (L.len + 7) / 8;
        if (tn > p.tneed) p.tneed = tn;
        if (len0 < 0) len0 = L.len;
        if (L.len != len0 || L.depth != p.H || (L.len & 7)) p.regular = false;
    }
    if (p.LW == 0) {
        const int64_t chains_per_wave = 64 >> (3 + p.H);
        const int64_t waves = (C + chains_per_wave - 1) / chains_per_wave;
        p.blocks = (waves + 3) / 4;
    } else {
        const int64_t chains_per_block = (p.LW == 3 ? 8 : 4) >> p.LW;
        p.blocks = (C + chains_per_block - 1) / chains_per_block;
    }
    return p;
}

// hmc_gauss_split.hip: few chains of D in {768, 1024} spread over 2 / 4 waves each
int gauss_split_factor(int64_t C, int32_t H, bool regular, int tneed);
hipError_t launch_gauss_split(const GaussNArgs &a, int tneed, int split, bool unit, bool fma,
                              hipStream_t st);

// In-lane part of np.sum: numpy's j-th accumulator of a leaf adds a[8t+j] for
// t = 0..T-1 in order; element t == T (if the lane has one) is a tail element
// and is added after the leaf's accumulators have been combined.
struct LaneSum {
    double r;
    double tail;
};

template <bool REGULAR>
__device__ inline void lane_sum_add(LaneSum &s, double v, int t, int T)
{
    if (REGULAR) {
        s.r = (t == 0) ? v : s.r + v;
    } else {
        const double n = s.r + v;
        s.r = (t == 0) ? v : ((t < T) ? n : s.r);
        s.tail = (t == T) ? v : s.tail;
    }
}

// The same running sum of squares with ONE rounding per element, acc = fma(x, x, acc): what a
// FASTSUM kernel decides its accepts from (accept_decide).  Not numpy's bits: numpy rounds the
// square and the addition separately.  Regular leaves only.
__device__ inline void lane_sum_fused(LaneSum &s, double x, int t)
{
    s.r = (t == 0) ? x * x : __builtin_fma(x, x, s.r);
}

// Cross-lane part of np.sum.  All lanes of the wave must call this (the
// shuffles need a full exec mask).  LW = log2(waves per chain): levels 0..2 of
// the leaf tree live inside a wave (xor-shuffles 8, 16, 32), levels >= 3 join
// the waves of a chain through the LDS slots `xch` (one per wave of the
// block; every wave of the block must call this the same number of times).
template <bool REGULAR, int LW = 0>
__device__ inline double chain_sum_finish(const LaneSum &s, int T, int rem,
                                          int lane, int H, int leafdepth,
                                          double *xch = nullptr, int wib = 0)
{
    // ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7))
    const double r = sum8_f64(s.r);
    double res = r;
    if (!REGULAR) {
        // n < 8: no accumulators, numpy starts from -0.0 and adds in order
        res = (T > 0) ? r : -0.0;
        const int leafbase = lane & ~7;
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            const double v = shfl_f64(s.tail, leafbase + i);
            const double n = res + v;
            res = (i < rem) ? n : res;
        }
    }
    // join the leaves: level l combines the two depth-(H-l) subtrees
    const int hin = (LW > 0) ? 3 : H;
    for (int l = 0; l < hin; ++l) {
        const double o = xor_level_f64(res, l, lane);
        const double n = res + o;
        res = (leafdepth >= H - l) ? n : res;
    }
    if (LW > 0) {
#pragma unroll
        for (int l = 3; l < 3 + LW; ++l) {
            __syncthreads();
            if (lane == 0) xch[wib] = res;
            __syncthreads();
            const double o = xch[wib ^ (1 << (l - 3))];
            const double n = res + o;
            res = (leafdepth >= H - l) ? n : res;
        }
    }
    return 0.0 + res;   // np.add.reduce starts from the identity +0.0
}

// chain_sum_finish of N independent sums of a regular one-wave chain whose tree
// height H is a compile-time constant (every leaf at depth H, T = TMAX, no tail):
// the same additions in the same order -- sum8_f64, the xor levels 8/16/32 up to
// H, then 0.0 + res -- with the levels unrolled and no selects on the leaf
// depth.  The N sums go up the tree level by level together, so that each
// level's shuffles and adds are N independent chains instead of one.
template <int H, int N>
__device__ inline void chain_sum_finish_fixed(double (&v)[N], int lane)
{
    static_assert(H >= 0 && H <= 3, "one-wave chains: at most 8 leaves");
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = v[i] + xor1_f64(v[i]);
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = v[i] + xor2_f64(v[i]);
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = v[i] + other_quad_f64(v[i]);
#pragma unroll
    for (int l = 0; l < H; ++l) {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = v[i] + xor_level_f64(v[i], l, lane);
    }
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = 0.0 + v[i];
}

// ---- shared trees: several sums in one register pair ----------------------------------
// IEEE addition is commutative bit for bit, so the two lanes that a level joins need not
// both compute own + other, and two different sums A and B can share one exchange: the
// lanes of one half (banks BANKS_A of each row of 16) keep their A and fetch the partner's
// A, the others keep their B and fetch the partner's B, and ONE add yields A's next level
// in the first half and B's in the second -- the same additions between the same operands
// as `v + partner(v)` on each sum alone.  CTRL is the DPP control that reaches the partner:
// row_half_mirror (0x141) with banks 0x5 for the xor-4 level, row_ror:8 (0x128) with banks
// 0x3 for the xor-8 level.
template <int CTRL, int BANKS_A>
__device__ inline double pair_level_f64(double a, double b)
{
    constexpr int BANKS_B = 0xf & ~BANKS_A;
    const int alo = __double2loint(a), ahi = __double2hiint(a);
    const int blo = __double2loint(b), bhi = __double2hiint(b);
    // t: own A | partner's B;  u: partner's A | own B
    const int tlo = __builtin_amdgcn_update_dpp(alo, blo, CTRL, 0xf, BANKS_B, false);
    const int thi = __builtin_amdgcn_update_dpp(ahi, bhi, CTRL, 0xf, BANKS_B, false);
    const int ulo = __builtin_amdgcn_update_dpp(blo, alo, CTRL, 0xf, BANKS_A, false);
    const int uhi = __builtin_amdgcn_update_dpp(bhi, ahi, CTRL, 0xf, BANKS_A, false);
    return __hiloint2double(thi, tlo) + __hiloint2double(uhi, ulo);
}
__device__ inline double pair_xor4_f64(double a, double b) { return pair_level_f64<0x141, 0x5>(a, b); }
__device__ inline double pair_xor8_f64(double a, double b) { return pair_level_f64<0x128, 0x3>(a, b); }

// v + partner(v) across the xor-16 / xor-32 exchange without a select: swapping a copy
// of v with v leaves the even rows' (lower half's) values in one register and the odd
// rows' (upper half's) in the other, in EVERY lane, so every lane adds even + odd.
__device__ inline double sum_xor16_f64(double v)
{
    const int lo = __double2loint(v), hi = __double2hiint(v);
    const auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    const auto b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    return __hiloint2double((int)b[0], (int)a[0]) + __hiloint2double((int)b[1], (int)a[1]);
}
__device__ inline double sum_xor32_f64(double v)
{
    const int lo = __double2loint(v), hi = __double2hiint(v);
    const auto a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    const auto b = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    return __hiloint2double((int)b[0], (int)a[0]) + __hiloint2double((int)b[1], (int)a[1]);
}

// lane L's value as a wave-uniform (scalar) double
template <int L>
__device__ inline double lane_value_f64(double v)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), L),
                            __builtin_amdgcn_readlane(__double2loint(v), L));
}

// The energy sums of one transition of a regular chain that fills its wave (H = 3), up
// ONE tree: np.sum's additions for each sum as in chain_sum_finish_fixed<3, .>, with the
// sums joined pairwise on the way up (pair_level_f64), so that a single register pair
// climbs the xor-16 and xor-32 levels.  a, b, c are the lanes' accumulators of three
// sums; d is a fourth one that is only summed when FOUR (the start state's, on the first
// transition of a launch).  Returns a register whose lanes 0 / 4 / 8 / 12 hold the
// finished sums of a / b / c / d (lane 12: c again without FOUR).
__device__ inline double chain_sums_shared(double a, double b, double c, double d, bool four)
{
    a = a + xor1_f64(a);
    b = b + xor1_f64(b);
    c = c + xor1_f64(c);
    a = a + xor2_f64(a);
    b = b + xor2_f64(b);
    c = c + xor2_f64(c);
    if (four) {
        d = d + xor1_f64(d);
        d = d + xor2_f64(d);
        c = pair_xor4_f64(c, d);                  // lane bit 2: 0 -> c, 1 -> d
    } else {
        c = c + other_quad_f64(c);
    }
    double r = pair_xor4_f64(a, b);               // lane bit 2: 0 -> a, 1 -> b
    r = pair_xor8_f64(r, c);                      // lane bit 3: 0 -> a | b, 1 -> c | d
    r = sum_xor16_f64(r);
    r = sum_xor32_f64(r);
    return 0.0 + r;   // np.add.reduce starts from the identity +0.0
}

// The same tree for the kernel that decides from two sums (ONESUM): a, b and, when THREE (the
// first transition of a launch), the start state's d.  Lanes 0 / 4 / 8 hold the finished sums
// of a / b / d (lane 8: a again without THREE).  Without THREE nothing shares the xor-8 level
// and it is the plain exchange: two exchanges and an add, where the pair costs four and one.
__device__ inline double chain_sums_shared2(double a, double b, double d, bool three)
{
    a = a + xor1_f64(a);
    b = b + xor1_f64(b);
    a = a + xor2_f64(a);
    b = b + xor2_f64(b);
    double r = pair_xor4_f64(a, b);               // lane bit 2: 0 -> a, 1 -> b
    if (three) {
        d = d + xor1_f64(d);
        d = d + xor2_f64(d);
        d = d + other_quad_f64(d);
        r = pair_xor8_f64(r, d);                  // lane bit 3: 0 -> a | b, 1 -> d
    } else {
        r = r + xor8_f64(r);
    }
    r = sum_xor16_f64(r);
    r = sum_xor32_f64(r);
    return 0.0 + r;
}

// A double constant held in an SGPR pair at the point of use.  The volatile
// asm keeps LLVM from hoisting it out of the transition loop into a VGPR pair
// (the hoisted exp() constants alone cost the persistent kernel 20 VGPRs and
// with them the fourth wave per SIMD).
__device__ inline double sgpr_const(unsigned long long bits)
{
    double c = __longlong_as_double((long long)bits);
    asm volatile("" : "+s"(c));
    return c;
}

// exp(x) for x in [-308, 709] (the clipped exponent of the accept test,
// hmc.py:151 + csb.numeric.exp).  Same algorithm and coefficients as the
// device math library's exp (argument reduction by ln2 in two parts, degree-11
// polynomial, ldexp), so the accept decisions are those of the library call it
// replaces; written out so that its constants stay in SGPRs.
__device__ inline double exp_clipped_range(double x)
{
    const double n = __builtin_rint(x * sgpr_const(0x3ff71547652b82feULL));     // 1/ln2
    double r = __builtin_fma(sgpr_const(0xbfe62e42fefa39efULL), n, x);          // -ln2 (hi)
    r = __builtin_fma(sgpr_const(0xbc7abc9e3b39803fULL), n, r);                 // -ln2 (lo)
    double p = __builtin_fma(sgpr_const(0x3e5ade156a5dcb37ULL), r,
                             sgpr_const(0x3e928af3fca7ab0cULL));
    p = __builtin_fma(r, p, sgpr_const(0x3ec71dee623fde64ULL));
    p = __builtin_fma(r, p, sgpr_const(0x3efa01997c89e6b0ULL));
    p = __builtin_fma(r, p, sgpr_const(0x3f2a01a014761f6eULL));
    p = __builtin_fma(r, p, sgpr_const(0x3f56c16c1852b7b0ULL));
    p = __builtin_fma(r, p, sgpr_const(0x3f81111111122322ULL));
    p = __builtin_fma(r, p, sgpr_const(0x3fa55555555502a1ULL));
    p = __builtin_fma(r, p, sgpr_const(0x3fc5555555555511ULL));
    p = __builtin_fma(r, p, sgpr_const(0x3fe000000000000bULL));
    p = __builtin_fma(r, p, 1.0);
    p = __builtin_fma(r, p, 1.0);
    return __builtin_ldexp(p, (int)n);
}

// The Metropolis test of every HMC kernel here, hmc.py:151 + csb.numeric.exp:
//   u < exp(clip(x, -308, 709)),   x = -(E_after - E_before).
// Returns exactly what `u < exp_clipped_range(clip(x))` returns, for every pair of
// doubles, but evaluates the exponential only where it can matter:
//   x >= 0 and u < 1: accepted.  exp_clipped_range never returns less than 1 for
//     x >= 0: with n = 0 it is fma(r, p, 1) with r, p >= 0, and with n >= 1 it is
//     2^n * e^r with r >= -ln2/2, at least 2 * 0.707 (tests/test_gpu_metropolis_accept.py).
//   -1/2 <= x < 0: 1 + x <= e^x <= 1 + x + x^2/2.  The two bounds are formed with two and
//     four roundings of values in [1/2, 1], each at most 2^-53, so they are off by at
//     most 2^-51; exp_clipped_range is within 2^-52 of e^x there (under 1 ulp of a value
//     below 1).  2^-40 covers both five hundred times over, so u below the lower bound
//     less the margin is below the computed exponential, and u at or above the upper
//     bound plus the margin is not.  At |x| ~ 0.01 the window between them is 5e-5 wide.
// Everything else (NaN, x < -1/2, u >= 1, u inside the window) takes the exponential,
// under a branch that a wave skips when none of its lanes needs it.
// BOUNDS = false is the exponential alone, for a kernel in which the bounds' few extra
// scalar registers cost a wave per SIMD (see hmc_gauss_persist_kernel).
template <bool BOUNDS = true>
__device__ inline bool metropolis_accept(double u, double x)
{
    if (!BOUNDS) {
        x = (x < -308.0) ? -308.0 : x;
        x = (x > 709.0) ? 709.0 : x;
        return u < exp_clipped_range(x);
    }
    const double margin = 0x1p-40;
    const double lo = (1.0 + x) - margin;
    const bool small = x >= -0.5 && x < 0.0;
    bool acc = (x >= 0.0 && u < 1.0) || (small && u < lo);
    if (!(acc || (small && u >= (1.0 + x + x * x * 0.5) + margin))) {
        x = (x < -308.0) ? -308.0 : x;
        x = (x > 709.0) ? 709.0 : x;
        acc = u < exp_clipped_range(x);
    }
    return acc;
}

// The Metropolis test from an exponent that is only known to within delta: the decision of
// metropolis_accept(u, xe) for EVERY xe with |xe - x| <= delta / 2, or GAUSS_UNDECIDED.
//
// Where x and delta come from (hmc_gauss_persist_kernel<..., FASTSUM>): xe is the exponent the
// kernel forms from the three energy sums in numpy's order, x the same expression of the
// sums accumulated as fma(d, d, acc).  With w = 2^-53 and every term of a sum >= 0:
//   * an element of a lane's accumulator passes through its own square and at most 15
//     additions in numpy's order (16 roundings), and through at most 16 fused steps in the
//     fused order; the 3 + 3 tree levels above the accumulator are the same additions on both,
//     6 roundings more (the final 0.0 + r is exact).  So each computed sum is S (1 + t) with
//     |t| <= g22 = 22 w / (1 - 22 w) of the true sum S, in either order.  The count is by depth
//     alone, 16 roundings in the lane and 6 tree levels, each sum set against the TRUE sum of
//     non-negative terms: it does not ask which elements a lane holds, so it stands as it is
//     for the WIDE kernel (hmc_gauss_kernel.hpp), whose lane l sums elements 128 r + 2 l + b
//     (tests/test_gauss_wide_bound.py restates that order);
//   * an energy is -(c * Sq) + 0.5 * Sp: one rounded product (the halving is exact), one
//     rounded addition, both terms >= 0 for k > 0: E (1 + t), |t| <= g24, in either order.
//     The two orders' energies differ by at most 2 g24 E;
//   * the difference Ea - Eb is rounded once on each side, at most w (Eb + Ea) each.
// Together |x - xe| <= (48 + 2) w (1 + 25 w) (Eb + Ea), and forming x - delta and x + delta
// below costs at most one w (Eb + Ea) more: 51 w (Eb + Ea) in all.  The kernel passes
// delta = 2^-46 (Eb~ + Ea~) = 128 w (Eb~ + Ea~) of its fused energies, which are at least
// (1 - g24) of the true ones: 2.5 times the bound, from one multiplication.  (k <= 0 or NaN
// breaks "both terms >= 0": the kernel sends every such transition to the exact sums.  Squares
// that underflow leave |x| and |xe| far below 2^-54, where every u < 1 is accepted by both.)
//
// The rules.  E is exp_clipped_range o clip, xl = x - delta, xh = x + delta; xe lies in
// [xl, xh] with room to spare.  Inputs must satisfy 0 <= u < 1, 0 <= delta <= 2^-21 and x
// finite, otherwise UNDECIDED (NaN fails each of these comparisons).
//   ACCEPT if xl >= -1/2 and u < (1 + xl) - margin.  For xe >= 0, E >= 1 > u.  For xe in
//     [xl, 0), a part of [-1/2, 0), E(xe) >= e^xe - 2^-52 >= 1 + xl - 2^-52 (metropolis_accept
//     above), and the three roundings on this side stay below 2^-51: the margin of 2^-40
//     covers both, so u < E(xe) and metropolis_accept returns true on whichever of its paths.
//   REJECT if xl >= -1/2, xh < 0 and u >= (1 + xh + xh^2 / 2) + margin.  On [-1/2, 0) the
//     upper bound rises with its argument, so E(xe) <= e^xe + 2^-52 <= bound(xh) + 2^-52 <= u.
//   Otherwise ONE exponential, y = E(x), taken under a branch as in metropolis_accept:
//     ACCEPT if u < (y - 2 delta y) - margin, REJECT if u >= (y + 2 delta y) + margin.
//     clip moves no two arguments apart, so c = clip(x) and ce = clip(xe) are within
//     delta / 2 <= 2^-22 of each other and e^ce lies in [e^c (1 - delta), e^c (1 + delta)].
//     E is the library's exponential, within 1 ulp of e^x; 4 ulps granted, E(ce) lies in
//     y [1 - delta - 2^-49, 1 + delta + 2^-49].  Where xl < 0 (else every xe >= 0, and u < 1
//     decides for acceptance as the rule does) x < 2^-21 and y < 1.001, so the 2^-49 y and the
//     three roundings are again inside the margin: below the lower value u < E(ce); at or
//     above the upper one u >= E(ce), and also u >= (1 - delta)(1 + 2 delta) >= 1 whenever
//     xe >= 0 is possible at all (c >= -delta / 2), so no path of metropolis_accept accepts.
//   Everything else is UNDECIDED: u within 2 delta e^x + margin of the threshold.  In particular
//   every u with |u - e^x| <= delta e^x is: the bounds 1 + xl and bound(xh) lie outside
//   e^x (1 -+ delta) but for 2 delta^2 <= 2^-41 at 0 < x < 2 delta, inside the margin.  (This
//   is what holds delta to 2^-21, i.e. Eb + Ea below 2^25; above it every transition takes
//   the exact sums.)
// For the unit Gaussian at D = 1024 delta is 3e-11 and the window about 2e-12 wide on either
// side of the bounds' own: order 1e-11 of the transitions take the exact sums.
enum { GAUSS_REJECT = 0, GAUSS_ACCEPT = 1, GAUSS_UNDECIDED = 2 };

__device__ inline int accept_decide(double u, double x, double delta)
{
    const double margin = 0x1p-40;
    // 0 <= u < 1 and 0 <= delta <= 2^-21 as comparisons of the bit patterns: one instruction
    // each, false for negative values (-0.0 too), infinities and NaN
    const bool ok = (unsigned long long)__double_as_longlong(u) < 0x3ff0000000000000ULL &&
                    (unsigned long long)__double_as_longlong(delta) <= 0x3ea0000000000000ULL &&
                    __builtin_fabs(x) < __builtin_inf();
    const double xl = x - delta, xh = x + delta;
    const bool inb = xl >= -0.5;
    bool acc = inb && u < (1.0 + xl) - margin;
    bool rej = inb && xh < 0.0 && u >= (1.0 + xh + xh * xh * 0.5) + margin;
    if (ok && !(acc || rej)) {
        double c = (x < -308.0) ? -308.0 : x;
        c = (c > 709.0) ? 709.0 : c;
        const double y = exp_clipped_range(c);
        const double w = (delta + delta) * y;
        acc = u < (y - w) - margin;
        rej = u >= (y + w) + margin;
    }
    return (!ok || !(acc || rej)) ? GAUSS_UNDECIDED : (acc ? GAUSS_ACCEPT : GAUSS_REJECT);
}

// np.exp on the whole real line (the accept test of the RWMC sampler,
// binf/example/samplers.py:86, uses numpy's exp, not csb's clipped one): +inf above
// the overflow threshold, subnormals and 0 below, NaN for NaN -- the same
// polynomial as every other accept test here.
__device__ inline double np_exp(double x)
{
    if (x > 709.782712893384) return __builtin_inf();
    if (x < -745.2) return 0.0;
    return exp_clipped_range(x);
}

template <bool UNIT>
__device__ inline double gauss_grad(double q, double k, double x0)
{
    // k*(x - x0), binf/pdf/__init__.py:191.  For k == 1, x0 == 0 both
    // operations are exact identities, so skipping them changes no bit.
    return UNIT ? q : k * (q - x0);
}

template <bool FMA>
__device__ inline double kick(double p, double dt, double g)
{
    return FMA ? __builtin_fma(-dt, g, p) : p - dt * g;   // hmc.py:116,120,123
}

template <bool FMA>
__device__ inline double drift(double q, double p, double dt)
{
    return FMA ? __builtin_fma(p, dt, q) : q + p * dt;    // hmc.py:119,122
}

}  // namespace binf
