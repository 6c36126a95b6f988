// Pairwise-distance-restraint model (BASELINE config C5, "chromatin-like"):
// n beads in 3-D per chain, forward model = all n(n-1)/2 pair distances,
// Gaussian error model on the distances.  gfx950, wave64.
//
// No reference code exists for this model (reference README.rst:9 only names
// the application); it is build-defined in the shape of the reference's
// plug-in surface (AbstractForwardModel / AbstractErrorModel,
// binf/model/forwardmodels.py:10-66, binf/pdf/likelihoods.py:141-155).
//
//   forward : d_p = sqrt(((xi-xj)**2).sum()) for pair p = (i<j) in np.triu order
//   energy gradient w.r.t. bead i:  tau * sum_{j != i} (d_ij - y_ij) (x_i - x_j)/d_ij
//
// This file is the model's one translation unit and holds its HOST side only: the
// extern "C" entry points, the launch helpers and the policy that chooses a force scheme
// (pair_force_route).  The device code is in the headers it includes:
//   pairdist_energy.hpp    forward distances, chi^2 by rows / by chunks, the one-launch energy
//                          (bit-identical to numpy: correctly rounded sqrt, np.sum's order);
//   pairdist_force.hpp     what the force schemes share: pair_weight, PairLeapArgs, and the
//                          integrator arithmetic (pair_chain, pair_kick, store_scaled_force);
//   pairdist_sym.hpp       32 <= n <= 256: every unordered pair once, target distances in
//                          registers, one workgroup of 1 / 4 / 9 / 16 waves per chain;
//   pairdist_ring.hpp      257 .. 1024 (packed targets): every unordered pair once as well, a
//                          wave per block of 64 row beads, block pairs walked in phases, targets
//                          streamed from the packed array; and the same tiles as a wave per tile
//                          (few chains, and the only symmetric form from 1025 to 8192 beads);
//   pairdist_onesided.hpp  other n: one-sided all-pairs loops, the chain's coordinates staged
//                          in LDS, target distances read from a symmetric [n x n] matrix.
// The [3n x n(n-1)/2] Jacobian the generic Likelihood path would need -- 200 MB per chain at
// n = 256 -- is never formed.  Each scheme has a force-only kernel and a fused leapfrog (the
// whole _leapfrog() of binf/samplers/hmc.py:92-125 in one launch) that are bit-identical to
// each other.
#include <atomic>
#include <type_traits>
#include "pairdist_energy.hpp"
#include "pairdist_force.hpp"
#include "pairdist_onesided.hpp"
#include "pairdist_sym.hpp"
#include "pairdist_ring.hpp"

using namespace binf;

// ---- launch helpers

static int32_t launched(const char *what)
{
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? hip_fail(e, what) : 0;
}

// A run-time choice as a template argument: f(std::integral_constant<int, N>{}) with N = v
// clamped to [LO, HI]; f(std::true_type{} / std::false_type{}).
template <int LO, int HI, class F>
static void with_int(int v, F &&f)
{
    if constexpr (LO < HI) {
        if (v <= LO) f(std::integral_constant<int, LO>{});
        else with_int<LO + 1, HI>(v, f);
    } else {
        f(std::integral_constant<int, LO>{});
    }
}

template <class F>
static void with_bool(bool v, F &&f)
{
    if (v) f(std::true_type{});
    else f(std::false_type{});
}

// Few chains (less than ~4 workgroups of 256 threads per CU): four lanes per
// bead; many chains: one.  Both sum in the same order (bit-identical results).
static int lanes_per_bead(int64_t C) { return C < 1024 ? 4 : 1; }

static int cu_count()
{
    // CU count of the CURRENT device (the wrappers make the stream's device current),
    // cached per device id; atomics make the first calls of several threads harmless
    static std::atomic<int> cu_cache[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    int cus = cu_cache[dev].load(std::memory_order_relaxed);
    if (cus <= 0) {
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
            cus = 256;
        cu_cache[dev].store(cus, std::memory_order_relaxed);
    }
    return cus;
}

static int blocks_of_64(int64_t n_beads) { return (int)((n_beads + 63) / 64); }

// ---- energy side

extern "C" int32_t binf_pairdist_forward_f64(const double *x, const int32_t *pair_i,
                                             const int32_t *pair_j, double *out,
                                             int64_t C, int64_t n_beads,
                                             int64_t n_pairs, void *stream)
{
    if (C < 0 || n_beads < 1 || n_pairs < 0)
        return fail(BINF_E_ARG, "pairdist_forward: bad sizes");
    if (C == 0 || n_pairs == 0) return 0;
    if (!x || !pair_i || !pair_j || !out)
        return fail(BINF_E_ARG, "pairdist_forward: null buffer");
    if (C > 65535) return fail(BINF_E_UNSUPPORTED, "pairdist_forward: more than 65535 chains per call");
    int64_t bx = (n_pairs + 255) / 256;
    if (bx > 1024) bx = 1024;
    pairdist_forward_kernel<<<dim3((unsigned)bx, (unsigned)C), 256, 0, (hipStream_t)stream>>>(
        x, pair_i, pair_j, out, n_beads, n_pairs);
    return launched("pairdist_forward launch");
}

// The chi^2 reduction of C chains over n_pairs restraints, finished as the error model's
// lp = -0.5 chi2 tau + N/2 log tau; skip = [skip [C], way [C]] of the memo, or null.
static RowGeom chi2_geom(int64_t C, int64_t n_pairs, double precision, const double *precision_chain,
                         const uint8_t *skip, double *memo_chi2)
{
    RowGeom g;
    g.C = C; g.D = (int32_t)n_pairs; g.scale = 1.0;
    g.fin.on = 1; g.fin.minus = nullptr; g.fin.tau = precision; g.fin.tau_chain = precision_chain;
    g.fin.n_data = (double)n_pairs;
    g.skip = skip; g.way = skip ? skip + C : nullptr; g.memo_sum = memo_chi2;
    g.H = row_tree_height(n_pairs);
    return g;
}

// chi^2 by chunks (pairdist_chi2_chunk_kernel) pays while a workgroup per chain leaves CUs idle and
// the pair list is long enough to split; beyond 2048 beads it is the only form that keeps the
// coordinates out of HBM round trips
static bool chunks_pay(int64_t C, int64_t n_beads, int64_t n_pairs)
{
    if (C < 1 || C > 65535 || n_pairs < 2 * NPY_BUFSIZE || n_pairs > 0x7fffffffLL) return false;
    return n_beads > 2048 || C < (int64_t)cu_count();
}

static int64_t chi2_chunks(int64_t n_pairs) { return (n_pairs + NPY_BUFSIZE - 1) / NPY_BUFSIZE; }

// the chunk sums of every chain to workspace[0 .. C K), joined into out (log-prob) and / or
// chi2_out (workspace[C K .. C K + C) when the caller passes that)
static int32_t chi2_by_chunks(const PairArgs &a, const RowGeom &g, double *workspace, double *out,
                              double *chi2_out, hipStream_t st)
{
    const int K = (int)chi2_chunks(g.D);
    pairdist_chi2_chunk_kernel<8><<<dim3((unsigned)K, (unsigned)g.C), 256, 0, st>>>(a, g, workspace, K);
    pairdist_chi2_join_kernel<<<dim3((unsigned)((g.C + 255) / 256)), 256, 0, st>>>(g, workspace, K, out, chi2_out);
    return launched("pairdist chi^2 by chunks");
}

extern "C" int64_t binf_pairdist_chi2_workspace_bytes(int64_t C, int64_t n_beads, int64_t n_pairs)
{
    if (!chunks_pay(C, n_beads, n_pairs)) return 0;
    return (C * chi2_chunks(n_pairs) + C) * (int64_t)sizeof(double);
}

// chains per workgroup of the chi^2 reduction: more than one once there are enough chains
// to fill the chip that way
static int pairdist_logp_rows(int64_t C, int64_t n_beads, int64_t n_pairs)
{
    int rows = (C >= 1024 && n_pairs >= 2048) ? 2 : 1;
    while (rows > 1 && (int64_t)rows * n_beads * 3 * (int64_t)sizeof(double) > 48 * 1024) rows >>= 1;
    return rows;
}

static int32_t pairdist_logp_run(const double *x, const int32_t *pair_i, const int32_t *pair_j,
                                 const double *ys, double precision, const double *precision_chain,
                                 double *out, const uint8_t *skip, double *memo_chi2, int64_t C,
                                 int64_t n_beads, int64_t n_pairs, void *workspace,
                                 int64_t workspace_bytes, void *stream)
{
    if (C < 0 || n_beads < 0 || n_pairs < 0)
        return fail(BINF_E_ARG, "pairdist_gauss_logp: negative size");
    if (C == 0) return 0;
    if (!out || (n_pairs > 0 && (!x || !pair_i || !pair_j || !ys)))
        return fail(BINF_E_ARG, "pairdist_gauss_logp: null buffer");
    PairArgs a;
    a.x = x; a.I = pair_i; a.J = pair_j; a.ys = ys; a.n_beads = n_beads;
    hipStream_t st = (hipStream_t)stream;
    const RowGeom g = chi2_geom(C, n_pairs, precision, precision_chain, skip, memo_chi2);
    {
        // few chains (or more than 2048 beads): every 8192-pair chunk a workgroup of its own
        const int64_t need = binf_pairdist_chi2_workspace_bytes(C, n_beads, n_pairs);
        if (need > 0 && workspace && workspace_bytes >= need) {
            if (overlap_f64(workspace, need / 8, x, C * 3 * n_beads) || overlap_f64(workspace, need / 8, out, C))
                return fail(BINF_E_ALIAS, "pairdist_gauss_logp: the workspace overlaps x or out");
            if (g.H > 7) return fail(BINF_E_UNSUPPORTED, "pairdist_gauss_logp: pairwise tree height %d", g.H);
            return chi2_by_chunks(a, g, (double *)workspace, out, nullptr, st);
        }
    }
    if (n_beads <= 2048) {          // 48 KiB of coordinates fit the LDS budget
        if (C > 0x7fffffffLL || n_pairs > 0x7fffffffLL)
            return fail(BINF_E_UNSUPPORTED, "pairdist_gauss_logp: too large");
        const int rows = pairdist_logp_rows(C, n_beads, n_pairs);
        if (g.H > 7) return fail(BINF_E_UNSUPPORTED, "pairdist_gauss_logp: pairwise tree height %d", g.H);
        const size_t lds = (size_t)rows * n_beads * 3 * sizeof(double);
        const dim3 grid((unsigned)((C + rows - 1) / rows));
        // two chains per workgroup from 2048 chains up; fewer chains than ~4 workgroups per CU
        // (and rows long enough to feed them): 16 waves per chain instead of 4
        if (rows == 2)
            pairdist_chi2_rows_kernel<2, 8, 256><<<grid, 256, lds, st>>>(a, g, out);
        else if (C < 1024 && n_pairs >= 2048)
            pairdist_chi2_rows_kernel<1, 8, 1024><<<grid, 1024, lds, st>>>(a, g, out);
        else
            pairdist_chi2_rows_kernel<1, 8, 256><<<grid, 256, lds, st>>>(a, g, out);
        return launched("pairdist_gauss_logp");
    }
    return row_reduce_launch<PairResidMake, PairArgs>(a, C, n_pairs, 1.0, out, st, true,
                                                      "pairdist_gauss_logp", &g.fin, skip, memo_chi2);
}

extern "C" int32_t binf_pairdist_gauss_logp_f64(const double *x, const int32_t *pair_i,
                                                const int32_t *pair_j, const double *ys,
                                                double precision,
                                                const double *precision_chain, double *out,
                                                int64_t C, int64_t n_beads,
                                                int64_t n_pairs, void *workspace,
                                                int64_t workspace_bytes, void *stream)
{
    return pairdist_logp_run(x, pair_i, pair_j, ys, precision, precision_chain, out, nullptr, nullptr,
                             C, n_beads, n_pairs, workspace, workspace_bytes, stream);
}

// The same with a per-chain memo of chi^2 (a function of the chain's coordinates alone),
// checked on the device bit for bit: rowsum.hpp, row_memo_check_kernel.
extern "C" int32_t binf_pairdist_gauss_logp_memo_f64(const double *x, const int32_t *pair_i,
                                                     const int32_t *pair_j, const double *ys,
                                                     double precision,
                                                     const double *precision_chain, double *out,
                                                     double *memo_x, double *memo_chi2,
                                                     uint8_t *skip, int64_t C, int64_t n_beads,
                                                     int64_t n_pairs, void *workspace,
                                                     int64_t workspace_bytes, void *stream)
{
    if (C < 0 || n_beads < 0 || n_pairs < 0)
        return fail(BINF_E_ARG, "pairdist_gauss_logp_memo: negative size");
    if (C == 0) return 0;
    if (!x || !memo_x || !memo_chi2 || !skip)
        return fail(BINF_E_ARG, "pairdist_gauss_logp_memo: null buffer");
    // every refusal of the reduction BEFORE the memo is touched (row_memo_check rewrites the
    // stored coordinates of a missed chain; their chi^2 is stored by the reduction after it)
    if (!out || (n_pairs > 0 && (!pair_i || !pair_j || !ys)))
        return fail(BINF_E_ARG, "pairdist_gauss_logp_memo: null buffer");
    int32_t rc = row_reduce_check(C, n_pairs, "pairdist_gauss_logp_memo");
    if (rc) return rc;
    {
        const int64_t need = binf_pairdist_chi2_workspace_bytes(C, n_beads, n_pairs);
        if (need > 0 && workspace && workspace_bytes >= need &&
            (overlap_f64(workspace, need / 8, x, C * 3 * n_beads) || overlap_f64(workspace, need / 8, out, C) ||
             overlap_f64(workspace, need / 8, memo_x, 2 * C * 3 * n_beads) || overlap_f64(workspace, need / 8, memo_chi2, 2 * C)))
            return fail(BINF_E_ALIAS, "pairdist_gauss_logp_memo: the workspace overlaps a buffer");
    }
    rc = row_memo_check(x, memo_x, skip, C, 3 * n_beads, (hipStream_t)stream,
                        "pairdist_gauss_logp_memo check launch");
    if (rc) return rc;
    return pairdist_logp_run(x, pair_i, pair_j, ys, precision, precision_chain, out, skip, memo_chi2,
                             C, n_beads, n_pairs, workspace, workspace_bytes, stream);
}

extern "C" int32_t binf_pairdist_hmc_energy_f64(const double *x, const double *p,
                                                const int32_t *pair_i, const int32_t *pair_j,
                                                const double *ys, double precision,
                                                const double *precision_chain, double prior_k,
                                                double prior_x0, int32_t n_terms,
                                                const int32_t *term_kind, const double *extra0,
                                                double extra0_scalar, const double *extra1,
                                                double extra1_scalar,
                                                double *energy, double *log_prob, double *memo_x,
                                                double *memo_chi2, uint8_t *memo_state, int64_t C,
                                                int64_t n_beads, int64_t n_pairs, void *workspace,
                                                int64_t workspace_bytes, void *stream)
{
    if (C < 0 || n_beads < 1 || n_pairs < 0)
        return fail(BINF_E_ARG, "pairdist_hmc_energy: bad sizes");
    if (n_terms < 1 || n_terms > 4 || !term_kind)
        return fail(BINF_E_ARG, "pairdist_hmc_energy: 1 to 4 terms, with their kinds");
    int has_prior = 0, seen = 0;
    for (int k = 0; k < n_terms; ++k) {
        const int kind = term_kind[k];
        if (kind < 0 || kind > 3 || (seen & (1 << kind)))
            return fail(BINF_E_ARG, "pairdist_hmc_energy: term kinds are 0..3, each at most once");
        seen |= 1 << kind;
        if (kind == 0) has_prior = 1;
    }
    if (!(seen & 2)) return fail(BINF_E_ARG, "pairdist_hmc_energy: the likelihood (kind 1) must be a term");
    if (C == 0) return 0;
    if (!x || !p || !energy || (n_pairs > 0 && (!pair_i || !pair_j || !ys)))
        return fail(BINF_E_ARG, "pairdist_hmc_energy: null buffer");
    if ((memo_x != nullptr) != (memo_chi2 != nullptr) || (memo_x != nullptr) != (memo_state != nullptr))
        return fail(BINF_E_ARG, "pairdist_hmc_energy: memo_x, memo_chi2 and memo_state go together");
    if (C > 0x7fffffffLL || n_pairs > 0x7fffffffLL)
        return fail(BINF_E_UNSUPPORTED, "pairdist_hmc_energy: too large");
    if (n_beads > 2048)
        return fail(BINF_E_UNSUPPORTED, "pairdist_hmc_energy: n_beads=%lld > 2048 (coordinates staged in LDS)",
                    (long long)n_beads);
    const RowGeom g = chi2_geom(C, n_pairs, precision, precision_chain, nullptr, memo_chi2);
    PairEnergyArgs a;
    a.x = x; a.p = p; a.I = pair_i; a.J = pair_j; a.ys = ys; a.memo_x = memo_x; a.memo_state = memo_state;
    a.energy = energy; a.log_prob = log_prob;
    a.prior_scale = -0.5 * prior_k; a.prior_x0 = prior_x0;
    a.has_prior = has_prior; a.n_terms = n_terms;
    for (int k = 0; k < 4; ++k) a.term_kind[k] = k < n_terms ? term_kind[k] : 1;
    a.extra[0] = extra0; a.extra[1] = extra1; a.extra_scalar[0] = extra0_scalar; a.extra_scalar[1] = extra1_scalar;
    a.n_beads = (int32_t)n_beads; a.H_d = row_tree_height(3 * n_beads);
    a.chi2_in = nullptr;
    if (g.H > 7 || a.H_d > 7)
        return fail(BINF_E_UNSUPPORTED, "pairdist_hmc_energy: pairwise tree height %d", g.H > a.H_d ? g.H : a.H_d);
    hipStream_t st = (hipStream_t)stream;
    {
        // few chains: chi^2 by chunks first (every 8192-pair chunk a workgroup of its own), the rest
        // of the energy from it
        const int64_t need = binf_pairdist_chi2_workspace_bytes(C, n_beads, n_pairs);
        if (need > 0 && workspace && workspace_bytes >= need) {
            if (overlap_f64(workspace, need / 8, x, C * 3 * n_beads) || overlap_f64(workspace, need / 8, p, C * 3 * n_beads) ||
                overlap_f64(workspace, need / 8, energy, C) || (log_prob && overlap_f64(workspace, need / 8, log_prob, C)))
                return fail(BINF_E_ALIAS, "pairdist_hmc_energy: the workspace overlaps a buffer");
            PairArgs pa;
            pa.x = x; pa.I = pair_i; pa.J = pair_j; pa.ys = ys; pa.n_beads = n_beads;
            RowGeom gc = g;
            if (memo_x) {
                // the memo as the log-prob entry point keeps it: checked (and, on a miss, its
                // coordinates rewritten) by a launch of its own, hits skip their chunks, the join
                // stores the new sums -- the same entries and flags the one-launch kernel leaves
                if (overlap_f64(workspace, need / 8, memo_x, 2 * C * 3 * n_beads) || overlap_f64(workspace, need / 8, memo_chi2, 2 * C))
                    return fail(BINF_E_ALIAS, "pairdist_hmc_energy: the workspace overlaps the memo");
                const int32_t rm = row_memo_check(x, memo_x, memo_state, C, 3 * n_beads, st,
                                                  "pairdist_hmc_energy memo check launch");
                if (rm) return rm;
                gc.skip = memo_state; gc.way = memo_state + C; gc.memo_sum = memo_chi2;
            } else {
                gc.memo_sum = nullptr; gc.skip = nullptr; gc.way = nullptr;
            }
            double *chi2 = (double *)workspace + C * chi2_chunks(n_pairs);
            const int32_t rc = chi2_by_chunks(pa, gc, (double *)workspace, nullptr, chi2, st);
            if (rc) return rc;
            a.chi2_in = chi2;
        }
    }
    const int rows = pairdist_logp_rows(C, n_beads, n_pairs);
    const size_t lds = (size_t)rows * n_beads * 3 * sizeof(double);
    if (rows == 2)
        pairdist_energy_kernel<2, 8, 256><<<dim3((unsigned)((C + 1) / 2)), 256, lds, st>>>(a, g);
    else if (C < 1024 && n_pairs >= 2048)           // few chains: 16 waves per chain (as the log-prob)
        pairdist_energy_kernel<1, 8, 1024><<<dim3((unsigned)C), 1024, lds, st>>>(a, g);
    else
        pairdist_energy_kernel<1, 8, 256><<<dim3((unsigned)C), 256, lds, st>>>(a, g);
    return launched("pairdist_hmc_energy launch");
}

// ---- force side: which scheme serves a call

static bool sym_serves(int64_t n_beads)
{
    return n_beads >= SYM_MIN_BEADS && n_beads <= SYM_MAX_BEADS;
}

// 257 .. 1024 beads WITH packed targets: the ring kernels
static bool ring_serves(int64_t n_beads)
{
    return n_beads > SYM_MAX_BEADS && n_beads <= RING_MAX_BEADS;
}

// ... and up to TILES_MAX_BEADS the tile kernels (alone beyond RING_MAX_BEADS: no
// workgroup-per-chain form there)
static bool tiles_serve(int64_t n_beads)
{
    return n_beads > SYM_MAX_BEADS && n_beads <= TILES_MAX_BEADS;
}

// Few chains of 257..1024 beads: every tile a wave of its own (pairdist_tiles_kernel) when the
// caller brings the workspace for the tiles' partial sums -- same bits as the ring kernels,
// which serve every other case.  A workgroup per chain keeps 64 NBLK threads busy per chain:
// tiles pay while that leaves most of the chip idle.
static bool tiles_pay(int64_t C, int64_t n_beads)
{
    if (!tiles_serve(n_beads) || C > 65535) return false;
    if (n_beads > RING_MAX_BEADS) return true;       // the only symmetric form beyond 1024 beads
    // measured cross-over (scripts/probe_pairdist_few_chains.py, 256 CUs): a sample() of L = 20
    // costs 0.52 / 0.87 / 2.9 ms with a workgroup per chain at 320 / 512 / 1024 beads whatever
    // the number of chains up to ~256, and 0.35 + 0.0013 C / 0.43 + 0.0033 C / 0.82 + 0.0105 C ms
    // with a wave per tile: tiles win up to ~140 / 130 / 195 chains
    const int64_t nblk = blocks_of_64(n_beads);
    return C <= (96 + 6 * nblk) * (int64_t)cu_count() / 256;
}

extern "C" int64_t binf_pairdist_tiles_workspace_bytes(int64_t C, int64_t n_beads)
{
    if (C < 1 || n_beads < 1 || !tiles_pay(C, n_beads)) return 0;
    return C * ring_tiles(blocks_of_64(n_beads)) * 2 * 3 * 64 * (int64_t)sizeof(double);
}

extern "C" int64_t binf_pairdist_packed_targets_bytes(int64_t n_beads)
{
    const int64_t nblk = blocks_of_64(n_beads);
    if (tiles_serve(n_beads)) return nblk * ring_steps((int)nblk) * 64 * (int64_t)sizeof(double);
    if (!sym_serves(n_beads)) return 0;
    return nblk * nblk * SYM_STEPS * 64 * (int64_t)sizeof(double);
}

// The scheme of a force evaluation or a fused leapfrog of C chains.  The sym kernels take
// packed or unpacked targets; ring and tiles need the packed ones, tiles also the workspace of
// binf_pairdist_tiles_workspace_bytes (which is 0 where tiles do not pay).  None: beyond 1024
// beads without the tile route -- the two entry points differ in what they do then.
enum class PairRoute { Sym, Tiles, Ring, OneSided, None };

static PairRoute pair_force_route(int64_t C, int64_t n_beads, bool packed, const void *workspace,
                                  int64_t workspace_bytes)
{
    if (sym_serves(n_beads)) return PairRoute::Sym;
    if (packed && tiles_serve(n_beads)) {
        const int64_t need = binf_pairdist_tiles_workspace_bytes(C, n_beads);
        if (need > 0 && workspace && workspace_bytes >= need) return PairRoute::Tiles;
        if (ring_serves(n_beads)) return PairRoute::Ring;
    }
    return n_beads <= RING_MAX_BEADS ? PairRoute::OneSided : PairRoute::None;
}

// does the tile route's workspace overlap a [C x 3n] buffer of the call?
static bool tiles_workspace_overlaps(const void *workspace, int64_t C, int64_t n_beads, const void *buf)
{
    return overlap_f64(workspace, binf_pairdist_tiles_workspace_bytes(C, n_beads) / 8, buf, C * 3 * n_beads);
}

// workgroups of the n <= 256 kernels: as many as the chip holds at a time (16 waves per
// CU at 126 VGPRs: 16 / 4 / 1 / 1 workgroups of 1 / 4 / 9 / 16 waves); each walks its
// share of the chains
static unsigned sym_grid(int64_t C, int nblk)
{
    const int64_t slots = (int64_t)cu_count() * (nblk == 1 ? 16 : (nblk == 2 ? 4 : 1));
    return (unsigned)(C < slots ? C : slots);
}

// workgroups of the ring kernels: as many as the chip holds at a time (NBLK <= 8: two
// per CU, 16 waves; else one), each walks its share of the chains
static unsigned ring_grid(int64_t C, int nblk)
{
    const int64_t slots = (int64_t)cu_count() * (nblk <= 8 ? 2 : 1);
    return (unsigned)(C < slots ? C : slots);
}

extern "C" int32_t binf_pairdist_pack_targets_f64(const double *ymat, double *packed,
                                                  int64_t n_beads, void *stream)
{
    if (n_beads < 1) return fail(BINF_E_ARG, "pairdist_pack_targets: bad size");
    if (!sym_serves(n_beads) && !tiles_serve(n_beads))
        return fail(BINF_E_UNSUPPORTED, "pairdist_pack_targets: n_beads=%lld has no packed form "
                    "(binf_pairdist_packed_targets_bytes is 0)", (long long)n_beads);
    if (!ymat || !packed) return fail(BINF_E_ARG, "pairdist_pack_targets: null buffer");
    hipStream_t st = (hipStream_t)stream;
    const int nblk = blocks_of_64(n_beads);
    if (tiles_serve(n_beads))
        ring_pack_targets_kernel<<<dim3((unsigned)nblk), 256, 0, st>>>(ymat, packed, (int)n_beads, nblk);
    else
        with_int<1, 4>(nblk, [&](auto NB) {
            sym_pack_targets_kernel<decltype(NB)::value><<<1, dim3(64 * nblk * nblk), 0, st>>>(ymat, packed, (int)n_beads);
        });
    return launched("pairdist_pack_targets launch");
}

// ---- force side: the gradient of the per-step tier

static void launch_tiles(const double *x, const double *ypk, double *part, int64_t C, int64_t n, hipStream_t st)
{
    const int nblk = blocks_of_64(n);
    const dim3 grid((unsigned)((ring_tiles(nblk) + TILE_WAVES - 1) / TILE_WAVES), (unsigned)C);
    with_bool(n == 64 * nblk, [&](auto FULL) {
        pairdist_tiles_kernel<decltype(FULL)::value><<<grid, 64 * TILE_WAVES, 0, st>>>(x, ypk, part, (int32_t)n, nblk);
    });
}

extern "C" int32_t binf_pairdist_gauss_grad_f64(const double *x, const double *ymat,
                                                double precision,
                                                const double *precision_chain,
                                                double *out, int64_t C,
                                                int64_t n_beads, void *stream)
{
    return binf_pairdist_gauss_grad_packed_f64(x, ymat, nullptr, precision, precision_chain, out, C,
                                               n_beads, nullptr, 0, stream);
}

extern "C" int32_t binf_pairdist_gauss_grad_packed_f64(const double *x, const double *ymat,
                                                       const double *packed, double precision,
                                                       const double *precision_chain,
                                                       double *out, int64_t C,
                                                       int64_t n_beads, void *workspace,
                                                       int64_t workspace_bytes, void *stream)
{
    if (C < 0 || n_beads < 1) return fail(BINF_E_ARG, "pairdist_gauss_grad: bad sizes");
    if (C == 0) return 0;
    if (!x || !ymat || !out) return fail(BINF_E_ARG, "pairdist_gauss_grad: null buffer");
    if (n_beads > 46340 || C > 0x7fffffffLL)
        return fail(BINF_E_UNSUPPORTED, "pairdist_gauss_grad: too large");
    const PairRoute route = pair_force_route(C, n_beads, packed != nullptr, workspace, workspace_bytes);
    if (route == PairRoute::Tiles && (tiles_workspace_overlaps(workspace, C, n_beads, x) ||
                                      tiles_workspace_overlaps(workspace, C, n_beads, out)))
        return fail(BINF_E_ALIAS, "pairdist_gauss_grad: the workspace overlaps x or out");
    hipStream_t st = (hipStream_t)stream;
    const int32_t n = (int32_t)n_beads;
    const int nblk = blocks_of_64(n_beads);
    const bool full = n_beads == 64 * nblk;
    const size_t lds = (size_t)n_beads * 3 * sizeof(double);
    switch (route) {
    case PairRoute::Sym:
        with_int<1, 4>(nblk, [&](auto NB) { with_bool(full, [&](auto FULL) { with_bool(packed != nullptr, [&](auto PK) {
            constexpr int NBLK = decltype(NB)::value;
            pairdist_grad_sym_kernel<decltype(FULL)::value, NBLK, decltype(PK)::value>
                <<<dim3(sym_grid(C, NBLK)), dim3(64 * NBLK * NBLK), 0, st>>>(x, ymat, packed, precision,
                                                                             precision_chain, out, n, C);
        }); }); });
        break;
    case PairRoute::Tiles:
        launch_tiles(x, packed, (double *)workspace, C, n_beads, st);
        pairdist_tiles_grad_kernel<<<dim3((unsigned)((n_beads + 255) / 256), (unsigned)C), 256, 0, st>>>(
            (const double *)workspace, precision, precision_chain, out, n, nblk);
        break;
    case PairRoute::Ring:
        with_bool(nblk <= 8, [&](auto SMALL) { with_bool(full, [&](auto FULL) {
            pairdist_grad_ring_kernel<decltype(FULL)::value, decltype(SMALL)::value ? 8 : 16>
                <<<dim3(ring_grid(C, nblk)), dim3(64 * nblk), 0, st>>>(x, packed, precision, precision_chain,
                                                                       out, n, nblk, C);
        }); });
        break;
    case PairRoute::OneSided:
        with_bool(lanes_per_bead(C) == 4, [&](auto FOUR) {
            constexpr int LANES = decltype(FOUR)::value ? 4 : 1;
            pairdist_grad_lanes_kernel<LANES><<<dim3((unsigned)C), 256 * LANES, lds, st>>>(x, ymat, precision,
                                                                                          precision_chain, out, n);
        });
        break;
    case PairRoute::None:           // beyond 1024 beads the gradient still has one-sided loops; the leapfrog has none
        pairdist_grad_kernel<256><<<dim3((unsigned)C), 256, 0, st>>>(x, ymat, precision, precision_chain, out, n);
        break;
    }
    return launched("pairdist_gauss_grad launch");
}

// ---- force side: the fused leapfrog

extern "C" int32_t binf_pairdist_leapfrog_f64(double *q, double *p, const double *ymat,
                                              double precision, const double *precision_chain,
                                              int32_t has_prior, double prior_k, double prior_x0,
                                              int32_t prior_first, double timestep,
                                              const double *dt_chain, int32_t nsteps, int64_t C,
                                              int64_t n_beads, int32_t mode, void *stream)
{
    return binf_pairdist_leapfrog_packed_f64(q, nullptr, p, ymat, nullptr, precision, precision_chain,
                                             has_prior, prior_k, prior_x0, prior_first, timestep, dt_chain,
                                             nsteps, C, n_beads, mode, nullptr, 0, stream);
}

extern "C" int32_t binf_pairdist_leapfrog_packed_f64(double *q, const double *q_from, double *p,
                                                     const double *ymat,
                                                     const double *packed, double precision,
                                                     const double *precision_chain,
                                                     int32_t has_prior, double prior_k, double prior_x0,
                                                     int32_t prior_first, double timestep,
                                                     const double *dt_chain, int32_t nsteps, int64_t C,
                                                     int64_t n_beads, int32_t mode, void *workspace,
                                                     int64_t workspace_bytes, void *stream)
{
    if (C < 0 || n_beads < 1 || nsteps < 1)
        return fail(BINF_E_ARG, "pairdist_leapfrog: need C>=0, n_beads>=1, nsteps>=1");
    if (mode != BINF_MODE_EXACT && mode != BINF_MODE_FMA)
        return fail(BINF_E_ARG, "pairdist_leapfrog: unknown mode %d", mode);
    if (C == 0) return 0;
    if (!q || !p || !ymat) return fail(BINF_E_ARG, "pairdist_leapfrog: null buffer");
    const PairRoute route = pair_force_route(C, n_beads, packed != nullptr, workspace, workspace_bytes);
    if (route == PairRoute::None)   // beyond 1024 beads only as a wave per tile; no one-sided leapfrog there
        return fail(BINF_E_UNSUPPORTED, "pairdist_leapfrog: n_beads=%lld > 1024 needs packed targets and the "
                    "workspace of binf_pairdist_tiles_workspace_bytes (up to %d beads)", (long long)n_beads,
                    TILES_MAX_BEADS);
    if (C > 0x7fffffffLL) return fail(BINF_E_UNSUPPORTED, "pairdist_leapfrog: too many chains");
    // q_from may be q itself (in place) or a separate buffer; a PARTIAL overlap -- with q, or with
    // the momenta the launch updates -- would have chains read what others already wrote
    if (q_from && q_from != q && (overlap_f64(q_from, C * 3 * n_beads, q, C * 3 * n_beads) ||
                                  overlap_f64(q_from, C * 3 * n_beads, p, C * 3 * n_beads)))
        return fail(BINF_E_ALIAS, "pairdist_leapfrog: q_from may be exactly q or a separate buffer, "
                    "not a partial overlap with q or p");
    if (overlap_f64(q, C * 3 * n_beads, p, C * 3 * n_beads))
        return fail(BINF_E_ALIAS, "pairdist_leapfrog: q and p overlap");
    if (route == PairRoute::Tiles && (tiles_workspace_overlaps(workspace, C, n_beads, q) ||
                                      tiles_workspace_overlaps(workspace, C, n_beads, p) ||
                                      (q_from && tiles_workspace_overlaps(workspace, C, n_beads, q_from))))
        return fail(BINF_E_ALIAS, "pairdist_leapfrog: the workspace overlaps q, q_from or p");
    PairLeapArgs a;
    a.q = q; a.q_from = (q_from == q) ? nullptr : q_from; a.p = p; a.ymat = ymat; a.ypk = packed;
    a.tau_chain = precision_chain; a.dt_chain = dt_chain;
    a.tau = precision; a.timestep = timestep; a.prior_k = prior_k; a.prior_x0 = prior_x0;
    a.has_prior = has_prior ? 1 : 0; a.prior_first = prior_first ? 1 : 0;
    a.nsteps = nsteps; a.n_beads = (int32_t)n_beads; a.n_chains = C;
    hipStream_t st = (hipStream_t)stream;
    const bool fma = mode == BINF_MODE_FMA;
    const int nblk = blocks_of_64(n_beads);
    const bool full = n_beads == 64 * nblk;
    switch (route) {
    case PairRoute::Sym:
        with_int<1, 4>(nblk, [&](auto NB) { with_bool(fma, [&](auto FMA) { with_bool(full, [&](auto FULL) {
            with_bool(packed != nullptr, [&](auto PK) {
                constexpr int NBLK = decltype(NB)::value;
                pairdist_leapfrog_sym_kernel<decltype(FMA)::value, decltype(FULL)::value, NBLK, decltype(PK)::value>
                    <<<dim3(sym_grid(C, NBLK)), dim3(64 * NBLK * NBLK), 0, st>>>(a);
            });
        }); }); });
        break;
    case PairRoute::Tiles: {
        // few chains: per force evaluation one launch of a wave per tile and one that adds the
        // partial sums and kicks / drifts -- the ring kernel's arithmetic, bit for bit
        const dim3 ug((unsigned)((n_beads + 255) / 256), (unsigned)C);
        for (int e = 0; e <= nsteps; ++e) {
            const double *qin = (e == 0 && a.q_from) ? a.q_from : q;
            launch_tiles(qin, packed, (double *)workspace, C, n_beads, st);
            with_bool(fma, [&](auto FMA) {
                pairdist_tiles_update_kernel<decltype(FMA)::value><<<ug, 256, 0, st>>>((const double *)workspace, a, qin, nblk, e);
            });
        }
        break;
    }
    case PairRoute::Ring:
        with_bool(fma, [&](auto FMA) { with_bool(full, [&](auto FULL) { with_bool(nblk <= 8, [&](auto SMALL) {
            pairdist_leapfrog_ring_kernel<decltype(FMA)::value, decltype(FULL)::value, decltype(SMALL)::value ? 8 : 16>
                <<<dim3(ring_grid(C, nblk)), dim3(64 * nblk), 0, st>>>(a, nblk);
        }); }); });
        break;
    case PairRoute::OneSided: {
        const int nb = (int)((n_beads + 255) / 256);
        const bool four = lanes_per_bead(C) == 4;
        // positions; four tiles x four lanes keep the momentum there as well
        const size_t lds = (size_t)n_beads * 3 * sizeof(double) * ((nb >= 4 && four) ? 2 : 1);
        with_int<1, 4>(nb, [&](auto NB) { with_bool(fma, [&](auto FMA) { with_bool(four, [&](auto FOUR) {
            constexpr int LANES = decltype(FOUR)::value ? 4 : 1;
            pairdist_leapfrog_kernel<decltype(NB)::value, decltype(FMA)::value, LANES>
                <<<dim3((unsigned)C), 256 * LANES, lds, st>>>(a);
        }); }); });
        break;
    }
    case PairRoute::None:
        break;                      // refused above
    }
    return launched("pairdist_leapfrog launch");
}
