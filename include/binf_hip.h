/*
 * binf_hip.h -- C ABI of libbinf_hip.so, the MI355X (gfx950) engine behind
 * binf's HMC hot path.  Plain C types only; every pointer marked "device" is
 * HBM memory owned by the CALLER (e.g. a PyTorch-ROCm tensor's data_ptr()).
 *
 * Conventions (all functions)
 *   - return 0 on success, <0 for an argument error (BINF_E_*), >0 = hipError_t.
 *     Nothing is thrown across the ABI; binf_last_error() gives the text.
 *   - stateless and re-entrant; work is enqueued on `stream` (a hipStream_t,
 *     NULL = the default stream) and the call returns without synchronising.
 *   - the library allocates nothing persistent, keeps no pointer past return
 *     and never frees caller memory.  Safe inside hipGraph stream capture.
 *   - layout: chain-major row-major fp64, x[c*D + i] for chain c, dimension i.
 *
 * The reference (simeoncarstens/binf) has no native code and no FFI; each
 * entry point below names the reference Python it replaces (paths relative to
 * the reference root).
 */
#ifndef BINF_HIP_H
#define BINF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: every entry point that GENERATES draws takes the global index of its first
 *    chain / element (chain_offset, elem_offset) so that a sharded run reproduces
 *    the unsharded one bit for bit; new entry points for the RWMC subsampler.
 *    (1 -> 2 also covers the contract changes made late in ABI 1: the polynomial
 *    gradient's workspace is mandatory, binf_hmc_sample_poly_f64 accepts N <= 1024.)
 * 3: binf_hmc_sample_poly_f64 spreads a chain's data over a lane group for EVERY
 *    N <= 1024 (the force's summation order for N <= 128 changed with it; one lane
 *    per chain is now the opt-in BINF_MODE_LANE_PER_CHAIN); binf_gibbs_poly_sample_n_f64,
 *    binf_jacobian_contract_f64, binf_sum_terms_f64, binf_poly_leapfrog_f64,
 *    binf_poly_gauss_logp_memo_f64, binf_pairdist_gauss_logp_memo_f64,
 *    binf_hmc_sample_n_gauss_big_f64 / _rng_f64.
 * 4: binf_pairdist_packed_targets_bytes, binf_pairdist_pack_targets_f64,
 *    binf_pairdist_gauss_grad_packed_f64, binf_pairdist_leapfrog_packed_f64,
 *    binf_pairdist_hmc_energy_f64, binf_rng_normal_zig_uniform_f64; the chi^2
 *    memos of binf_poly_gauss_logp_memo_f64 / binf_pairdist_gauss_logp_memo_f64 hold two
 *    entries per chain (their buffers are twice the ABI 3 size).
 * 5: binf_sum_terms_bcast_f64 (terms that are ONE device double, broadcast: a 0-dim
 *    tensor never has to be read back to the host); binf_hmc_sample_n_gauss_rng_f64 /
 *    binf_hmc_gauss_rng_draws_f64 take one stream position per TRANSITION (offset + i),
 *    as the long-chain entry points always did.
 * 6: optional workspace for the pair-distance log-prob / energy entry points (chi^2 by chunks with
 *    few chains: binf_pairdist_chi2_workspace_bytes); packed targets and the ring kernels for 257..1024 beads (binf_pairdist_packed_targets_bytes
 *    is no longer 0 there), the `_packed_` entry points take an optional workspace
 *    (binf_pairdist_tiles_workspace_bytes: a wave per tile when there are few chains); binf_predictive_density_f64 / _workspace_bytes (the consumer side of the sample store: the
 *    posterior-predictive density over a grid of points in one launch).
 * 7: binf_linear_forward_f64, binf_linear_gauss_logp_f64 / _workspace_bytes (linear forward
 *    models with any design matrix).  Grown since without a new number, by symbols only:
 *    binf_linear_resident_supported, binf_hmc_sample_linear_f64,
 *    binf_gibbs_linear_sample_n_f64, binf_replica_gather_f64, binf_replica_swap_f64,
 *    binf_chain_moments_f64, binf_chain_autocov_f64 / _workspace_bytes,
 *    binf_diag_summary_f64 / _workspace_bytes, binf_rank_normalise_f64,
 *    binf_rank_sort_workspace_bytes, binf_sorted_quantiles_f64, binf_draws_map_f64,
 *    binf_rank_diag_combine_f64, binf_leapfrog_kick_scaled_f64,
 *    binf_leapfrog_drift_scaled_f64, binf_leapfrog_kick_drift_scaled_f64,
 *    binf_metric_accumulate_f64, binf_metric_pool_f64, binf_leapfrog_kick_dense_f64,
 *    binf_leapfrog_drift_dense_f64, binf_leapfrog_kick_drift_dense_f64,
 *    binf_metric_comoments_f64, binf_metric_factor_f64, binf_nuts_begin_f64,
 *    binf_nuts_leaf_f64, binf_nuts_pending, binf_nuts_adapt_step_f64,
 *    binf_replica_work_f64, binf_free_energy_chunk, binf_free_energy_bar_f64 /
 *    _workspace_bytes, binf_chees_accept_prob_f64, binf_chees_means_f64,
 *    binf_chees_terms_f64, binf_chees_sums_f64, binf_chees_workspace_bytes,
 *    binf_smc_temper_f64, binf_smc_resample_f64, binf_smc_gather_f64,
 *    binf_gauss_pointwise_loglik_f64, binf_psis_loo_f64 / _workspace_bytes,
 *    binf_pointwise_totals_f64, binf_glm_pointwise_f64, binf_linear_glm_logp_f64 /
 *    _workspace_bytes, binf_linear_glm_grad_f64 / _workspace_bytes,
 *    binf_linear_glm_leapfrog_f64 / _workspace_bytes, binf_negbin_count_term_f64,
 *    binf_negbin_pointwise_f64, binf_linear_negbin_logp_f64, binf_linear_negbin_grad_f64,
 *    binf_linear_negbin_leapfrog_f64 (the number guards changed
 *    contracts; none changed). */
#define BINF_ABI_VERSION 7

#define BINF_E_ARG        (-1)  /* null pointer / negative size / bad flag    */
#define BINF_E_UNSUPPORTED (-2) /* shape outside what the kernels cover       */
#define BINF_E_ALIAS      (-3)  /* illegal partial overlap of buffers         */

/* arithmetic mode of the leapfrog update */
#define BINF_MODE_EXACT 0  /* every multiply and add rounded separately, numpy
                              pairwise-sum order: bit-identical to the CPU
                              restatement of the reference's numpy path      */
#define BINF_MODE_FMA   1  /* p-=dt*g and q+=p*dt contracted to one FMA each:
                              within 1e-10 relative of EXACT, not bit-equal  */
/* flag, OR-ed into `mode` of binf_hmc_sample_poly_f64 only: one LANE per chain
 * (N <= 128) instead of a lane group -- the faster layout from ~10^5 chains up.
 * Energies are the same bits; the force is summed in data order instead of
 * per-lane partial sums + butterfly, so trajectories differ at rounding level. */
#define BINF_MODE_LANE_PER_CHAIN 16

int32_t binf_abi_version(void);

/* Copies the calling thread's last error text (NUL-terminated, truncated to
 * n) into buf; returns its full length. */
int32_t binf_last_error(char *buf, size_t n);

/* ------------------------------------------------------------------------
 * Fused HMC transition on an isotropic Gaussian  (BASELINE config C2)
 *
 * Replaces, for C independent chains in one launch:
 *   HMCSampler.sample()          binf/samplers/hmc.py:136-164
 *   HMCSampler._leapfrog()       binf/samplers/hmc.py:92-125
 *   HMCSampler._adapt_timestep() binf/samplers/hmc.py:183-191
 *   TestHO log_prob / gradient   binf/pdf/__init__.py:181-191
 *       log p(x) = -0.5*k*sum((x-x0)**2),  gradient = k*(x-x0)  [of -log p]
 *
 * Per chain c:   p = p0[c];  E_b = V(q0)+0.5*sum(p**2);  leapfrog nsteps;
 *   E_a = V(q)+0.5*sum(p**2);  acc = u[c] < exp(clip(-(E_a-E_b),-308,709));
 *   q_out[c] = acc ? q : q0[c].
 *
 *   q0, p0      device, [C*D]   start positions; momentum draws (the
 *                               np.random.normal(size=D) of hmc.py:146)
 *   u           device, [C]     uniform draws (hmc.py:151)
 *   q_out       device, [C*D]   returned samples.  May be EXACTLY q0 (state
 *                               updated in place) or disjoint from q0/p0.
 *   accepted    device, [C]     1/0
 *   n_accepted  device, [C] or NULL  per-chain acceptance counter, += 1 on
 *                               accept (hmc.py:161)
 *   e_before/e_after device,[C] energies of hmc.py:148,150 (may be NULL)
 *   timestep    host scalar     used when dt_chain == NULL
 *   dt_chain    device, [C] or NULL  per-chain timestep; when adapt != 0 it is
 *                               updated in place: *uprate on accept,
 *                               *downrate on reject (hmc.py:188-191).
 *                               adapt != 0 requires dt_chain != NULL.
 *   mode        BINF_MODE_EXACT | BINF_MODE_FMA
 * Supported: 1 <= D <= 8192 whose numpy pairwise-sum tree has height <= 6
 * (every D <= 7400 and all multiples of 64 up to 8192; one wave per chain up to
 * height 3, i.e. D <= ~1024, then 2 / 4 / 8 waves per chain); nsteps >= 1.
 * ---------------------------------------------------------------------- */
int32_t binf_hmc_sample_gauss_f64(const double *q0, const double *p0,
                                  const double *u, double *q_out,
                                  uint8_t *accepted, int64_t *n_accepted,
                                  double *e_before,
                                  double *e_after, double timestep,
                                  double *dt_chain, int64_t C, int64_t D,
                                  int32_t nsteps, double k, double x0,
                                  int32_t adapt, double uprate, double downrate,
                                  int32_t mode, void *stream);

/* ------------------------------------------------------------------------
 * Persistent variant: n consecutive transitions of every chain in ONE launch
 * -- the `for i in range(n): sampler.sample()` loop of example_script.py:33-34
 * for the same Gaussian.  Bit-identical to n calls of
 * binf_hmc_sample_gauss_f64 (same arithmetic, same order); the state stays in
 * registers between transitions, so HBM sees only the momentum draws in and
 * the recorded states out.
 *
 *   p0        device, [n*C*D]   draw s at p0 + s*C*D
 *   u         device, [n*C]
 *   q_out     device, [C*D]     state after the n-th transition (may be == q0)
 *   samples   device, [(n/thin)*C*D] or NULL: the state after transitions
 *             thin, 2*thin, ... (thin >= 1; thinning as example_script.py:41)
 *   accepted, e_before, e_after   device, [n*C] or NULL (per transition)
 *   n_accepted device, [C] or NULL: += number of accepted transitions
 *   n_adapt   the first n_adapt transitions adapt dt_chain (hmc.py:156-157:
 *             a caller with `counter` samples drawn and adaption limit `lim`
 *             passes max(0, min(n, lim - 1 - counter)))
 * ---------------------------------------------------------------------- */
int32_t binf_hmc_sample_n_gauss_f64(const double *q0, const double *p0,
                                    const double *u, double *q_out,
                                    double *samples, uint8_t *accepted,
                                    int64_t *n_accepted, double *e_before,
                                    double *e_after, double timestep,
                                    double *dt_chain, int64_t C, int64_t D,
                                    int32_t nsteps, int32_t n, int32_t thin,
                                    double k, double x0, int32_t n_adapt,
                                    double uprate, double downrate,
                                    int32_t mode, void *stream);

/* Waves per chain binf_hmc_sample_[n_]gauss_f64 uses for a [C x D] batch: 1, or
 * 2 / 4 for few chains of D = 768 / 1024 (a chain spread over several waves), or
 * 2 / 4 / 8 for 1024 < D <= 8192; 0 if the shape is not covered.  Host function. */
int32_t binf_hmc_gauss_waves_per_chain(int64_t C, int64_t D);

/* ------------------------------------------------------------------------
 * One transition for chains of ANY length -- what binf_hmc_sample_gauss_f64
 * does not cover (D > 8192; lengths whose pairwise tree is deeper than 6).
 * numpy sums long vectors 8192 elements at a time, so the trajectory runs per
 * (chain, 8192-chunk) with the state in registers, the chunk sums are chained
 * per chain, and rejected chains are restored from q0: three launches and
 * 24 D bytes per chain instead of ~3 L launches and 32 D bytes per leapfrog
 * step of the per-step tier; same bits.  Arguments as
 * binf_hmc_sample_gauss_f64, plus
 *   workspace  device scratch of binf_hmc_sample_gauss_big_workspace_bytes(C, D)
 *              bytes (caller-owned; too small or NULL -> BINF_E_ARG)
 * q_out must not overlap q0 or p0 (BINF_E_ALIAS).
 * ---------------------------------------------------------------------- */
int64_t binf_hmc_sample_gauss_big_workspace_bytes(int64_t C, int64_t D);
int32_t binf_hmc_sample_gauss_big_f64(const double *q0, const double *p0,
                                      const double *u, double *q_out,
                                      uint8_t *accepted, int64_t *n_accepted,
                                      double *e_before, double *e_after,
                                      double timestep, double *dt_chain,
                                      int64_t C, int64_t D, int32_t nsteps,
                                      double k, double x0, int32_t adapt,
                                      double uprate, double downrate,
                                      int32_t mode, void *workspace,
                                      int64_t workspace_bytes, void *stream);

/* n consecutive long-chain transitions from one call: the loop
 * `for i in range(n): sampler.sample()` (example_script.py:33-34) for chains of
 * any length.  Transition s writes its proposal straight into its record slot
 * samples[(s + 1) / thin - 1] (or into q_out / a scratch state when it is not
 * recorded), rejected chains are restored from the state the transition read,
 * and transition s + 1 reads what s wrote: 3 launches and 24 D bytes per chain
 * and transition, recorded or not (a loop of single calls copies every recorded
 * state once more).  BIT-IDENTICAL to n calls of binf_hmc_sample_gauss_big_f64
 * (the same kernels).  p0 [n x C x D], u [n x C], accepted / e_before / e_after
 * [n x C], samples [n / thin x C x D] or NULL; the first n_adapt transitions adapt
 * dt_chain.  workspace: binf_hmc_sample_n_gauss_big_workspace_bytes(C, D) bytes
 * (chunk sums + one [C x D] scratch state).  q_out holds the state after
 * transition n.  The _rng form generates the draws in the kernels, transition s
 * under (seed, offset + s): exactly the draws of n calls of
 * binf_hmc_sample_gauss_big_rng_f64 with offsets offset, offset + 1, ...
 * (No persistent kernel: the trajectory kernel moves its 24 D bytes as fast per
 * byte as the persistent kernel of binf_hmc_sample_n_gauss_f64 moves its 16 D;
 * chains longer than a workgroup's registers stream through HBM either way.) */
int64_t binf_hmc_sample_n_gauss_big_workspace_bytes(int64_t C, int64_t D);
int32_t binf_hmc_sample_n_gauss_big_f64(const double *q0, const double *p0,
                                        const double *u, double *q_out, double *samples,
                                        uint8_t *accepted, int64_t *n_accepted,
                                        double *e_before, double *e_after,
                                        double timestep, double *dt_chain, int64_t C,
                                        int64_t D, int32_t nsteps, int32_t n,
                                        int32_t thin, double k, double x0,
                                        int32_t n_adapt, double uprate, double downrate,
                                        int32_t mode, void *workspace,
                                        int64_t workspace_bytes, void *stream);
int32_t binf_hmc_sample_n_gauss_big_rng_f64(const double *q0, double *q_out,
                                            double *samples, uint8_t *accepted,
                                            int64_t *n_accepted, double *e_before,
                                            double *e_after, double timestep,
                                            double *dt_chain, int64_t C, int64_t D,
                                            int32_t nsteps, int32_t n, int32_t thin,
                                            double k, double x0, int32_t n_adapt,
                                            double uprate, double downrate, int32_t mode,
                                            uint64_t seed, uint64_t offset,
                                            int64_t chain_offset, void *workspace,
                                            int64_t workspace_bytes, void *stream);

/* The long-chain transition with its draws generated inside the kernels (one
 * xoshiro128++ stream per lane and (chain, 8192-chunk) for the momentum, one per
 * chain for the acceptance draw; keyed by (seed, offset), a caller advances
 * offset by one per call): binf_hmc_sample_gauss_big_f64 without p0 / u.
 * chain_offset (>= 0) is the GLOBAL index of chain 0 of this call: the streams are
 * keyed by global chain, so a rank that owns chains [s, s + C) of a larger run
 * passes chain_offset = s and draws exactly what the unsharded call draws for them.
 * binf_hmc_gauss_big_rng_draws_f64 writes those draws out instead (p0_out [C*D],
 * u_out [C]); feeding them to binf_hmc_sample_gauss_big_f64 reproduces the fused
 * call bit for bit. */
int32_t binf_hmc_sample_gauss_big_rng_f64(const double *q0, double *q_out,
                                          uint8_t *accepted, int64_t *n_accepted,
                                          double *e_before, double *e_after,
                                          double timestep, double *dt_chain,
                                          int64_t C, int64_t D, int32_t nsteps,
                                          double k, double x0, int32_t adapt,
                                          double uprate, double downrate,
                                          int32_t mode, uint64_t seed,
                                          uint64_t offset, int64_t chain_offset,
                                          void *workspace,
                                          int64_t workspace_bytes, void *stream);
int32_t binf_hmc_gauss_big_rng_draws_f64(double *p0_out, double *u_out, int64_t C,
                                         int64_t D, uint64_t seed, uint64_t offset,
                                         int64_t chain_offset, void *stream);

/* ------------------------------------------------------------------------
 * The same n transitions with the random draws generated INSIDE the kernel:
 * HMCSampler.sample() as the reference defines it, np.random.normal(size=
 * q.shape) ... np.random.uniform() (binf/samplers/hmc.py:146,151), with no
 * momentum buffer in HBM.  Per-lane xoshiro128++ streams seeded from the Philox
 * block (lane's element set, offset) under `seed`, normals by a 1024-layer
 * ziggurat; chain c of the call draws the stream of GLOBAL chain chain_offset + c:
 * deterministic in (seed, offset, global chain, D), independent of the launch
 * geometry, of the batch size C and of how a run is sharded over GPUs (a rank that
 * owns chains [s, s + C) passes chain_offset = s); NOT numpy's MT19937 stream
 * (parity runs inject host draws through binf_hmc_sample_n_gauss_f64).  Transition
 * i of a launch draws from stream position offset + i -- what a single-transition
 * launch at that position draws, so n transitions in one launch equal n launches of
 * one (ABI 5; before, a launch ran on from ONE position) -- and a caller advances
 * `offset` by n per launch.
 * Arguments as binf_hmc_sample_n_gauss_f64 without p0 / u.
 * Supported: the shapes of binf_hmc_sample_n_gauss_f64 (D <= 8192, pairwise
 * tree height <= 6); otherwise BINF_E_UNSUPPORTED (use the stand-alone
 * generators below + binf_hmc_sample_gauss_big_f64).
 * ---------------------------------------------------------------------- */
int32_t binf_hmc_sample_n_gauss_rng_f64(const double *q0, double *q_out,
                                        double *samples, uint8_t *accepted,
                                        int64_t *n_accepted, double *e_before,
                                        double *e_after, double timestep,
                                        double *dt_chain, int64_t C, int64_t D,
                                        int32_t nsteps, int32_t n, int32_t thin,
                                        double k, double x0, int32_t n_adapt,
                                        double uprate, double downrate,
                                        int32_t mode, uint64_t seed,
                                        uint64_t offset, int64_t chain_offset,
                                        void *stream);

/* The draws binf_hmc_sample_n_gauss_rng_f64 consumes for (seed, offset, chain_offset, C, D, n),
 * written out instead of used: p0_out [n*C*D], u_out [n*C].  Feeding them to
 * binf_hmc_sample_n_gauss_f64 reproduces the fused call bit for bit -- the
 * handle by which the fused generator is tested and its stream inspected. */
int32_t binf_hmc_gauss_rng_draws_f64(double *p0_out, double *u_out, int64_t C,
                                     int64_t D, int32_t n, uint64_t seed,
                                     uint64_t offset, int64_t chain_offset,
                                     void *stream);

/* ------------------------------------------------------------------------
 * Generic per-step tier: the pieces of HMCSampler.sample() as separate
 * chain-batched launches, for posteriors whose gradient comes from other code
 * (any plug-in with log_prob / gradient, reference binf/samplers/hmc.py:114,143).
 * ---------------------------------------------------------------------- */

/* Row reductions in numpy's pairwise order, bit-identical to np.sum on each
 * row:  out[c] = scale * np.sum(f(x[c,:])).
 *   op = BINF_ROW_SUM          f(x) = x
 *        BINF_ROW_SUMSQ        f(x) = x*x            (0.5*np.sum(p**2): scale=0.5,
 *                                                     hmc.py:148,150)
 *        BINF_ROW_SUMSQ_SHIFT  f(x) = (x-shift)**2   (binf/pdf/__init__.py:185)
 * (rows longer than numpy's 8192-element buffer are accumulated chunk by chunk,
 * as numpy does).  x device [C*D], out device [C]; any D < 2^31. */
#define BINF_ROW_SUM 0
#define BINF_ROW_SUMSQ 1
#define BINF_ROW_SUMSQ_SHIFT 2
int32_t binf_row_sum_f64(const double *x, double *out, int64_t C, int64_t D,
                         int32_t op, double shift, double scale, void *stream);

/* HMCSampler.sample()'s energy (binf/samplers/hmc.py:143,148,150)
 *   out[c] = -log_prob[c] + 0.5 * np.sum(p[c,:]**2)
 * in one launch (the kinetic row sum in numpy's order, the subtraction as its
 * epilogue; bit-identical to negating, summing and adding separately).
 * p device [C*D], log_prob / out device [C] (out may alias log_prob). */
int32_t binf_hmc_energy_f64(const double *p, const double *log_prob, double *out,
                            int64_t C, int64_t D, void *stream);

/* p[c,:] -= (half ? 0.5*dt : dt) * grad[c,:]     hmc.py:116,120,123
 * dt = dt_chain[c] if dt_chain != NULL else timestep. */
int32_t binf_leapfrog_kick_f64(double *p, const double *grad, double timestep,
                               const double *dt_chain, int32_t half, int64_t C,
                               int64_t D, int32_t mode, void *stream);

/* q[c,:] += p[c,:] * dt                           hmc.py:119,122 */
int32_t binf_leapfrog_drift_f64(double *q, const double *p, double timestep,
                                const double *dt_chain, int64_t C, int64_t D,
                                int32_t mode, void *stream);

/* p[c,:] -= dt * grad[c,:];  q[c,:] += p[c,:] * dt    hmc.py:120 then :119 / :122
 * (one interior leapfrog step after its gradient call; the same roundings as
 * binf_leapfrog_kick_f64 followed by binf_leapfrog_drift_f64, one pass). */
int32_t binf_leapfrog_kick_drift_f64(double *q, double *p, const double *grad,
                                     double timestep, const double *dt_chain,
                                     int64_t C, int64_t D, int32_t mode,
                                     void *stream);

/* out = k * (x - x0): energy gradient of TestHO, binf/pdf/__init__.py:187-191 */
int32_t binf_gauss_grad_f64(const double *x, double *out, double k, double x0,
                            int64_t C, int64_t D, void *stream);

/* out[i] = exp(clip(x[i], -308, 709)): csb.numeric.exp as the reference uses it
 * in the accept test (binf/samplers/hmc.py:10,151) and in
 * AbstractBinfPDF._evaluate (binf/pdf/__init__.py:10,89).  The SAME device
 * function decides every accept test of this library. */
int32_t binf_clipped_exp_f64(const double *x, double *out, int64_t n, void *stream);

/* acc[c] = u[c] < exp(clip(-(e_after[c]-e_before[c]), -308, 709));
 * q_out[c,:] = acc ? q_prop[c,:] : q_old[c,:];  optional step-size adaption of
 * dt_chain as in binf_hmc_sample_gauss_f64.       hmc.py:151-164,188-191
 * n_accepted (device [C] or NULL) += 1 on accept.
 * q_out may be exactly q_prop or exactly q_old. */
int32_t binf_accept_select_f64(const double *q_prop, const double *q_old,
                               const double *e_before, const double *e_after,
                               const double *u, double *q_out, uint8_t *accepted,
                               int64_t *n_accepted, double *dt_chain,
                               int32_t adapt, double uprate,
                               double downrate, int64_t C, int64_t D,
                               void *stream);

/* out[i] = the accept test of (u[i], xe) for EVERY exponent xe within delta[i] / 2 of
 * x[i], where one answer holds for all of them: BINF_ACCEPT_NO (0) or BINF_ACCEPT_YES (1),
 * the flag binf_accept_select_f64 gives for each such xe; BINF_ACCEPT_UNDECIDED (2) where u
 * lies within 2 * delta * e^x + 2^-40 of the threshold, and for every input outside
 * 0 <= u < 1, 0 <= delta <= 2^-21, x finite (NaN included).  The device function by which
 * binf_hmc_sample_n_gauss_f64 decides from energy sums accumulated with one rounding per
 * element when it records no energies; exposed for testing. */
#define BINF_ACCEPT_NO 0
#define BINF_ACCEPT_YES 1
#define BINF_ACCEPT_UNDECIDED 2
int32_t binf_accept_decide_f64(const double *u, const double *x, const double *delta,
                               int32_t *out, int64_t n, void *stream);

/* out[c] = scale * np.sum((x[c,:] - y[:])**2 / w[:]), numpy order; y, w device
 * [D]; w == NULL means no division.  The chi^2 of GaussianErrorModel
 * (binf/example/likelihood.py:57) and the GaussianPrior exponent
 * (binf/example/priors.py:54). */
int32_t binf_row_sumsq_diff_f64(const double *x, const double *y, const double *w,
                                double *out, int64_t C, int64_t D, double scale,
                                void *stream);

/* ------------------------------------------------------------------------
 * Polynomial forward model + Gaussian error model (the reference's example
 * application, BASELINE configs C1/C3/C4).  K coefficients (<= 64), N data.
 *   precision / precision_chain: host scalar, or device [C] per-chain values
 *   (non-NULL wins) -- the Gibbs state's 'precision' variable.
 * ---------------------------------------------------------------------- */

/* out[c,n] = polyval(xs[n], coeffs[c,:]), Horner in numpy's order (bit-exact).
 * ForwardModel._evaluate, binf/example/likelihood.py:24-26.  C <= 65535. */
int32_t binf_poly_forward_f64(const double *coeffs, const double *xs, double *out,
                              int64_t C, int64_t K, int64_t N, void *stream);

/* out[c,n] = (mock[c,n] - ys[n]) * precision_c.
 * GaussianErrorModel._evaluate_gradient, likelihood.py:59-61.  C <= 65535. */
int32_t binf_gauss_err_grad_f64(const double *mock, const double *ys,
                                double precision, const double *precision_chain,
                                double *out, int64_t C, int64_t N, void *stream);

/* out[c] = -0.5*np.sum((mock[c,:]-ys)**2)*precision_c + N*0.5*log(precision_c).
 * GaussianErrorModel._evaluate_log_prob, likelihood.py:54-57. */
int32_t binf_gauss_err_logp_f64(const double *mock, const double *ys,
                                double precision, const double *precision_chain,
                                double *out, int64_t C, int64_t N, void *stream);

/* Likelihood._evaluate_log_prob (binf/pdf/likelihoods.py:141-146) for the
 * polynomial + Gaussian pair, fused: the mock data is never materialised.
 * chi^2 is bit-identical to the numpy path; log() is the device's. */
int32_t binf_poly_gauss_logp_f64(const double *coeffs, const double *xs,
                                 const double *ys, double precision,
                                 const double *precision_chain, double *out,
                                 int64_t C, int64_t K, int64_t N, void *stream);

/* The same log-prob with a per-chain MEMO of chi^2 = np.sum((polyval - ys)**2), the
 * expensive part (a Horner pass over all N data points per chain), which depends on the
 * coefficients alone.  The memo has TWO entries per chain (HMCSampler.sample() evaluates
 * the state and the proposal, hmc.py:148,150, and the next call's state is one of the two
 * whichever way the acceptance test went): memo_coeffs [2 x C x K] / memo_chi2 [2 x C]
 * (caller-owned, device; fill both with NaN before the first use) hold the coefficients
 * a stored chi^2 belongs to; memo_state [2 x C] bytes (zero before the first use) is the
 * memo's bookkeeping: [0..C) 1 = this call reused a stored chi^2 for the chain, [C..2C)
 * the entry it used or refilled.  A chain whose coefficients equal one entry's BIT FOR BIT
 * takes that entry's chi^2; every other chain is summed and replaces the entry it did not
 * use last.  The check runs on the device, chain by chain -- no tensor identities,
 * versions or host synchronisation are involved, so the results are those of
 * binf_poly_gauss_logp_f64 bit for bit whatever happened to the buffers in between.
 * In a Gibbs sweep (binf/samplers/gibbs.py:146-149) the log-prob is asked for the
 * proposal (hmc.py:150), again for the sweep's new coefficients at precision = 1
 * (binf/example/samplers.py:34-41) and once more as the next sweep's E_before
 * (hmc.py:148): one Horner pass instead of three, accepted or not. */
int32_t binf_poly_gauss_logp_memo_f64(const double *coeffs, const double *xs,
                                      const double *ys, double precision,
                                      const double *precision_chain, double *out,
                                      double *memo_coeffs, double *memo_chi2,
                                      uint8_t *memo_state, int64_t C, int64_t K, int64_t N,
                                      void *stream);

/* Likelihood._evaluate_gradient (binf/pdf/likelihoods.py:148-155) for the same
 * pair: out[c,:] = J . ((mock_c - ys) * precision_c) with the Jacobian
 * J = design [K x N] (design[i][n] = xs[n]**i, likelihood.py:28-30), as two
 * chained f64 MFMA products per tile.  workspace: device scratch of
 * binf_poly_gauss_grad_workspace_bytes(C,K,N) bytes (caller-owned; 0 bytes
 * needed -> may be NULL; NULL or too small otherwise -> BINF_E_ARG, the
 * summation order is never changed silently).  The data range is summed in a
 * number of pieces that follows from (C, N), partial sums joined in a fixed
 * order: a call is deterministic, but the same chain evaluated in batches of
 * different size (one GPU vs a shard) can differ at rounding level -- inside
 * the 1e-10 bar the contraction is held to (the reference's BLAS order is not
 * reproducible either). */
int64_t binf_poly_gauss_grad_workspace_bytes(int64_t C, int64_t K, int64_t N);
int32_t binf_poly_gauss_grad_f64(const double *coeffs, const double *design,
                                 const double *ys, double precision,
                                 const double *precision_chain, double *out,
                                 void *workspace, int64_t workspace_bytes,
                                 int64_t C, int64_t K, int64_t N, void *stream);

/* HMCSampler._leapfrog (binf/samplers/hmc.py:92-125) under the force of the
 * polynomial + Gaussian likelihood alone (the example's conditional posterior of
 * the coefficients: its priors are not differentiable, posteriors.py:183), IN
 * PLACE on q = coefficients [C x K] and p [C x K]: per gradient call one launch of
 * the MFMA gradient kernel of binf_poly_gauss_grad_f64 (partial sums over the
 * data splits) and ONE launch that adds the partial sums in split order and
 * applies the kick (hmc.py:116,120,123) and the drift that follows it (:119,122)
 * -- 2 (nsteps + 1) launches from one call instead of ~3 per step through the
 * class stack.  BIT-IDENTICAL to the per-step sequence binf_poly_gauss_grad_f64,
 * binf_leapfrog_kick_f64 (half), binf_leapfrog_drift_f64,
 * binf_leapfrog_kick_drift_f64 ... on the same batch.  (Combining a chain tile
 * inside the gradient launch -- last workgroup, agent-scope release / acquire --
 * was built and measured: 68-130 us per step slower, a tile's 16 x 34 KB of
 * partial sums are too much for one workgroup to read.)  workspace: caller-owned
 * device scratch of binf_poly_leapfrog_workspace_bytes(C, K, N) bytes
 * (mandatory).  timestep / dt_chain, mode as elsewhere. */
int64_t binf_poly_leapfrog_workspace_bytes(int64_t C, int64_t K, int64_t N);
int32_t binf_poly_leapfrog_f64(double *q, double *p, const double *design,
                               const double *ys, double precision,
                               const double *precision_chain, void *workspace,
                               int64_t workspace_bytes, int64_t C, int64_t K,
                               int64_t N, double timestep, const double *dt_chain,
                               int32_t nsteps, int32_t mode, void *stream);

/* ------------------------------------------------------------------------
 * Linear forward models: mock = coeffs . design for ANY constant design matrix
 * [K x N] shared by all chains (Fourier or spline bases, regression on measured
 * covariates, a fixed dictionary); K <= 64, else BINF_E_UNSUPPORTED.  The gradient
 * and the leapfrog of such a model under the Gaussian error model are
 * binf_poly_gauss_grad_f64 / binf_poly_leapfrog_f64 above, which take the design
 * matrix as it is.
 * ------------------------------------------------------------------------ */

/* AbstractForwardModel._evaluate (binf/model/forwardmodels.py:23-28) of a linear
 * model: out[c, n] = sum_k coeffs[c, k] * design[k, n], on the f64 matrix pipe.
 * Used when the error model is not the Gaussian one (or is overridden).  out must
 * not overlap coeffs or design (BINF_E_ALIAS). */
int32_t binf_linear_forward_f64(const double *coeffs, const double *design, double *out,
                                int64_t C, int64_t K, int64_t N, void *stream);

/* Likelihood._evaluate_log_prob (binf/pdf/likelihoods.py:141-146) for a linear
 * forward model (binf/model/forwardmodels.py:23-28) + the Gaussian error model, fused:
 *   out[c] = -0.5 * sum_n (mock[c, n] - ys[n])**2 * tau_c + N * 0.5 * log(tau_c),
 * mock = coeffs . design in f64 MFMA tiles of 16 data points x 16 chains that never
 * leave registers.  The error model's epilogue is that of binf_poly_gauss_logp_f64
 * (same scaling, the device's log, precision per chain if precision_chain != NULL).
 * The data range is summed in pieces whose length follows from N ALONE, partial sums
 * joined in piece order: the summation order of a chain is a function of (K, N) and
 * never of C or of the chain's place in the batch -- a shard of a batch reproduces it
 * bit for bit.  workspace: device scratch of
 * binf_linear_gauss_logp_workspace_bytes(C, K, N) bytes (caller-owned; 0 bytes needed
 * -> may be NULL; NULL or too small otherwise -> BINF_E_ARG).  out and the workspace
 * must not overlap each other or an input (BINF_E_ALIAS). */
int64_t binf_linear_gauss_logp_workspace_bytes(int64_t C, int64_t K, int64_t N);
int32_t binf_linear_gauss_logp_f64(const double *coeffs, const double *design,
                                   const double *ys, double precision,
                                   const double *precision_chain, double *out,
                                   void *workspace, int64_t workspace_bytes,
                                   int64_t C, int64_t K, int64_t N, void *stream);

/* ------------------------------------------------------------------------
 * Generalised linear models on a linear forward model: binomial-logit (logistic
 * regression on y successes of m trials) and Poisson-log (count regression) error
 * terms (csrc/glm_term.hpp, csrc/glm.hip; restated in tests/glm_ref.py; the models in
 * binf_amd/model/glm.py).  Build-defined: the reference has no such error model; the
 * entry points stand in for what a user's error model would run through
 * binf/pdf/likelihoods.py:141-155.  Added within ABI 7: new symbols only.
 *
 * The term, per datum, every operation rounded on its own; eta = mock + offset[n]
 * (offset NULL: + 0.0); the gradient is that of MINUS the log density with respect to
 * the mock datum, the sign of GaussianErrorModel._evaluate_gradient:
 *   BINF_GLM_BINOMIAL_LOGIT, m = trials[n] (NULL: 1.0):
 *     t = exp(-|eta|)   sp = max(eta, 0) + log1p(t)   ll = y * eta - m * sp
 *     s = eta >= 0 ? 1 / (1 + t) : t / (1 + t)        g = m * s - y
 *   BINF_GLM_POISSON_LOG (trials is not read):
 *     e = exp(eta)      ll = y * eta - e              g = e - y
 * IEEE results are left as they fall: a Poisson eta beyond exp's range gives ll = -inf
 * and g = +inf; a binomial term is finite for every finite eta.  The data-only constants
 * (sum_n log C(m_n, y_n); -sum_n lgamma(y_n + 1)) are the caller's, computed once on the
 * host: the fused log-prob takes their sum log_norm and adds it LAST, the element-wise
 * record takes them per datum (lconst [N], NULL: none) and adds each to its ll.
 *
 * binf_glm_pointwise_f64: mock, out_ll, out_grad device [S x N]; ys, trials, offset,
 *   lconst device [N].  One element-wise launch: out_ll[s,n] = ll (+ lconst[n]),
 *   out_grad[s,n] = g.  Either output may be NULL, not both.  It is the error models'
 *   own _evaluate_log_prob (followed by binf_row_sum_f64), their _evaluate_gradient, and
 *   the pointwise record of PSIS-LOO.  S == 0 or N == 0: nothing is done.
 *
 * binf_linear_glm_logp_f64: Likelihood._evaluate_log_prob fused, coeffs [C x K],
 *   design [K x N], K <= 64: out[c] = (sum_n ll[c, n]) + log_norm with mock = coeffs .
 *   design in f64 MFMA tiles of 16 data points x 16 chains that never leave registers
 *   (the loop of binf_linear_gauss_logp_f64).  Summation order: pieces of 1024 data
 *   points; inside a piece lane lk of four sums n = lk, lk + 4, ... ascending, the four
 *   joined as (0 + 1) + (2 + 3); pieces joined in piece order; log_norm last.  A function
 *   of (K, N) alone: a shard of a batch reproduces the batch bit for bit.  workspace:
 *   binf_linear_glm_logp_workspace_bytes(C, K, N) bytes (0 -> may be NULL).
 *
 * binf_linear_glm_grad_f64: Likelihood._evaluate_gradient fused: out[c, i] = sum_n
 *   design[i, n] g[c, n], two chained MFMA products per tile as binf_poly_gauss_grad_f64,
 *   with its data splits (a function of (C, N)), partial sums joined in split order, and
 *   its split of K between the matrix pipe and the VALU; deterministic per call, but the
 *   same chain in batches of different size may differ at rounding level, as there.
 *   workspace: binf_linear_glm_grad_workspace_bytes(C, K, N) bytes (0 -> may be NULL).
 *
 * binf_linear_glm_leapfrog_f64: HMCSampler._leapfrog (binf/samplers/hmc.py:92-125) in
 *   place on q, p [C x K] under the force of ONE such likelihood plus, with has_prior = 1,
 *   one isotropic Gaussian prior's prior_k * (q - prior_x0) (has_prior = 0: the term is
 *   not evaluated).  Per gradient call one gradient launch and one launch for partial
 *   sums + prior + kick + drift: 2 (nsteps + 1) launches.  Bit-identical to the per-step
 *   sequence binf_linear_glm_grad_f64, binf_gauss_grad_f64, binf_sum_terms_f64 (two terms:
 *   either order), kick and drift on the same batch.  timestep, dt_chain and mode as in
 *   binf_poly_leapfrog_f64.  workspace: binf_linear_glm_leapfrog_workspace_bytes(C, K, N)
 *   bytes, always needed.
 *
 * BINF_E_ARG: a NULL required buffer, an unknown family, nsteps < 1, an unknown mode, a
 * has_prior other than 0 / 1, negative sizes, a workspace that is NULL or too small where
 * one is needed (never another summation order).  BINF_E_UNSUPPORTED: K > 64, C > 65535 *
 * 64, N > 2^31 - 17, N == 0 with C > 0 (fused entry points); N >= 2^31 - 1 or more than
 * 2^53 elements (pointwise).  BINF_E_ALIAS: an output or the workspace that overlaps an
 * input, another output or the workspace.  Refusals come before anything is touched;
 * everything is stream-ordered and graph-capturable; no atomics.
 * ---------------------------------------------------------------------- */
#define BINF_GLM_BINOMIAL_LOGIT 0
#define BINF_GLM_POISSON_LOG    1

int32_t binf_glm_pointwise_f64(const double *mock, const double *ys, const double *trials,
                               const double *offset, const double *lconst, int32_t family,
                               double *out_ll, double *out_grad, int64_t S, int64_t N,
                               void *stream);
int64_t binf_linear_glm_logp_workspace_bytes(int64_t C, int64_t K, int64_t N);
int32_t binf_linear_glm_logp_f64(const double *coeffs, const double *design, const double *ys,
                                 const double *trials, const double *offset, int32_t family,
                                 double log_norm, double *out, void *workspace,
                                 int64_t workspace_bytes, int64_t C, int64_t K, int64_t N,
                                 void *stream);
int64_t binf_linear_glm_grad_workspace_bytes(int64_t C, int64_t K, int64_t N);
int32_t binf_linear_glm_grad_f64(const double *coeffs, const double *design, const double *ys,
                                 const double *trials, const double *offset, int32_t family,
                                 double *out, void *workspace, int64_t workspace_bytes,
                                 int64_t C, int64_t K, int64_t N, void *stream);
int64_t binf_linear_glm_leapfrog_workspace_bytes(int64_t C, int64_t K, int64_t N);
int32_t binf_linear_glm_leapfrog_f64(double *q, double *p, const double *design,
                                     const double *ys, const double *trials,
                                     const double *offset, int32_t family, int32_t has_prior,
                                     double prior_k, double prior_x0, void *workspace,
                                     int64_t workspace_bytes, int64_t C, int64_t K, int64_t N,
                                     double timestep, const double *dt_chain, int32_t nsteps,
                                     int32_t mode, void *stream);

/* ------------------------------------------------------------------------
 * Negative-binomial regression (NB2: mean mu = exp(eta), variance mu + mu^2 / phi) on the
 * same fused path (csrc/glm_term.hpp, csrc/glm.hip, csrc/negbin.hip; restated in
 * tests/negbin_ref.py; the model in binf_amd/model/glm.py).  Build-defined, as the block
 * above.  Added within ABI 7: new symbols only; the entry points above refuse family 2.
 *
 * The dispersion is per chain: log_dispersion[c] = lam_c = log(phi_c).  Every kernel
 * computes phi = exp(lam) itself.  One datum's log density is
 *   y z - (y + phi) softplus(z) + sum_{j<y} log(phi + j) - lgamma(y + 1),   z = eta - lam.
 * The term (per datum, every operation rounded on its own):
 *     z = eta - lam   m = y + phi   then the BINF_GLM_BINOMIAL_LOGIT lines at (z, y, m):
 *     ll = y * z - m * sp(z)        g = m * s(z) - y
 * The count term (binf_negbin_count_term_f64) is the third part summed over the data,
 *   out_chain[c] = (sum_{j=0}^{ymax-1} tail_counts[j] * log(phi_c + j)) + log_norm,
 * tail_counts[j] = #{n : ys[n] > j} (device doubles, exact integers), log_norm the host's
 * -sum_n lgamma(ys[n] + 1); and, for the record, out_prefix[c][k] = sum_{j<values[k]}
 * log(phi_c + j) at the distinct values of ys, ascending (device doubles).  Orders, both a
 * function of the table alone: out_chain -- thread t of 256 sums j = t, t + 256, ...
 * ascending from 0.0, a wave's 64 sums by the butterfly x += x[lane ^ o], o = 1 .. 32, the
 * four waves as (0 + 1) + (2 + 3), log_norm last (ymax = 0: log_norm itself); out_prefix --
 * one running sum over j = 0, 1, ... from 0.0, written when j reaches values[k].  Either
 * output may be NULL, not both.
 *
 * Domain of lam: REGULAR is -708.0 <= lam <= 709.0 (phi a normal, finite double).  A chain
 * outside it (NaN included) has log-prob -inf (out_chain, the fused log-prob and out_ll);
 * its term, and so its gradient and its leapfrog, are evaluated at the nearer end of the
 * range: never NaN for finite eta.  Other chains of the launch keep their bits.
 *
 * binf_negbin_pointwise_f64: mock, out_ll, out_grad [S x N]; row s under log_dispersion[s].
 *   out_ll = ll, then + prefix[s][prefix_index[n]] (prefix [S x J] with prefix_index [N],
 *   both or neither; an index outside [0, J) is clamped), then + lconst[n] (NULL: none).
 * binf_linear_negbin_logp_f64 / _grad_f64 / _leapfrog_f64: as the binf_linear_glm_ entry
 *   points without trials and family, with log_dispersion [C]; the log-prob adds
 *   log_norm_chain[c] (out_chain above) LAST where the others add log_norm, in the
 *   finishing launch too.  Summation orders, data splits, K limits and workspaces are those
 *   of the binf_linear_glm_ entry points: the same _workspace_bytes functions apply.
 *
 * Refusals as in the block above, before anything is touched.  BINF_E_UNSUPPORTED also
 * for ymax > 2^20 or J > 2^20 + 1.  Stream-ordered, graph-capturable, no atomics.
 * ---------------------------------------------------------------------- */
#define BINF_GLM_NEGBIN_LOG 2

int32_t binf_negbin_count_term_f64(const double *log_dispersion, const double *tail_counts,
                                   int64_t ymax, double log_norm, double *out_chain,
                                   const double *values, int64_t J, double *out_prefix,
                                   int64_t C, void *stream);
int32_t binf_negbin_pointwise_f64(const double *mock, const double *ys, const double *offset,
                                  const double *log_dispersion, const double *prefix,
                                  const int32_t *prefix_index, const double *lconst,
                                  double *out_ll, double *out_grad, int64_t S, int64_t N,
                                  int64_t J, void *stream);
int32_t binf_linear_negbin_logp_f64(const double *coeffs, const double *design, const double *ys,
                                    const double *offset, const double *log_dispersion,
                                    const double *log_norm_chain, double *out, void *workspace,
                                    int64_t workspace_bytes, int64_t C, int64_t K, int64_t N,
                                    void *stream);
int32_t binf_linear_negbin_grad_f64(const double *coeffs, const double *design, const double *ys,
                                    const double *offset, const double *log_dispersion,
                                    double *out, void *workspace, int64_t workspace_bytes,
                                    int64_t C, int64_t K, int64_t N, void *stream);
int32_t binf_linear_negbin_leapfrog_f64(double *q, double *p, const double *design,
                                        const double *ys, const double *offset,
                                        const double *log_dispersion, int32_t has_prior,
                                        double prior_k, double prior_x0, void *workspace,
                                        int64_t workspace_bytes, int64_t C, int64_t K,
                                        int64_t N, double timestep, const double *dt_chain,
                                        int32_t nsteps, int32_t mode, void *stream);

/* One HMCSampler.sample() (binf/samplers/hmc.py:136-164,183-191) for every
 * chain on the example's polynomial posterior with a SMALL or MEDIUM data set
 * (K <= 16 coefficients; N <= 1024 data points with a pairwise tree of height
 * <= 3 -- every N <= 920 and the multiples of 8 up to 1024; a chain's data are
 * spread over a group of 8 << H lanes, 8 lanes up to 128 points, one wave from
 * 513; mode | BINF_MODE_LANE_PER_CHAIN: one lane per chain, N <= 128; else
 * BINF_E_UNSUPPORTED), the whole transition in one launch (the per-step tier is
 * launch-bound there):
 *   log p(theta) = [lp_pre] + {prior, likelihood in the order prior_first says} + [lp_post]
 *   likelihood = -0.5 * sum((polyval(xs, theta) - ys)**2) * precision + N/2 * log(precision)
 *                (binf/example/likelihood.py:24-26,54-57; precision per chain if
 *                precision_chain != NULL)
 *   prior      = -0.5 * sum((theta - prior_means)**2 / prior_vars)
 *                (binf/example/priors.py:49-54; NULL, NULL = no prior)
 *   lp_pre / lp_post [C] or NULL: the posterior's theta-independent component
 *                terms that come before / after in its summation order
 *                (binf/pdf/posteriors.py:147-151).
 * The force is the likelihood's gradient only (the prior is registered
 * non-differentiable, posteriors.py:183).  Energies follow numpy's summation
 * order and are bit-identical to the per-step tier's; the force is an FMA dot
 * product (tolerance, like the MFMA path).  Other arguments as
 * binf_hmc_sample_gauss_f64. */
int32_t binf_hmc_sample_poly_f64(const double *q0, const double *p0,
                                 const double *u, double *q_out,
                                 uint8_t *accepted, int64_t *n_accepted,
                                 double *e_before, double *e_after,
                                 const double *xs, const double *ys,
                                 double precision, const double *precision_chain,
                                 const double *prior_means, const double *prior_vars,
                                 int32_t prior_first, const double *lp_pre,
                                 const double *lp_post, double timestep,
                                 double *dt_chain, int64_t C, int64_t K,
                                 int64_t N, int32_t nsteps, int32_t adapt,
                                 double uprate, double downrate, int32_t mode,
                                 void *stream);

/* ------------------------------------------------------------------------
 * The generic chain-rule contraction of the Likelihood plug-in surface,
 * Likelihood._evaluate_gradient (binf/pdf/likelihoods.py:148-155):
 *     return dfm.dot(emgrad)
 * for any forward model without a fused kernel of its own.
 *   batched == 0: jacobian [K x N], shared by all chains (linear forward models;
 *                 forwardmodels.py:23-28) -- two-operand f64 MFMA tiles;
 *   batched != 0: jacobian [C x K x N], one per chain -- streamed row products.
 *   emgrad [C x N] (error_model.gradient(mock_data=...), likelihoods.py:152-153),
 *   out [C x K]:  out[c,k] = sum_n jacobian[(c,) k, n] * emgrad[c, n].
 * The reference's BLAS summation order is not reproducible; this contraction is
 * held to 1e-10 * sum_n |J||r| (tests/poly_bounds.py).  Its own order depends on
 * (K, N) only: deterministic, and the same for any number of chains.
 * ---------------------------------------------------------------------- */
int32_t binf_jacobian_contract_f64(const double *jacobian, const double *emgrad,
                                   double *out, int64_t C, int64_t K, int64_t N,
                                   int32_t batched, void *stream);

/* out[i] = ((t_0[i] + t_1[i]) + t_2[i]) + ... : the Posterior's sums over its
 * components, Posterior._evaluate_log_prob (numpy.sum of a short list: sequential,
 * binf/pdf/posteriors.py:147-151) and _evaluate_gradient (posteriors.py:173-187),
 * in ONE launch and in the order given (the build's order: sorted component
 * name).  terms: HOST array of n_terms (<= 16) device vectors of n elements; a
 * NULL entry t stands for the host scalar scalars[t] (a component whose log-prob
 * is a Python float).  out may be one of the terms. */
int32_t binf_sum_terms_f64(const double *const *terms, const double *scalars,
                           int32_t n_terms, double *out, int64_t n, void *stream);

/* The same sum with a third kind of term: broadcast[t] != 0 (HOST array of n_terms
 * flags, or null = none) marks terms[t] as a pointer to ONE device double used for
 * every element -- a component whose log-prob is a 0-dim device tensor (e.g. the
 * GammaPrior of a precision shared by all chains) enters the sum without a device ->
 * host read-back.  A broadcast term must not lie inside out (BINF_E_ALIAS). */
int32_t binf_sum_terms_bcast_f64(const double *const *terms, const double *scalars,
                                 const uint8_t *broadcast, int32_t n_terms, double *out,
                                 int64_t n, void *stream);

/* ------------------------------------------------------------------------
 * n sweeps of the example's Gibbs loop in ONE launch:
 *     for i in range(n): gips.sample()          example_script.py:33-34
 * around GibbsSampler.sample (binf/samplers/gibbs.py:136-151; alphabetical
 * sweep: coefficients, then precision), for every chain, with a chain's state
 * in registers between the sweeps.  Per sweep and chain:
 *   coefficients  move == BINF_MOVE_HMC:  HMCSampler.sample (hmc.py:136-164,
 *                   183-191) on the conditional posterior of the coefficients
 *                   -- exactly the transition of binf_hmc_sample_poly_f64 with
 *                   precision_chain = the chain's current precision;
 *                 move == BINF_MOVE_RWMC: RWMCSampler.sample
 *                   (binf/example/samplers.py:78-92): proposal = state + change,
 *                   accept iff u < np.exp(lp_new - lp_old) (numpy's exp);
 *   precision     GammaSampler.sample (samplers.py:27-51):
 *                   rate = 0.5 * chi2(coefficients) + gamma_rate
 *                   precision = g / rate,  g ~ Gamma(gamma_shape, 1).
 * The conditional posterior of the coefficients is
 *   [gp] + {prior, likelihood in the order prior_first says} + [gp]
 *   gp = (gp_shape - 1) * log(precision) - precision * gp_rate: the GammaPrior
 *   term (binf/example/priors.py:23-25; a constant of the move), added first
 *   (gp_where == 1), last (2) or absent (0).
 * Draws: p0 / u / g supplied ([n x C x K], [n x C], [n x C]; parity with a host
 * stream), or NULL = generated in place from the Philox streams of binf_rng_*:
 *   p0[i][c][k] = element (chain_offset + c) * K + k of
 *                 binf_rng_normal_zig_f64 (zig != 0) / binf_rng_normal_f64 under
 *                 (seed_m, off_m + i * stride_m)          (HMC), or
 *                 -stepsize + 2 stepsize * (that element of binf_rng_uniform_f64)
 *                 as binf_rwmc_propose_f64 forms it         (RWMC);
 *   u[i][c]     = element chain_offset + c of binf_rng_uniform_f64 (seed_u, off_u + i * stride_u);
 *   g[i][c]     = element chain_offset + c of binf_rng_gamma_f64 (gamma_shape; seed_g, off_g + i * stride_g)
 *                 (generated only for gamma_shape >= 1, else BINF_E_UNSUPPORTED).
 * With samplers/rng.py:DeviceRNG serving all three: off_u = off_m + 1, off_g =
 * off_m + 2, strides 130 -- n sweeps then draw what n single sweeps draw.
 * Results are BIT-IDENTICAL to n single sweeps through binf_hmc_sample_poly_f64
 * (or binf_rwmc_*), binf_poly_gauss_logp_f64 and binf_gamma_precision_update_f64
 * with the same draws.  Records: the state after sweeps thin, 2 thin, ...
 * K <= 16, N <= 1024 with a pairwise tree of height <= 3, as
 * binf_hmc_sample_poly_f64.  struct_size = sizeof(binf_gibbs_poly_args)
 * (layout check; mismatch -> BINF_E_ARG).
 * ---------------------------------------------------------------------- */
#define BINF_MOVE_HMC  0
#define BINF_MOVE_RWMC 1
typedef struct binf_gibbs_poly_args {
    uint64_t struct_size;
    /* state, device */
    const double *coefficients;   /* [C x K] start                                  */
    const double *precision;      /* [C]     start                                  */
    double *coefficients_out;     /* [C x K] after sweep n; may be `coefficients`   */
    double *precision_out;        /* [C]     after sweep n; may be `precision`      */
    double *rec_coefficients;     /* [n / thin x C x K] or NULL                     */
    double *rec_precision;        /* [n / thin x C] or NULL                         */
    uint8_t *accepted;            /* [n x C] or NULL: the move's accept flags       */
    int64_t *n_accepted;          /* [C] or NULL, += accepted moves                 */
    double *e_before;             /* [n x C] or NULL (HMC)                          */
    double *e_after;              /* [n x C] or NULL (HMC)                          */
    /* model, device */
    const double *xs;             /* [N] */
    const double *ys;             /* [N] */
    const double *prior_means;    /* [K] or NULL (then prior_vars NULL too)         */
    const double *prior_vars;     /* [K] */
    /* supplied draws, device, or NULL */
    const double *p0;
    const double *u;
    const double *g;
    double *dt_chain;             /* [C] or NULL: per-chain HMC step sizes (in/out)  */
    double timestep;              /* HMC step size when dt_chain == NULL            */
    double uprate, downrate;      /* hmc.py:188-191                                  */
    double stepsize;              /* RWMC half-width                                 */
    double gp_shape, gp_rate;     /* GammaPrior term of the coefficient conditional  */
    double gamma_shape;           /* 0.5 N + prior.shape - 1, samplers.py:27-32       */
    double gamma_rate;            /* prior.rate of the precision conditional         */
    int64_t C, K, N;
    int64_t chain_offset;
    uint64_t seed_m, off_m, stride_m;
    uint64_t seed_u, off_u, stride_u;
    uint64_t seed_g, off_g, stride_g;
    int32_t move;                 /* BINF_MOVE_*                                     */
    int32_t mode;                 /* BINF_MODE_EXACT / BINF_MODE_FMA (HMC)           */
    int32_t nsteps;               /* leapfrog steps (HMC)                            */
    int32_t n;                    /* sweeps                                          */
    int32_t thin;
    int32_t n_adapt;              /* the first n_adapt HMC transitions adapt dt_chain */
    int32_t prior_first;
    int32_t gp_where;             /* 0 / 1 / 2, see above                            */
    int32_t zig;                  /* generated momenta: ziggurat (1) or Box-Muller (0) */
    int32_t keep_precision;       /* != 0: no precision draw -- n moves of the coefficients
                                     alone under a FIXED precision: n HMCSampler.sample()
                                     calls on the conditional posterior (g and the gamma
                                     arguments are ignored)                              */
} binf_gibbs_poly_args;
int32_t binf_gibbs_poly_sample_n_f64(const binf_gibbs_poly_args *args, void *stream);

/* ------------------------------------------------------------------------
 * The resident kernels of a LINEAR forward model (binf/model/forwardmodels.py:23-33
 * inside binf/pdf/likelihoods.py:141-155): mock[c, n] = sum_k theta[c, k] design[k, n]
 * with the caller's design matrix [K x N] (row-major, shared by all chains) in place
 * of the polynomial's abscissae.  A chain's state stays on chip for a whole
 * transition / for n Gibbs sweeps; the design matrix is staged once per workgroup in
 * LDS (csrc/linear_chain_kernel.hpp).
 *
 * binf_linear_resident_supported(K, N): 1 if the two entry points below cover the
 * shape -- 1 <= K <= 16, 0 <= N <= 1024 with a pairwise tree of height <= 3 (every
 * N <= 920 and the multiples of 8 up to 1024) -- else 0.  The one place these limits
 * are written down: callers ask, they do not repeat them.
 *
 * binf_hmc_sample_linear_f64: one HMCSampler.sample() (binf/samplers/hmc.py:136-164,
 * 183-191) for every chain; the arguments, the log-probability's composition and the
 * refusals are those of binf_hmc_sample_poly_f64 with `design` [K x N] in place of
 * `xs` (mode: BINF_MODE_EXACT or BINF_MODE_FMA; there is no one-lane-per-chain
 * layout).
 *
 * binf_gibbs_linear_sample_n_f64: n sweeps (coefficients by HMC or RWMC, then the
 * conjugate precision draw) in ONE launch; binf_gibbs_linear_args is
 * binf_gibbs_poly_args field for field with `design` in place of `xs`, and every
 * field means what it means there (struct_size, keep_precision, both moves, supplied
 * or generated draws at the same stream positions, chain_offset, records, adaption).
 *
 * Arithmetic contract of both:
 *   mock      ONE fixed chain over k: design[0][n] * theta[0], then
 *             fma(design[k][n], theta[k], .) for k = 1, 2, ... -- in the energy and in
 *             the force, in both modes.  (The reference's BLAS order is not
 *             reproducible: energies are held to the rounding bound of a K-term dot
 *             product, not to bits.)
 *   chi^2, prior, kinetic energy   numpy's pairwise summation order;
 *   force     per-lane partial sums over the lane's data + an xor butterfly over the
 *             chain's lanes;
 *   every order is a function of (K, N) ALONE -- never of C, of a chain's place in
 *   the batch or of chain_offset: a shard, a permutation or a batch of one give a
 *   chain the same bits.  n sweeps in one launch are BIT-IDENTICAL to n launches of
 *   one sweep, and generated draws to the same launch fed binf_rng_* output.
 *   A non-finite coefficient poisons its own chain only: that chain's move is
 *   rejected and its state kept.
 * Caller owns every buffer; nothing is allocated; BINF_E_ARG / BINF_E_ALIAS /
 * BINF_E_UNSUPPORTED are answered before any launch; C == 0 is not an error.
 * Added within ABI 7: new symbols only, no existing signature or struct changed, so
 * a caller built against the earlier ABI 7 header keeps working and the version
 * number, which guards CHANGED contracts, stays.
 * ---------------------------------------------------------------------- */
int32_t binf_linear_resident_supported(int64_t K, int64_t N);
int32_t binf_hmc_sample_linear_f64(const double *q0, const double *p0,
                                   const double *u, double *q_out,
                                   uint8_t *accepted, int64_t *n_accepted,
                                   double *e_before, double *e_after,
                                   const double *design, const double *ys,
                                   double precision, const double *precision_chain,
                                   const double *prior_means, const double *prior_vars,
                                   int32_t prior_first, const double *lp_pre,
                                   const double *lp_post, double timestep,
                                   double *dt_chain, int64_t C, int64_t K,
                                   int64_t N, int32_t nsteps, int32_t adapt,
                                   double uprate, double downrate, int32_t mode,
                                   void *stream);
typedef struct binf_gibbs_linear_args {
    uint64_t struct_size;
    /* state, device */
    const double *coefficients;   /* [C x K] start                                  */
    const double *precision;      /* [C]     start                                  */
    double *coefficients_out;     /* [C x K] after sweep n; may be `coefficients`   */
    double *precision_out;        /* [C]     after sweep n; may be `precision`      */
    double *rec_coefficients;     /* [n / thin x C x K] or NULL                     */
    double *rec_precision;        /* [n / thin x C] or NULL                         */
    uint8_t *accepted;            /* [n x C] or NULL: the move's accept flags       */
    int64_t *n_accepted;          /* [C] or NULL, += accepted moves                 */
    double *e_before;             /* [n x C] or NULL (HMC)                          */
    double *e_after;              /* [n x C] or NULL (HMC)                          */
    /* model, device */
    const double *design;         /* [K x N] */
    const double *ys;             /* [N] */
    const double *prior_means;    /* [K] or NULL (then prior_vars NULL too)         */
    const double *prior_vars;     /* [K] */
    /* supplied draws, device, or NULL */
    const double *p0;
    const double *u;
    const double *g;
    double *dt_chain;             /* [C] or NULL: per-chain HMC step sizes (in/out)  */
    double timestep;              /* HMC step size when dt_chain == NULL            */
    double uprate, downrate;      /* hmc.py:188-191                                  */
    double stepsize;              /* RWMC half-width                                 */
    double gp_shape, gp_rate;     /* GammaPrior term of the coefficient conditional  */
    double gamma_shape;           /* 0.5 N + prior.shape - 1, samplers.py:27-32       */
    double gamma_rate;            /* prior.rate of the precision conditional         */
    int64_t C, K, N;
    int64_t chain_offset;
    uint64_t seed_m, off_m, stride_m;
    uint64_t seed_u, off_u, stride_u;
    uint64_t seed_g, off_g, stride_g;
    int32_t move;                 /* BINF_MOVE_*                                     */
    int32_t mode;                 /* BINF_MODE_EXACT / BINF_MODE_FMA (HMC)           */
    int32_t nsteps;               /* leapfrog steps (HMC)                            */
    int32_t n;                    /* sweeps                                          */
    int32_t thin;
    int32_t n_adapt;              /* the first n_adapt HMC transitions adapt dt_chain */
    int32_t prior_first;
    int32_t gp_where;             /* 0 / 1 / 2, as binf_gibbs_poly_args              */
    int32_t zig;                  /* generated momenta: ziggurat (1) or Box-Muller (0) */
    int32_t keep_precision;       /* != 0: no precision draw, as binf_gibbs_poly_args */
} binf_gibbs_linear_args;
int32_t binf_gibbs_linear_sample_n_f64(const binf_gibbs_linear_args *args, void *stream);

/* GammaPrior._evaluate_log_prob (binf/example/priors.py:10-25), one value per chain:
 *   out[c] = (shape - 1) * log(precision[c]) - precision[c] * rate
 * (each operation rounded on its own, as the numpy / torch expression).
 * precision / out device [C] (out may alias precision). */
int32_t binf_gamma_logp_f64(const double *precision, double shape, double rate,
                            double *out, int64_t C, void *stream);

/* Conjugate precision draw, GammaSampler.sample (binf/example/samplers.py:34-51):
 * out[c] = g[c] / (-lp_unit[c] + prior_rate), g = supplied Gamma(shape) variates,
 * lp_unit = likelihood log-prob evaluated at precision = 1. */
int32_t binf_gamma_precision_update_f64(const double *g, const double *lp_unit,
                                        double prior_rate, double *out, int64_t C,
                                        void *stream);

/* ------------------------------------------------------------------------
 * Random-walk Metropolis subsampler, RWMCSampler.sample
 * (binf/example/samplers.py:78-92), as two launches around the pdf's evaluation
 * of the proposal.  Draws: supplied by the caller (parity with the reference's
 * np.random stream) or, when the pointer is NULL, generated from the Philox
 * stream of binf_rng_uniform_f64 under (seed, offset), keyed by GLOBAL index
 * (chain_offset = global index of chain 0 of this call).
 *
 * binf_rwmc_propose_f64 (samplers.py:81-83):
 *   proposal[c,k] = state[c,k] + change[c,k]
 *   change == NULL: change[c,k] = -stepsize + (stepsize - -stepsize) * U, U =
 *   element (chain_offset + c) * K + k of the uniform stream (seed, offset) --
 *   np.random.uniform(low=-stepsize, high=stepsize) as legacy numpy forms it.
 *   proposal may be exactly state (in place).
 *
 * binf_rwmc_accept_f64 (samplers.py:84-90):
 *   acc[c] = u[c] < np.exp(-(E_new[c] - E_old[c])),  E = -log_prob: lp_old / lp_new
 *   are the LOG-PROBABILITIES the pdf returned ([C]); numpy's exp, not csb's
 *   clipped one (overflow -> inf accepts, NaN rejects).
 *   u == NULL: u[c] = element chain_offset + c of the uniform stream (seed, offset).
 *   state_out[c,:] = acc ? proposal[c,:] : state[c,:]   (exactly proposal, exactly
 *   state, or disjoint);  accepted [C] or NULL;  n_accepted [C] or NULL, += acc
 *   (samplers.py:88).
 * ---------------------------------------------------------------------- */
int32_t binf_rwmc_propose_f64(const double *state, const double *change,
                              double *proposal, double stepsize, int64_t C,
                              int64_t K, uint64_t seed, uint64_t offset,
                              int64_t chain_offset, void *stream);
int32_t binf_rwmc_accept_f64(const double *proposal, const double *state,
                             const double *lp_old, const double *lp_new,
                             const double *u, double *state_out,
                             uint8_t *accepted, int64_t *n_accepted, int64_t C,
                             int64_t K, uint64_t seed, uint64_t offset,
                             int64_t chain_offset, void *stream);

/* ------------------------------------------------------------------------
 * Replica exchange between neighbouring slots of a tempered ladder (build-defined:
 * the reference has the hooks such a scheme drives, binf/samplers/hmc.py:171-176 and
 * binf/samplers/gibbs.py:117,143-144, and no exchange of its own).  Two launches
 * around the pdf's evaluation of the exchanged states.  Added within ABI 7: new
 * symbols only.
 *
 * C = n_ladders * R chains; chain c is slot r = c % R of ladder c / R.  parity in
 * {0, 1}: slot r is the LOWER member of the pair (r, r + 1) iff r >= parity,
 * (r - parity) is even and r + 1 < R; partner(c) is the other member of c's pair, and c
 * itself for a chain without one.  x, out device [C x D] (any 8-byte alignment; rows
 * that are 16-byte aligned in both move with 16-byte accesses).
 *
 * binf_replica_gather_f64:
 *   out[c,:] = x[partner(c),:]          (unpaired chains copy themselves)
 *
 * binf_replica_swap_f64: for a pair (i, j = i + 1), with lp_own[c] = log p_c(x_c) and
 *   lp_swapped[c] = log p_c(x_partner(c)) (device [C]),
 *     delta  = (lp_swapped[i] + lp_swapped[j]) - (lp_own[i] + lp_own[j])
 *              (three roundings, in this order)
 *     accept = u < exp(clip(delta, -308, 709))    (the accept test of every HMC kernel
 *              here, hmc.py:151 + csb.numeric.exp; NaN rejects)
 *   u [C] supplied: the pair reads u[i].  u == NULL: element chain_offset + i of the
 *   uniform stream (seed, offset) of binf_rng_uniform_f64 (the convention of
 *   binf_rwmc_accept_f64); chain_offset = global index of chain 0 of this call, a
 *   multiple of R (ladders are never split).
 *   out[c,:]    = accepted(pair of c) ? x[partner(c),:] : x[c,:]
 *   accepted[c] = 1 for BOTH members of an accepted pair, 0 otherwise (unpaired: 0); [C]
 *   n_attempted[i] += 1, n_accepted[i] += accepted at the LOWER member i only ([C]
 *                 each; either may be NULL)
 *   walker      NULL or [C]: the two entries of an accepted pair are exchanged in place
 *                 (by the lower member's thread group; pairs are disjoint), so a caller
 *                 can follow a walker through the slots
 *   D == 0 makes the decision only; x and out may then be NULL.
 *
 * Both: C == 0 returns 0 without a launch.  BINF_E_ARG: a negative size, R < 1,
 * C % R != 0, parity outside {0, 1}, chain_offset < 0 or not a multiple of R, a NULL
 * required buffer.  BINF_E_ALIAS: any overlap of out with x (a partner's row is read
 * after its own chain may have been written).  Refusals come before anything is touched.
 * ---------------------------------------------------------------------- */
int32_t binf_replica_gather_f64(const double *x, double *out, int64_t C, int64_t D,
                                int64_t R, int32_t parity, void *stream);
int32_t binf_replica_swap_f64(const double *x, const double *lp_own,
                              const double *lp_swapped, const double *u, double *out,
                              uint8_t *accepted, int64_t *n_attempted,
                              int64_t *n_accepted, int64_t *walker, int64_t C,
                              int64_t D, int64_t R, int32_t parity, uint64_t seed,
                              uint64_t offset, int64_t chain_offset, void *stream);

/* ------------------------------------------------------------------------
 * Free-energy differences from a tempered ladder: the work record of a swap round and
 * Bennett's acceptance ratio (BAR) over a record of rounds (build-defined, as the exchange
 * above).  Added within ABI 7: new symbols only.
 *
 * binf_replica_work_f64: with the pairing, lp_own and lp_swapped of binf_replica_swap_f64,
 *   w_out[c] = lp_swapped[c] - lp_own[partner(c)]     a paired chain (one subtraction)
 *   w_out[c] = quiet NaN                              a chain without a partner
 * device [C] each.  For the pair (r, r + 1) of a ladder, i the chain of slot r:
 *   u = w[i]     = log p_r(x) - log p_{r+1}(x)  at the draw x of slot r + 1,
 *   v = w[i + 1] = log p_{r+1}(y) - log p_r(y)  at the draw y of slot r.
 * C == 0 returns 0 without a launch.  BINF_E_ARG: C < 0, R < 1, C % R != 0, parity outside
 * {0, 1}, a NULL buffer.  BINF_E_ALIAS: w_out overlapping an input.  A refused call leaves
 * w_out untouched.
 *
 * binf_free_energy_bar_f64: work is a record of T such rows, row t at work + t * stride_t
 * (elements; unit inner stride; read in place), row 0 written in round first_round of
 * alternating parity: row t holds the pair (r, r + 1) iff ((first_round + t) & 1) == (r & 1).
 * G divides n_ladders = C / R; group g is the ladders [g * n_ladders / G, (g + 1) * n_ladders
 * / G).  One independent problem per (g, r), r < R - 1, index g * (R - 1) + r, over the
 * n = T_r * n_ladders / G samples u and as many v of that pair in that group (T_r rows of
 * the pair's parity), in (row, ladder) order.  Outputs, device [G x (R - 1)] each:
 *   delta_fwd = (M + log(sum exp(u - M))) - log n   the exponential average of u
 *   delta_rev = -((M + log(sum exp(v - M))) - log n)
 *   delta     the root of g(D) = sum sigma(v + D) - sum sigma(u - D): the BAR estimate of
 *             log Z_r - log Z_{r+1}, Z_r = integral of exp(log_prob_r)
 *   info      S = sum over u and v of sigma (1 - sigma) at delta: the iid variance of delta
 *             is 1 / S - 2 / n, the overlap S / n
 *   n, n_invalid (int64), status (int32, BINF_FE_*)
 * with t = exp(-|z|), sigma(z) = z >= 0 ? 1 / (1 + t) : t / (1 + t), sigma (1 - sigma) =
 * t / ((1 + t) (1 + t)).  Sums: samples are cut into chunks of binf_free_energy_chunk()
 * counted from the start of the problem; in a chunk, thread j of 256 adds its samples j,
 * j + 256, ... in order (for info: u's term, then v's), the 64 lanes of a wave join as a
 * balanced tree over neighbouring lanes, the four waves in order; a problem's chunks add in
 * ascending order, the exponential sums as S_c * exp(m_c - M) with m_c the chunk's maximum.
 * The root is bracketed by lo = min(min u, -max v), hi = max(max u, -min v) over the finite
 * samples, started at (delta_fwd + delta_rev) / 2 where that lies inside (else the
 * midpoint), and moved by Newton steps D - g / S that must fall strictly inside the bracket
 * and be at most half the step before, else by bisection; it is final when g == 0 or D
 * stops changing.  The outputs are a pure function of the samples: independent of the row
 * stride, of G and of a group's place in the batch.  The call reads one 4-byte flag back
 * per batch of iterations and returns with the stream drained.
 *   -inf is a sample of weight 0 (sigma = 0, outside the bracket).
 *   BINF_FE_INVALID     a +inf or NaN in a paired position (counted in n_invalid): the
 *                       problem's floating outputs are NaN
 *   BINF_FE_NO_FINITE   no finite sample: delta_fwd = -inf, delta_rev = +inf, delta, info NaN
 *   BINF_FE_ONE_SIDED   no finite u: delta_fwd = delta = -inf; no finite v: delta_rev =
 *                       delta = +inf; info = 0
 *   BINF_FE_EMPTY       n == 0: NaN outputs, nothing is read
 *   BINF_FE_NO_OVERLAP  the problem closed with S == 0: every sigma under- or overflowed
 *                       (the two sides lie some 745 apart from the iterate), g is flat 0
 *                       around it and the root is not determined; delta is the iterate
 *                       that met the plateau, info = 0
 *   BINF_FE_NOT_CONVERGED  the iteration cap, 2200: Newton and bisection steps may
 *                       interleave, so the cap, not the halving, is what guarantees the end
 * R == 1 returns 0 with nothing written.  workspace: binf_free_energy_bar_workspace_bytes
 * (T, C, R, G) bytes, 8-byte aligned, caller-owned.  BINF_E_ARG: a negative size, R < 1,
 * C % R != 0, G < 1 or not a divisor of C / R, first_round < 0, stride_t < C with T > 1, a
 * NULL buffer, a workspace that is NULL, misaligned or too small.  BINF_E_UNSUPPORTED: T or
 * C beyond 2^31 - 1, more chunks than one launch covers.
 * ---------------------------------------------------------------------- */
#define BINF_FE_CHUNK 4096
#define BINF_FE_OK 0
#define BINF_FE_INVALID 1
#define BINF_FE_NO_FINITE 2
#define BINF_FE_EMPTY 3
#define BINF_FE_NOT_CONVERGED 4
#define BINF_FE_ONE_SIDED 5
#define BINF_FE_NO_OVERLAP 6
int32_t binf_replica_work_f64(const double *lp_own, const double *lp_swapped, double *w_out,
                              int64_t C, int64_t R, int32_t parity, void *stream);
int32_t binf_free_energy_chunk(void);
int64_t binf_free_energy_bar_workspace_bytes(int64_t T, int64_t C, int64_t R, int64_t G);
int32_t binf_free_energy_bar_f64(const double *work, int64_t stride_t, int64_t T, int64_t C,
                                 int64_t R, int64_t first_round, int64_t G, double *delta,
                                 double *delta_fwd, double *delta_rev, double *info,
                                 int64_t *n, int64_t *n_invalid, int32_t *status,
                                 void *workspace, int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------
 * Tempered sequential Monte Carlo over populations of chains: the reweighting with its
 * root search for the next temperature, systematic resampling and the row gather
 * (build-defined, as the exchange above).  Added within ABI 7: new symbols only.
 *
 * C = G * P chains: population g is the chains [g * P, (g + 1) * P); 1 <= P <= 65536.
 * One 256-thread workgroup serves a population.  THE SUM of a population's P terms, used
 * by every sum below: thread j adds its terms j, j + 256, ... in ascending order onto 0.0;
 * the 64 lanes of a wave join as a balanced tree over neighbouring lanes; the four waves as
 * ((w0 + w1) + w2) + w3.  Nothing depends on G, on a population's place in the batch or on
 * the launch geometry.
 *
 * binf_smc_temper_f64: ll [C] holds l = log p_1 - log p_0 of every particle, beta [G] the
 *   populations' temperatures (updated in place), rho = ess_fraction in (0, 1].
 *     m = the maximum of the finite l of the population; e_i = l_i - m (one subtraction)
 *     w_i(d) = exp(d * e_i) (one product, the device library's exp, within 1 ulp); exactly
 *              +0.0 where l_i is -inf or NaN or e_i overflows to -inf
 *     S1(d) = SUM w_i, S2(d) = SUM (w_i * w_i); ESS(d) = (S1 * S1) / S2 (two roundings)
 *     enough(d): ESS(d) >= rho * (double)P (one product)
 *   hi0 = 1 - beta.  enough(hi0): delta = hi0 and beta becomes exactly 1.0.  Otherwise
 *   lo = 0, hi = hi0 and n_bisect times mid = 0.5 * (lo + hi), enough(mid) ? lo = mid :
 *   hi = mid; then delta = lo, or, with lo still 0, delta = hi and status STALLED (progress
 *   is guaranteed); beta becomes beta + delta (one addition).  Outputs:
 *     delta [G], beta [G]; beta_chain [C] = the population's new beta at each of its chains
 *     w [C] = w_i(delta); ess [G] = ESS(delta)
 *     log_z_inc [G] = delta * m + (log(S1(delta)) - log((double)P))   in this order
 *     n_invalid [G] (int64) = the NaN among the population's l; status [G] (int32)
 *   BINF_SMC_OK        a step was taken
 *   BINF_SMC_STALLED   a step was taken, the smallest the bisection could resolve
 *   Pass-through (delta = 0, beta kept, every w = 1, log_z_inc = 0, ess = P), tested in
 *   this order:
 *   BINF_SMC_FINISHED  beta is not below 1
 *   BINF_SMC_INVALID   a +inf among the l
 *   BINF_SMC_NO_FINITE no finite l
 *   w doubles as the kernel's scratch for P > 8192 and must not overlap ll; beta_chain must
 *   not overlap ll or w (BINF_E_ALIAS).  BINF_E_ARG: a negative size, G * P != C, a rho
 *   outside (0, 1], n_bisect outside 1 ... 128, a NULL buffer.  BINF_E_UNSUPPORTED: P outside
 *   1 ... 65536, G beyond 2^31 - 1.  C == 0 returns 0 without a launch.
 *
 * binf_smc_resample_f64: systematic resampling of every population from w [C] (>= 0).
 *   u_g: u[g] where u [G] is supplied, else element chain_offset + g * P of the uniform
 *   stream (seed, offset) of binf_rng_uniform_f64 -- the global index of the population's
 *   first particle; chain_offset >= 0 = global index of chain 0 of this call.
 *   The prefix sums: thread j of 256 owns the particles [j * L, (j + 1) * L), L = ceil(P /
 *   256); r_i = its running sum, the first weight, then + w_i in ascending order; T_j = the
 *   segment's last r; E_0 = 0, E_j = E_(j-1) + T_(j-1) in ascending order; cs_i = E_j + r_i
 *   (one addition); total = cs_(P-1).
 *     t_k = (((double)k + u_g) / (double)P) * total        k = 0 .. P - 1, three roundings
 *     ancestor[g * P + k] = g * P + (the first i with cs_i > t_k, strictly; if there is
 *                           none, the last i with w_i > 0)
 *   cs never moves at a weight of 0, so such a particle is no ancestor for any u_g in
 *   [0, 1).  n_unique [G] (int64) = the distinct ancestors of the population.  A population
 *   gets the identity (ancestor[c] = c, n_unique = P) where status (NULL, or [G] from
 *   binf_smc_temper_f64) is FINISHED, INVALID or NO_FINITE, where total is not a finite
 *   positive number, or where u_g lies outside [0, 1).
 *   BINF_E_ARG: a negative size, G * P != C, chain_offset < 0, a NULL w, ancestor or
 *   n_unique.  BINF_E_UNSUPPORTED as above.  C == 0 returns 0 without a launch.
 *
 * binf_smc_gather_f64: out[c,:] = x[ancestor[c],:] for x, out [C x D] (any 8-byte
 *   alignment; rows that are 16-byte aligned in both move with 16-byte accesses, any D >=
 *   0), and side_out[k * C + c] = side_in[k * C + ancestor[c]] for the n_side <= 4 rows of
 *   two [n_side x C] arrays (NULL with n_side == 0).  ancestor [C] int64, any values in
 *   [0, C); an entry outside makes row c (and its side entries) quiet NaN.  x is never
 *   written: out must not overlap x, nor side_out side_in, nor an output the ancestors
 *   (BINF_E_ALIAS).  BINF_E_ARG: a negative size, n_side outside 0 ... 4, a NULL required
 *   buffer.  C == 0 returns 0 without a launch.
 *
 * All three: refusals come before anything is touched.
 * ---------------------------------------------------------------------- */
#define BINF_SMC_OK 0
#define BINF_SMC_FINISHED 1
#define BINF_SMC_NO_FINITE 2
#define BINF_SMC_INVALID 3
#define BINF_SMC_STALLED 4
#define BINF_SMC_MAX_P 65536
int32_t binf_smc_temper_f64(const double *ll, double *beta, int64_t C, int64_t P, int64_t G,
                            double ess_fraction, int32_t n_bisect, double *delta,
                            double *beta_chain, double *w, double *log_z_inc, double *ess,
                            int64_t *n_invalid, int32_t *status, void *stream);
int32_t binf_smc_resample_f64(const double *w, const double *u, const int32_t *status,
                              int64_t C, int64_t P, int64_t G, uint64_t seed, uint64_t offset,
                              int64_t chain_offset, int64_t *ancestor, int64_t *n_unique,
                              void *stream);
int32_t binf_smc_gather_f64(const double *x, const int64_t *ancestor, double *out,
                            const double *side_in, double *side_out, int32_t n_side,
                            int64_t C, int64_t D, void *stream);

/* ------------------------------------------------------------------------
 * Convergence diagnostics over the kept draws of many chains: split-R^, effective sample
 * size and Monte-Carlo standard error per dimension (build-defined: the reference runs one
 * chain, thins it by hand and judges the run by histograms, example_script.py:41-47).
 * Added within ABI 7: new symbols only.
 *
 * draws: device fp64 x[t][c][i], t < T, c < C, i < D, at element strides (stride_t,
 * stride_c, stride_i = 1): a sample store's buffer, a column slice of a wider slot and every
 * R-th chain of a ladder are read where they lie.  split in {1, 2}; n = T / split; segment
 * 0 is draws [0, n), segment 1 is [T - n, T) (the middle draw of an odd T is dropped); split
 * chain m = s * C + c, M = split * C.  Every multiply and add below is rounded separately;
 * every sum over draws is sequential from 0.0; every sum over split chains ("blocked") is
 * sequential from 0.0 inside blocks of 64 consecutive m, then sequential from 0.0 over the
 * block sums -- an order that depends on M only.  IEEE results are left as they fall: a
 * dimension that is constant in every chain gives NaN rhat, a NaN draw poisons its own
 * dimension only.
 *
 * binf_chain_moments_f64: per split chain and dimension, one pass over the draws,
 *     K0 = x[first draw of the segment], d_t = x_t - K0, s1 = sum d_t, s2 = sum d_t * d_t
 *     mean[m, i] = K0 + s1 / n        m2[m, i] = s2 - (s1 * s1) / n        (device [M x D])
 *
 * binf_chain_autocov_f64: lags 0 .. max_lag (<= n - 1), mean = the output of the above,
 *     c_i = x_i - mean,  a_m(k) = (sum_{i < n - k} c_i * c_{i+k}) / n
 *     workspace[b, k, i] = sum of a_m(k) over the split chains of block b (m in order)
 *   workspace: device, binf_chain_autocov_workspace_bytes(M, D, max_lag) =
 *   ceil(M / 64) * (max_lag + 1) * D * 8 bytes; it IS the result (the `autocov` of the
 *   summary).  The tiling (16 lags per thread) is not part of the contract: each lag's sum
 *   is sequential in i.
 *
 * binf_diag_summary_f64: from mean, m2 [M x D] and autocov (NULL: R^ only; ess, mcse,
 *   truncated are then not written and may be NULL), n >= 2, M >= 2:
 *     W        = blocked(m2 / (n - 1)) / M
 *     post_mean = g = blocked(mean) / M
 *     Bn       = blocked((mean - g)^2) / (M - 1)
 *     varplus  = ((n - 1) / n) * W + Bn          sd = sqrt(varplus) (sd may be NULL)
 *     rhat     = sqrt(varplus / W)
 *     A(k)     = (sum over blocks b, in order, of autocov[b, k, i]) / M
 *     rho(k)   = 1 - (W - (A(k) * n) / (n - 1)) / varplus
 *     P_j      = rho(2j) + rho(2j+1) while 2j + 1 <= max_lag; stop at the first P_j < 0;
 *                for j >= 1, P_j = P_{j-1} if P_{j-1} < P_j            (Geyer's initial
 *                monotone sequence on the multi-chain rho)
 *     tau      = -1 + 2 * sum P_j      ess = (M * n) / tau      mcse = sqrt(varplus / ess)
 *     truncated[i] = 1 if no negative pair was reached within max_lag (ess is then an
 *                upper bound), else 0                                        (uint8 [D])
 *   every output device [D]; workspace: binf_diag_summary_workspace_bytes(M, D) =
 *   3 * ceil(M / 64) * D * 8 bytes (the block sums).
 *
 * BINF_E_ARG: C < 1, D < 1, split outside {1, 2}, n < 2, stride_i != 1, a negative stride,
 * strides under which two draws share an element, max_lag outside [0, n - 1], M < 2 for the
 * summary, a NULL required buffer, a workspace that is NULL or too small.  BINF_E_ALIAS: an
 * output or workspace that overlaps the draws, an input or another output.
 * BINF_E_UNSUPPORTED: draws spanning more than 2^60 elements, more tiles than one launch
 * holds (indexing is 64-bit throughout).  Refusals come before anything is touched.
 * ---------------------------------------------------------------------- */
int32_t binf_chain_moments_f64(const double *draws, int64_t stride_t, int64_t stride_c,
                               int64_t stride_i, int64_t T, int64_t C, int64_t D,
                               int32_t split, double *mean, double *m2, void *stream);
int64_t binf_chain_autocov_workspace_bytes(int64_t M, int64_t D, int64_t max_lag);
int32_t binf_chain_autocov_f64(const double *draws, int64_t stride_t, int64_t stride_c,
                               int64_t stride_i, int64_t T, int64_t C, int64_t D,
                               int32_t split, const double *mean, int64_t max_lag,
                               void *workspace, int64_t workspace_bytes, void *stream);
int64_t binf_diag_summary_workspace_bytes(int64_t M, int64_t D);
int32_t binf_diag_summary_f64(const double *mean, const double *m2, const double *autocov,
                              int64_t n, int64_t M, int64_t D, int64_t max_lag,
                              double *post_mean, double *varplus, double *sd, double *W,
                              double *rhat, double *ess, double *mcse, uint8_t *truncated,
                              void *workspace, int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------
 * The rank layer of the diagnostics: a sort of the whole record per dimension, and from it
 * sorted values, rank-normalised draws (Vehtari et al. 2021) and quantiles; two element-wise
 * maps and one combination complete rank-normalised / folded split-R^ and bulk / tail ESS
 * (composed in binf_amd/diagnostics.py: rank_summary).  Build-defined.  Added within ABI 7:
 * new symbols only.
 *
 * Pooled set.  draws, its strides and split in {1, 2} are those of binf_chain_moments_f64,
 * n = T / split.  The compressed time index t' runs over [0, split * n): t = t' for t' < n,
 * t = t' + T - 2 n beyond (segment 1 starts at T - n; the middle draw of an odd T is
 * dropped).  Per dimension the pooled set has S = split * n * C values; element
 * e = t' * C + c.
 *
 * binf_rank_normalise_f64:
 *   sorted[i][j], device [D x S], optional: the S values of dimension i ascending; -0.0
 *     before +0.0; NaNs of either sign last (their sign and payload are not kept).
 *   rank: k(e) = lo + hi, twice the average rank, lo and hi the first and last 1-based
 *     positions of the tie group of x_e; ties are by numeric equality (-0.0 == +0.0), so k
 *     does not depend on how equal values were ordered; k in [2, 2 S].
 *   z[t'][c][i] = ztab[k(e)], device contiguous [split * n x C x D], optional; needs ztab,
 *     a device table of 2 S + 1 doubles the caller supplies (the library evaluates no
 *     inverse normal; binf_amd.diagnostics.rank_z_table builds the normal scores).  A
 *     dimension that holds a NaN gets NaN in all of its z; other dimensions are untouched.
 *   workspace: device, 8-byte aligned, binf_rank_sort_workspace_bytes(S, D) bytes (keys,
 *     element indices and padding to the power of two >= S; 0 for S < 2, S > 2^30, D < 1).
 *   The sorting algorithm is not part of the contract: every output is a function of the
 *   values alone.
 *
 * binf_sorted_quantiles_f64: probs is a HOST array of Q <= 16 doubles in [0, 1], read
 *   before the call returns; out device [Q x D].  Per dimension, of sorted [D x S]:
 *     h = (S - 1) * p    lo = floor(h)    g = h - lo
 *     a = sorted[lo]     b = sorted[min(lo + 1, S - 1)]     d = b - a
 *     out = a + d * g if g < 0.5, else b - d * (1 - g)       (numpy's linear method)
 *   NaN if sorted[i][S - 1] is NaN.
 *
 * binf_draws_map_f64: out[t'][c][i], device contiguous [split * n x C x D]; param device [D]:
 *     op = BINF_DRAWS_MAP_FOLD   |x - param[i]|
 *     op = BINF_DRAWS_MAP_LE     x <= param[i] ? 1.0 : 0.0
 *   IEEE results are left as they fall (a NaN draw folds to NaN and is not <= anything).
 *
 * binf_rank_diag_combine_f64, over device [D] vectors:
 *     rhat = max(rhat_bulk, rhat_folded)     ess_tail = min(ess_lo, ess_hi)
 *   a NaN in either operand gives NaN; truncated = trunc_mean | trunc_bulk | trunc_lo |
 *   trunc_hi (each the `truncated` of one binf_diag_summary_f64; 0 or 1).
 *
 * BINF_E_ARG: what binf_chain_moments_f64 refuses about draws; sorted and z both NULL; z
 * without ztab; a workspace that is NULL, too small or not 8-byte aligned; Q outside
 * [1, 16]; a probability outside [0, 1] (NaN included); S < 1 or D < 1; an op that is
 * neither of the two; a NULL required buffer.  BINF_E_ALIAS: an output or workspace that
 * overlaps an input or another output.  BINF_E_UNSUPPORTED: S > 2^30, more elements than
 * one launch holds (indexing is 64-bit throughout).  Refusals come before anything is
 * touched; everything is stream-ordered and graph-capturable.
 * ---------------------------------------------------------------------- */
#define BINF_DRAWS_MAP_FOLD 0
#define BINF_DRAWS_MAP_LE 1
int64_t binf_rank_sort_workspace_bytes(int64_t S, int64_t D);
int32_t binf_rank_normalise_f64(const double *draws, int64_t stride_t, int64_t stride_c,
                                int64_t stride_i, int64_t T, int64_t C, int64_t D,
                                int32_t split, const double *ztab, double *sorted, double *z,
                                void *workspace, int64_t workspace_bytes, void *stream);
int32_t binf_sorted_quantiles_f64(const double *sorted, int64_t S, int64_t D,
                                  const double *probs, int32_t Q, double *out, void *stream);
int32_t binf_draws_map_f64(const double *draws, int64_t stride_t, int64_t stride_c,
                           int64_t stride_i, int64_t T, int64_t C, int64_t D, int32_t split,
                           int32_t op, const double *param, double *out, void *stream);
int32_t binf_rank_diag_combine_f64(const double *rhat_bulk, const double *rhat_folded,
                                   const double *ess_lo, const double *ess_hi,
                                   const uint8_t *trunc_mean, const uint8_t *trunc_bulk,
                                   const uint8_t *trunc_lo, const uint8_t *trunc_hi, int64_t D,
                                   double *rhat, double *ess_tail, uint8_t *truncated,
                                   void *stream);

/* ------------------------------------------------------------------------
 * Posterior-predictive density of a Gaussian error model over a grid of points,
 * from S drawn samples: predict (binf/example/misc.py:3-16) for every point of the
 * [nx x ny] grid that plot_prediction_tube walks with two Python loops
 * (binf/example/plots.py:8-11) -- one launch.
 *   out[i,j] = exp(log_sum_exp_s f[s,i,j]) / S                          (misc.py:16)
 *   f[s,i,j] = -0.5 * (mock[s,i] - ys[i,j])**2 * precision[s]
 *              + 0.5 * log(precision[s]) - half_log_2pi                  (misc.py:8)
 *   log_sum_exp(x) = log(sum(exp(x - max(x)))) + max(x)   (csb.numeric.log_sum_exp:
 *   csb is absent, its published definition; "parity unpinned")
 * mock [S x nx]: the forward model at predict_space[i] for sample s (for the
 * polynomial model: binf_poly_forward_f64 of the sampled coefficients); precision
 * [S]; ys, out [nx x ny]; half_log_2pi = 0.5 * log(2 pi) as the host computes it.
 * NaN / inf follow numpy (a negative precision gives NaN, S >= 1 required: the
 * reference's max() of no samples raises).  Lane-strided sums and the device
 * library's log / exp: not bit-identical to the numpy restatement; the distance
 * from the exact value of the expression is inside the bound derived in
 * tests/predict_ref.py (density_bound).
 * workspace: binf_predictive_density_workspace_bytes(S, nx, ny) bytes of device
 * memory (0 for grids that fill the chip by themselves: NULL is then accepted) --
 * a small grid with many samples is computed chunk of samples by chunk and joined.
 * A workspace that is not NULL must be 8-byte aligned (BINF_E_ARG otherwise).
 * ---------------------------------------------------------------------- */
int64_t binf_predictive_density_workspace_bytes(int64_t S, int64_t nx, int64_t ny);
int32_t binf_predictive_density_f64(const double *mock, const double *precision,
                                    const double *ys, double *out, int64_t S,
                                    int64_t nx, int64_t ny, double half_log_2pi,
                                    void *workspace, int64_t workspace_bytes,
                                    void *stream);

/* ------------------------------------------------------------------------
 * Model comparison by predictive fit: the pointwise log-likelihood record of a Gaussian
 * error model, Pareto-smoothed importance-sampling leave-one-out (PSIS-LOO: Vehtari, Gelman
 * & Gabry 2017; Vehtari, Simpson, Gelman, Yao & Gabry 2024; the algorithm of the `loo` R
 * package and of ArviZ) with the Pareto-khat diagnostic per observation, and WAIC from the
 * same walk (csrc/loo.hip; composed in binf_amd/loo.py; restated in tests/loo_ref.py).
 * Build-defined.  Added within ABI 7: new symbols only.
 *
 * binf_gauss_pointwise_loglik_f64: mock, out device [S x N]; precision [S]; ys [N];
 *     hlp[s]    = 0.5 * log(precision[s])                       once per row
 *     d         = mock[s,i] - ys[i]
 *     out[s,i]  = (-0.5 * (d * d)) * precision[s] + hlp[s] - half_log_2pi
 *   the term of binf_predictive_density_f64, in its order of operations, each operation
 *   rounded on its own.  IEEE results are left as they fall: a precision below 0 gives NaN,
 *   a precision of 0 gives -inf (NaN where d is infinite).  S == 0 or N == 0: nothing is done.
 *   Within tests/loo_ref.py: pointwise_bound of the exact value; bit for bit numpy's where
 *   precision[s] is 1.0.
 *
 * binf_psis_loo_f64: sorted_ll device [N x S], per observation its S pointwise
 *   log-likelihoods ascending, NaNs last: what binf_rank_normalise_f64(..., split = 1,
 *   sorted = ...) writes for the record ll [S x N] passed as draws [T = S x C = 1 x D = N]
 *   (or any [T x C x N] view: strides are that call's business).  Nothing here sorts.
 *   Outputs, device [N]: elpd_loo, khat, n_eff, lppd, p_waic (double), tail_len (int32).
 *   Per observation, a[0] <= ... <= a[S-1]; exp is the library's on the whole real line:
 *     log ratios  lw_j = a[0] - a[j]  (the largest, 0, at j = 0)
 *     M = min(floor(S / 5), ceil(3 sqrt(S)))  in integers;  tail_len = M;  the tail is
 *     j = 0 .. M-1;  cutoff  lc = a[0] - a[M],  ec = exp(lc)
 *     exceedances, ascending:  x_t = exp(a[0] - a[M-t]) - ec,  t = 1 .. M
 *   No smoothing if M < 5, or x_M is not > 0, or x_M is not finite: lw'_j = lw_j for every
 *   j and khat = +inf.  Otherwise the fit of Zhang & Stephens (2009), m = 30 + floor(sqrt(M)):
 *     b_j = (1 - sqrt(m / (j - 0.5))) / (3 * x_q) + 1 / x_M,  q = floor(M / 4 + 0.5),  j = 1 .. m
 *     k_j = (sum_t log1p(-b_j * x_t)) / M
 *     L_j = M * (log(-b_j / k_j) - k_j - 1)
 *     w_j = 1 / sum_l exp(L_l - L_j)                            l = 1 .. m ascending from 0.0
 *     the w_j < 10 * 2^-52 are dropped;  W = sum of the kept w_j;  bhat = sum b_j * (w_j / W)
 *                                                               both ascending from 0.0
 *     k' = (sum_t log1p(-bhat * x_t)) / M;   sigma = -k' / bhat;   khat = (M k' + 5) / (M + 10)
 *     p_t = (t - 0.5) / M;   q_t = sigma * expm1(-khat * log1p(-p_t)) / khat
 *     lw'_(M-t) = min(log(q_t + ec), 0)      in order to the sorted tail, t <-> j = M - t;
 *     lw'_j = lw_j for j >= M.  Only order statistics enter: no element index is carried.
 *   IEEE results are left as they fall (a khat of exactly 0 divides 0 by 0: NaN).  Then
 *     sh1 = max_j lw'_j  (over the tail and lc)     sh2 = max(a[0], max_(j<M) (lw'_j + a[j]))
 *     s1  = sum_j exp(lw'_j - sh1)      s1q = sum_j exp(lw'_j - sh1)^2
 *     s2  = sum_(j<M) exp((lw'_j + a[j]) - sh2) + (S - M) * exp(a[0] - sh2)
 *           (a body draw's ratio times its likelihood is exp(a[0]) exactly)
 *     elpd_loo = (sh2 - sh1) + (log(s2) - log(s1))              n_eff = (s1 * s1) / s1q
 *     s3  = sum_j exp(a[j] - a[S-1])    lppd = a[S-1] + (log(s3) - log(S))
 *     abar = (sum_j a[j]) / S           p_waic = (sum_j (a[j] - abar)^2) / (S - 1)   two passes
 *   elpd_waic = lppd - p_waic and p_loo = lppd - elpd_loo are the caller's subtractions.
 *   Orders.  A sum over the tail's t inside the fit: 64 accumulators from 0.0, element t - 1
 *   to accumulator (t - 1) mod 64, ascending; the 64 joined by the balanced tree over
 *   neighbours, c[2i] + c[2i+1], level by level.  sum_j a[j]: the same with 256
 *   accumulators over j.  The tail's share of s1, s1q, s2 (j < M): 256 accumulators over j.
 *   s1, s1q (j >= M; a term of +0.0 for j < M), s3 and the squared deviations: per chunk
 *   [8192 c, min(S, 8192 (c + 1))) 256 accumulators over j - 8192 c and the tree; then
 *   ((start + chunk 0) + chunk 1) + ... ascending, start = the tail's share for s1 and s1q
 *   and 0.0 for the others.  The cut depends on S alone.
 *   So every output is a function of the column's VALUES alone: bit for bit independent of
 *   the order of the draws, of how many observations share the call, of the record's strides.
 *   A column whose largest entry a[S-1] is NaN (the sort puts NaNs last), or that holds +inf
 *   or -inf (then a[0] or a[S-1]), gives NaN in every floating output: a draw of zero
 *   likelihood has no finite importance ratio, and one of infinite likelihood no finite
 *   weight to give the others.  tail_len is M all the same; other columns are untouched.
 *   workspace: device, 8-byte aligned, binf_psis_loo_workspace_bytes(S, N) bytes =
 *   8 N (8 + 4 ceil(S / 8192)); 0 for a shape that is refused.
 *   Lane-strided sums and the device library's exp / log / log1p / expm1: not bit-identical
 *   to the numpy restatement; tests/test_gpu_loo.py holds the distance from the 50-digit
 *   value to 32 times the restatement's own.
 *
 * binf_pointwise_totals_f64: the reductions over observations.  x (and y, optional) device
 *   [R x N] contiguous rows; d[r][i] = x[r][i] - y[r][i], or x[r][i] without y:
 *     out[2 r]     = sum_i d[r][i]                    256 accumulators over i and the tree
 *     out[2 r + 1] = sum_i (d[r][i] - out[2 r] / N)^2               likewise, second pass
 *     out[2 R]     = number of khat[i] > threshold, as a double     only with khat (device [N])
 *   out: device, 2 R doubles, 2 R + 1 with khat.
 *
 * BINF_E_ARG: S < 2 or N < 1 (psis_loo), S < 0 or N < 0 (record), R < 1 or N < 1 (totals); a
 * NULL required buffer; a workspace that is NULL, too small or not 8-byte aligned.
 * BINF_E_UNSUPPORTED: S > 2^22 (the tail, 6144 values there, lives in LDS), N >= 2^31, a
 * record of more than 2^53 elements, R > 65536.  BINF_E_ALIAS: an output or the workspace
 * that overlaps an input, another output or the workspace.  Refusals come before anything
 * is touched; everything is stream-ordered and graph-capturable; no atomics.
 * ---------------------------------------------------------------------- */
int32_t binf_gauss_pointwise_loglik_f64(const double *mock, const double *precision,
                                        const double *ys, double *out, int64_t S, int64_t N,
                                        double half_log_2pi, void *stream);
int64_t binf_psis_loo_workspace_bytes(int64_t S, int64_t N);
int32_t binf_psis_loo_f64(const double *sorted_ll, int64_t S, int64_t N, double *elpd_loo,
                          double *khat, double *n_eff, double *lppd, double *p_waic,
                          int32_t *tail_len, void *workspace, int64_t workspace_bytes,
                          void *stream);
int32_t binf_pointwise_totals_f64(const double *x, const double *y, int64_t R, int64_t N,
                                  const double *khat, double threshold, double *out,
                                  void *stream);

/* ------------------------------------------------------------------------
 * Pairwise-distance-restraint model (BASELINE config C5; build-defined, the
 * reference has no code for it -- it follows the reference's forward-model /
 * error-model plug-in shape, binf/model/forwardmodels.py:10-66).
 * Coordinates x[c, 3*bead + axis]; pairs (i<j) in numpy.triu_indices order.
 * ---------------------------------------------------------------------- */

/* out[c,p] = sqrt(((x_i - x_j)**2).sum()) for p = (pair_i[p], pair_j[p]);
 * bit-identical to the numpy expression.  pair_i / pair_j device int32 [n_pairs]. */
int32_t binf_pairdist_forward_f64(const double *x, const int32_t *pair_i,
                                  const int32_t *pair_j, double *out, int64_t C,
                                  int64_t n_beads, int64_t n_pairs, void *stream);

/* Likelihood._evaluate_log_prob (binf/pdf/likelihoods.py:141-146) for the
 * pair-distance forward model + Gaussian error model, fused: the same bits as
 * binf_pairdist_forward_f64 followed by binf_gauss_err_logp_f64, without the
 * [C x n_pairs] distances going through HBM. */
/* workspace (ABI 6; the three entry points below): with FEWER chains than CUs -- or more than
 * 2048 beads -- a workgroup per chain walking the whole pair list leaves the chip idle (0.3 ms
 * at 1024 beads, 1.2 ms at 2048, 18 ms at 4096, whatever the number of chains).  np.sum adds
 * the sums of 8192-element chunks one after the other, so given
 * binf_pairdist_chi2_workspace_bytes(C, n_beads, n_pairs) bytes of device memory (0 when that
 * does not apply; NULL is always accepted -- only the speed changes) every chunk is a
 * workgroup of its own and a second launch adds the chunk sums in order: the same bits. */
int64_t binf_pairdist_chi2_workspace_bytes(int64_t C, int64_t n_beads, int64_t n_pairs);
int32_t binf_pairdist_gauss_logp_f64(const double *x, const int32_t *pair_i,
                                     const int32_t *pair_j, const double *ys,
                                     double precision, const double *precision_chain,
                                     double *out, int64_t C, int64_t n_beads,
                                     int64_t n_pairs, void *workspace,
                                     int64_t workspace_bytes, void *stream);

/* The same with a two-entry per-chain memo of chi^2 (it depends on the chain's coordinates
 * alone): memo_x [2 x C x 3 n_beads] / memo_chi2 [2 x C] / memo_state [2 x C] as in
 * binf_poly_gauss_logp_memo_f64 -- HMCSampler.sample() asks for the log-prob of the state
 * it ended the last transition with again as E_before (binf/samplers/hmc.py:148); that
 * state is the last proposal or the state before it, and both are in the memo. */
int32_t binf_pairdist_gauss_logp_memo_f64(const double *x, const int32_t *pair_i,
                                          const int32_t *pair_j, const double *ys,
                                          double precision, const double *precision_chain,
                                          double *out, double *memo_x, double *memo_chi2,
                                          uint8_t *memo_state, int64_t C, int64_t n_beads,
                                          int64_t n_pairs, void *workspace,
                                          int64_t workspace_bytes, void *stream);

/* HMCSampler.sample()'s energy (binf/samplers/hmc.py:143,148,150) for the restraint
 * posterior in ONE launch:
 *   energy[c]   = 0.5 * np.sum(p[c]**2) - log_prob[c]
 *   log_prob[c] = the Posterior's components added in their order, ((t0 + t1) + t2) + ...
 *                 (binf/pdf/posteriors.py:147-151).  term_kind[0 .. n_terms) (host array,
 *                 1 <= n_terms <= 4, each kind at most once) names them:
 *                   1  the restraint likelihood, -0.5 chi^2 precision_c + n_pairs/2 log
 *                      precision_c (as binf_pairdist_gauss_logp_f64) -- must be present;
 *                   0  an isotropic Gaussian prior, (-0.5 prior_k) * np.sum((x[c] - prior_x0)**2);
 *                   2, 3  a component whose variables are all fixed -- a constant of the
 *                      move, evaluated by the caller: extra0 / extra1 [C], or null and the
 *                      scalar (e.g. the GammaPrior of the precision inside a Gibbs sweep).
 * Replaces the per-step tier's row sum for the prior, memo check, chi^2 reduction,
 * binf_sum_terms_f64 and binf_hmc_energy_f64 (six launches) and is bit-identical to
 * them: every sum in numpy's order, every scalar operation in theirs.  x, p: device
 * [C x 3 n_beads]; energy [C]; log_prob [C] or null.  memo_x / memo_chi2 / memo_state: the
 * two-entry chi^2 memo of binf_pairdist_gauss_logp_memo_f64 (same buffers, same contents:
 * the two functions may share one memo), or all three null.  n_beads <= 2048. */
int32_t binf_pairdist_hmc_energy_f64(const double *x, const double *p, const int32_t *pair_i,
                                     const int32_t *pair_j, const double *ys, double precision,
                                     const double *precision_chain, double prior_k,
                                     double prior_x0, int32_t n_terms, const int32_t *term_kind,
                                     const double *extra0, double extra0_scalar,
                                     const double *extra1, double extra1_scalar,
                                     double *energy, double *log_prob, double *memo_x,
                                     double *memo_chi2, uint8_t *memo_state, int64_t C,
                                     int64_t n_beads, int64_t n_pairs, void *workspace, int64_t workspace_bytes,
                                     void *stream);

/* Energy gradient of the Gaussian restraint likelihood,
 *   out[c, 3i+a] = precision_c * sum_{j != i} (d_ij - ymat[j][i]) (x_i - x_j)[a] / d_ij,
 * i.e. Likelihood._evaluate_gradient (binf/pdf/likelihoods.py:148-155) without
 * forming the [3n x n(n-1)/2] Jacobian (coordinates in LDS; 32..256 beads: every
 * unordered pair once with its target distance in a register, otherwise
 * one-sided all-pairs loops).  Held to 1e-10 of the numpy expression; the
 * summation order depends on n_beads only, so a chain's result does not depend on
 * C.  ymat: device, SYMMETRIC [n_beads x n_beads] target distances (ymat[i][j] ==
 * ymat[j][i] is relied upon; the diagonal is ignored). */
int32_t binf_pairdist_gauss_grad_f64(const double *x, const double *ymat,
                                     double precision, const double *precision_chain,
                                     double *out, int64_t C, int64_t n_beads,
                                     void *stream);

/* The targets of the 32..256-bead force kernels in the order their waves hold them
 * (every unordered pair once, 32 targets per lane in registers): a function of
 * (ymat, n_beads) alone.  Packed once per model, the `_packed_` entry points below
 * read 32 coalesced values per lane at the start of a launch instead of walking the
 * [n x n] matrix tile by tile through LDS (once per workgroup: ~10 of the 175 us of
 * a 20-step trajectory at 256 chains).  binf_pairdist_packed_targets_bytes: size of
 * the packed form, 0 for bead counts the one-sided kernels serve (then there is
 * nothing to pack and `packed` must be null).  For 32..256 beads the results are the
 * same bits with and without `packed`; `packed` must have been made from the same ymat.
 * 257..1024 beads (ABI 6): the packed form is the step order of the ring kernels, which
 * compute every unordered pair once (2-4x the one-sided loops) and read their targets
 * from it for every force evaluation; WITH `packed` these bead counts take the ring
 * kernels, without it the one-sided loops -- the two agree to ~1e-15 relative (another
 * summation order), each is bit-identical between its force kernel and its fused
 * leapfrog and for any number of chains. */
int64_t binf_pairdist_packed_targets_bytes(int64_t n_beads);
int32_t binf_pairdist_pack_targets_f64(const double *ymat, double *packed, int64_t n_beads,
                                       void *stream);
/* workspace (ABI 6): for FEW chains of 257..1024 beads a workgroup per chain would leave most
 * of the chip idle; given binf_pairdist_tiles_workspace_bytes(C, n_beads) bytes of device
 * memory (0 when that does not apply: NULL is then fine, and it is always accepted -- only the
 * speed changes) every 64 x 64 tile of pairs becomes a wave of its own and a second launch adds
 * a bead's partial sums in the ring kernels' order: the same bits, ~5x at 32 chains of 1024
 * beads. */
int64_t binf_pairdist_tiles_workspace_bytes(int64_t C, int64_t n_beads);
int32_t binf_pairdist_gauss_grad_packed_f64(const double *x, const double *ymat,
                                            const double *packed, double precision,
                                            const double *precision_chain, double *out,
                                            int64_t C, int64_t n_beads, void *workspace,
                                            int64_t workspace_bytes, void *stream);

/* The whole leapfrog integration HMCSampler._leapfrog (binf/samplers/hmc.py:92-125)
 * for the restraint posterior in one launch: q, p device [C * 3n], integrated in
 * place over nsteps steps (half kick, (nsteps-1) x [drift, kick], drift, half
 * kick).  Gradient = precision_c * restraint force (+ optional isotropic
 * Gaussian prior term prior_k * (x - prior_x0), added before or after the
 * likelihood term as prior_first says -- the Posterior's component order).
 * Bit-identical to the per-step generic tier.  n_beads <= 1024. */
int32_t binf_pairdist_leapfrog_f64(double *q, double *p, const double *ymat,
                                   double precision, const double *precision_chain,
                                   int32_t has_prior, double prior_k, double prior_x0,
                                   int32_t prior_first, double timestep,
                                   const double *dt_chain, int32_t nsteps, int64_t C,
                                   int64_t n_beads, int32_t mode, void *stream);
/* the same with the packed targets (null: as binf_pairdist_leapfrog_f64) and, optionally,
 * the start positions read from q_from [C * 3n] instead of q (q then only receives the end
 * positions: the copy of the state HMCSampler.sample() makes before integrating,
 * hmc.py:140-141, is not needed); q_from null or == q: in place. */
int32_t binf_pairdist_leapfrog_packed_f64(double *q, const double *q_from, double *p,
                                          const double *ymat,
                                          const double *packed, double precision,
                                          const double *precision_chain, int32_t has_prior,
                                          double prior_k, double prior_x0, int32_t prior_first,
                                          double timestep, const double *dt_chain,
                                          int32_t nsteps, int64_t C, int64_t n_beads,
                                          int32_t mode, void *workspace,
                                          int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------
 * Device random draws (throughput mode): counter-based Philox4x32-10, key =
 * seed, element i of a call uses counter (i, offset).  Replace the
 * np.random.normal / uniform / gamma draws of binf/samplers/hmc.py:146,151 and
 * binf/example/samplers.py:47 when bit-parity with numpy's stream is not
 * required.  A caller advances `offset` by 1 per uniform / normal call and by
 * 128 per gamma call so that calls never reuse a counter.
 * `i` is a GLOBAL element index: out[l] receives element elem_offset + l
 * (elem_offset >= 0), so a rank filling its window of a larger logical array
 * (chains [s, s + C) of a [C_total x D] draw: elem_offset = s * D, n = C * D) writes
 * exactly what the unsharded call writes there.
 * ---------------------------------------------------------------------- */
int32_t binf_rng_uniform_f64(double *out, int64_t n, uint64_t seed, uint64_t offset,
                             int64_t elem_offset, void *stream);  /* [0, 1), 53 bits */
int32_t binf_rng_normal_f64(double *out, int64_t n, uint64_t seed, uint64_t offset,
                            int64_t elem_offset, void *stream);   /* Box-Muller       */
int32_t binf_rng_normal_zig_f64(double *out, int64_t n, uint64_t seed, uint64_t offset,
                                int64_t elem_offset, void *stream);  /* 1024-layer
                                                   ziggurat; offset < 2^48          */
/* The two draws of one HMC transition (hmc.py:146,151) in one launch: what
 * binf_rng_normal_zig_f64(normals, n_normals, seed, offset_normals, elem_offset_normals) and
 * binf_rng_uniform_f64(uniforms, n_uniforms, seed, offset_uniforms, elem_offset_uniforms)
 * write, bit for bit (the streams are those of the separate calls; their offsets must
 * differ). */
int32_t binf_rng_normal_zig_uniform_f64(double *normals, int64_t n_normals, double *uniforms,
                                        int64_t n_uniforms, uint64_t seed,
                                        uint64_t offset_normals, uint64_t offset_uniforms,
                                        int64_t elem_offset_normals,
                                        int64_t elem_offset_uniforms, void *stream);
int32_t binf_rng_gamma_f64(double *out, int64_t n, double shape, uint64_t seed,
                           uint64_t offset, int64_t elem_offset,
                           void *stream);                         /* Marsaglia-Tsang  */
/* ------------------------------------------------------------------------
 * Diagonal HMC metric with windowed warm-up adaption (build-defined: the reference
 * integrates with the identity mass only, binf/samplers/hmc.py:92-125).  Added within ABI 7:
 * new symbols only.
 *
 * A metric M = diag(1 / s^2) is carried through the whitened momentum r = p / sqrt(m): the
 * draw stays r ~ N(0, I) and the kinetic energy 0.5 * sum(r^2), so binf_hmc_energy_f64,
 * binf_accept_select_f64 and the generators serve unchanged; only kick and drift take the
 * per-element step.  scale: device fp64 [G x D]; chain c reads row c % G (G = 1: one metric
 * for all chains; G = R: one per ladder slot c % R; G = C: one per chain); C % G == 0.
 *
 * binf_leapfrog_kick_scaled_f64 / _drift_scaled_f64 / _kick_drift_scaled_f64: the twins of
 * binf_leapfrog_kick_f64 / _drift_f64 / _kick_drift_f64.  Per element, with d = dt_chain[c]
 * (or timestep when dt_chain == NULL), d = 0.5 * d first for a half kick:
 *     h = d * scale[c % G, i]                                        (one rounding)
 *     kick    BINF_MODE_EXACT  p = p - h * g  (the product rounded first)
 *             BINF_MODE_FMA    p = fma(-h, g, p)
 *     drift   BINF_MODE_EXACT  q = q + p * h        BINF_MODE_FMA  q = fma(p, h, q)
 *     kick_drift = the kick, then the drift with the new p, one pass over memory.
 *   With scale == 1.0 everywhere h == d exactly: the bits of the unscaled entry points.
 *   A NaN scale element reaches the elements of its own column (and rows c % G) only.
 *
 * binf_metric_accumulate_f64: one element-wise pass per warm-up transition over the state
 *   x [C x D]; k0, s1, s2 [C x D] hold one running moment set per chain and dimension:
 *     first != 0:  k0 = x, s1 = s2 = 0, then as below          (k0, s1, s2 need no init)
 *     always:      d = x - k0,  s1 = s1 + d,  s2 = s2 + d * d
 *   After n calls (the first with first != 0), k0 + s1 / n and s2 - (s1 * s1) / n are the mean
 *   and m2 of binf_chain_moments_f64(split = 1) over the stacked [n x C x D] record, bit for
 *   bit -- without the record.
 *
 * binf_metric_pool_f64: the variance of the n * C / G draws of group g in dimension i, pooled
 *   over the chains c = g, g + G, ... (increasing c), written into scale[g, i] in place.
 *   Cg = C / G, N = n * Cg:
 *     mean_c = k0 + s1 / n          m2_c = s2 - (s1 * s1) / n
 *     W    = blocked(m2_c)          mbar = blocked(mean_c) / Cg
 *     B    = blocked((mean_c - mbar)^2)
 *     var  = (W + n * B) / (N - 1)
 *     regularise != 0:  var = (N / (N + 5)) * var + 1e-3 * (5 / (N + 5))   (Stan's shrinkage)
 *     scale[g, i] = sqrt(var) if var is finite and > 0, else it keeps its value
 *   Every operation is rounded separately, sqrt is correctly rounded; "blocked" is the
 *   diagnostics' order over the Cg chains of the group: sequential from 0.0 inside blocks of
 *   64 consecutive chains of the group, then sequential from 0.0 over the block sums.  No
 *   workspace and no host read-back.  (n = 1 with Cg = 1 is 0 / 0: the scale stays.)
 *
 * All five: C == 0 or D == 0 returns 0 without a launch.  BINF_E_ARG: a negative size, an
 * unknown mode, G < 1, C % G != 0, n < 1, a NULL buffer.  BINF_E_ALIAS: the scale or dt_chain
 * overlapping a buffer that is written, q overlapping p, a gradient that overlaps p other
 * than exactly, any overlap among x, k0, s1, s2, the scale overlapping the moments.
 * BINF_E_UNSUPPORTED: n * C / G beyond 2^53.  Refusals come before anything is touched.
 * ---------------------------------------------------------------------- */
int32_t binf_leapfrog_kick_scaled_f64(double *p, const double *grad, const double *scale,
                                      int64_t G, double timestep, const double *dt_chain,
                                      int32_t half, int64_t C, int64_t D, int32_t mode,
                                      void *stream);
int32_t binf_leapfrog_drift_scaled_f64(double *q, const double *p, const double *scale,
                                       int64_t G, double timestep, const double *dt_chain,
                                       int64_t C, int64_t D, int32_t mode, void *stream);
int32_t binf_leapfrog_kick_drift_scaled_f64(double *q, double *p, const double *grad,
                                            const double *scale, int64_t G, double timestep,
                                            const double *dt_chain, int64_t C, int64_t D,
                                            int32_t mode, void *stream);
int32_t binf_metric_accumulate_f64(const double *x, double *k0, double *s1, double *s2,
                                   int32_t first, int64_t C, int64_t D, void *stream);
int32_t binf_metric_pool_f64(const double *k0, const double *s1, const double *s2, int64_t n,
                             int64_t C, int64_t D, int64_t G, int32_t regularise,
                             double *scale, void *stream);

/* ------------------------------------------------------------------------
 * Dense HMC metric with windowed covariance warm-up (build-defined, as the diagonal metric
 * above).  Added within ABI 7: new symbols only.
 *
 * M^-1 = L * L^T with L lower triangular.  chol: device fp64 [G x D x D], row-major; chain c
 * uses L = chol[c % G]; C % G == 0.  The momentum stays the whitened r ~ N(0, I) and the
 * kinetic energy 0.5 * sum(r^2): only kick and drift change.  Elements above the diagonal of
 * L are NEVER read (they may hold anything, NaN included).
 *
 * binf_leapfrog_kick_dense_f64 / _drift_dense_f64 / _kick_drift_dense_f64.  Per chain, with
 * d = dt_chain[c] (or timestep when dt_chain == NULL), d = 0.5 * d first for a half kick:
 *     kick    t_i = sum_{j = i .. D-1} L[j][i] * g_j        p_i = p_i - d * t_i
 *     drift   v_i = sum_{j = 0 .. i}   L[i][j] * p_j        q_i = q_i + v_i * d
 *     kick_drift = the kick of the whole row, then the drift with the new p.
 *   Every dot product is ONE sequential chain in ascending j:
 *     first term    t = L * g                      (the rounded product alone, in both modes)
 *     later terms   BINF_MODE_EXACT  t = t + L * g (the product rounded first: two roundings)
 *                   BINF_MODE_FMA    t = fma(L, g, t)
 *     update        BINF_MODE_EXACT  p - d * t,  q + v * d  (the product rounded first)
 *                   BINF_MODE_FMA    fma(-d, t, p),  fma(v, d, q)
 *   With L = I and finite inputs without negative zeros every later term adds an exact +0.0:
 *   the bits of binf_leapfrog_kick_f64 / _drift_f64 / _kick_drift_f64.  With L = diag(s) the
 *   result is NOT bitwise that of the *_scaled_f64 entry points: those round h = d * s first
 *   and then h * g; here s * g is rounded first and then d * t.
 *   A NaN in row r of L reaches t_i for the columns i it sits in and v_r only; a NaN gradient
 *   or momentum element stays in its own chain.
 *   The separately rounded products rule the matrix (MFMA) pipe out: VALU arithmetic.
 *
 * binf_metric_comoments_f64: one pass per warm-up transition over the state x [C x D] keeps
 *   the pooled co-moments of each group -- no per-chain D x D state and no record of draws.
 *   k0, s1: [G x D]; s2: [G x D x D], lower triangle with the diagonal (entries above are
 *   neither read nor written).  The chains of group g are c = g + m * G, m ascending:
 *     first != 0:  k0[g] = x[chain g], s1 = s2 = 0, then as below   (k0, s1, s2 need no init)
 *     always:      d_c = x_c - k0[g]
 *                  s1[g, i]    = s1[g, i]    + blocked_m(d_ci)
 *                  s2[g, i, j] = s2[g, i, j] + blocked_m(d_ci * d_cj)   j <= i, product rounded first
 *   "blocked" is the diagnostics' order: sequential from 0.0 inside blocks of 64 consecutive
 *   chains of the group, then sequential from 0.0 over the block sums.  No mode argument.
 *
 * binf_metric_factor_f64: pool and Cholesky, without a host read-back.  N = n * C / G draws
 *   per group (n: calls accumulated), N >= 2:
 *     cov_ij = (s2_ij - (s1_i * s1_j) / N) / (N - 1)                          j <= i
 *     regularise != 0:  cov_ij = (N / (N + 5)) * cov_ij,  then on the diagonal
 *                       cov_ii = cov_ii + 1e-3 * (5 / (N + 5))                (Stan's shrinkage)
 *   then the lower factor, column j = 0 .. D-1:
 *     a = cov_ij;  a = a - L_ik * L_jk for k = 0 .. j-1 (sequential, the product rounded first)
 *     L_jj = sqrt(a);  L_ij = a / L_jj for i > j          (sqrt and / correctly rounded)
 *   The factor is built in work [G x D x D]: after the call work[g] holds it on and below
 *   the diagonal and +0.0 above, whether it is accepted or not.  chol[g] is overwritten
 *   with work[g] only if every pivot a of L_jj was finite and > 0 and every entry of the
 *   factor is finite; otherwise the group keeps its previous factor (the analogue of "the
 *   scale stays").  status: int32 [G] or NULL; 0 = chol[g] updated, 1 = kept.  A failing
 *   factorisation is a flag, never a retry: the work done does not depend on the data.
 *
 * Sizes: the leapfrog entry points keep a chain's row in the LDS of one workgroup and one
 * workgroup factorises a group, so all five refuse D > 1024 (BINF_E_UNSUPPORTED); they are
 * meant for D <= 256.  C == 0 or D == 0 returns 0 without a launch.  BINF_E_ARG: a negative
 * size, an unknown mode, G < 1, C % G != 0, n < 1, N < 2, a NULL buffer (status excepted).
 * BINF_E_ALIAS: chol or dt_chain overlapping a buffer that is written, q overlapping p, a
 * gradient that overlaps p other than exactly (or q at all); any overlap among x, k0, s1,
 * s2; chol or work overlapping the moments or each other.  BINF_E_UNSUPPORTED also: N beyond
 * 2^53.  Caller-owned buffers, nothing allocated, stream-ordered, safe to capture.
 * ---------------------------------------------------------------------- */
int32_t binf_leapfrog_kick_dense_f64(double *p, const double *grad, const double *chol,
                                     int64_t G, double timestep, const double *dt_chain,
                                     int32_t half, int64_t C, int64_t D, int32_t mode,
                                     void *stream);
int32_t binf_leapfrog_drift_dense_f64(double *q, const double *p, const double *chol,
                                      int64_t G, double timestep, const double *dt_chain,
                                      int64_t C, int64_t D, int32_t mode, void *stream);
int32_t binf_leapfrog_kick_drift_dense_f64(double *q, double *p, const double *grad,
                                           const double *chol, int64_t G, double timestep,
                                           const double *dt_chain, int64_t C, int64_t D,
                                           int32_t mode, void *stream);
int32_t binf_metric_comoments_f64(const double *x, double *k0, double *s1, double *s2,
                                  int32_t first, int64_t C, int64_t D, int64_t G, void *stream);
int32_t binf_metric_factor_f64(const double *s1, const double *s2, int64_t n, int64_t C,
                               int64_t D, int64_t G, int32_t regularise, double *chol,
                               double *work, int32_t *status, void *stream);

/* ------------------------------------------------------------------------
 * No-U-turn sampler (csrc/nuts.hip): iterative multinomial NUTS, one tree per chain,
 * built leaf by leaf on the device.  The host integrates ONE leapfrog step of the working
 * state (q, r, g) per leaf with the existing kick / drift entry points and the signed
 * per-chain step dt_dir (0 for a chain whose tree is finished), evaluates logp(q), and calls
 * binf_nuts_leaf_f64.  Momenta are the whitened r ~ N(0, I) of every metric here, so the
 * generalised U-turn criterion is r . rho for the identity, the diagonal and the dense metric.
 *
 * All arithmetic unfused; dot(a, b) = np.sum(a * b) and K = 0.5 * np.sum(r * r) in numpy's
 * pairwise row order, H = K - logp (the bits of binf_hmc_energy_f64); expc(x) =
 * exp(clip(x, -308, 709)), the accept test's exponential.
 *
 * Uniforms of a transition: u[c, 0:S], S = 2 * max_depth + 2^max_depth - 1;
 *   udir = u[0:md], umerge = u[md:2md], uleaf = u[2md:] indexed by the leaf's number.
 * status: BINF_NUTS_RUN while the tree grows; TURN (the whole tree turned), SUBTURN (the
 * sub-tree being built turned: it is discarded), MAXD (max_depth doublings), DIV (H - H0 above
 * max_delta, or NaN).
 *
 * begin (the working state holds q0, r0, grad(q0); logp = logp(q0)):
 *   H0 = href = H; w_tree = 1; rho_tree = r0; both edges = (q0, r0, g0); prop = q0;
 *   j = n_leap = n_sub = 0; acc = w_sub = accept_stat = 0; status = RUN; moved = diverging = 0;
 *   tree_depth = 0; v = +1 if udir[0] < 0.5 else -1; dt_dir = v * eps.
 * leaf (chains with status != RUN: nothing written):
 *   H = K - logp; n = n_sub; n_leap += 1; delta = H - H0
 *   if not (delta <= max_delta): status = DIV; finish
 *   acc += min(1, expc(-delta))
 *   if H < href: s = expc(H - href); w_sub *= s; w_tree *= s; href = H; wl = 1
 *   else:        wl = expc(href - H)
 *   w_sub += wl;  if uleaf[n_leap - 1] * w_sub < wl: cand = q
 *   rho_sub = r if n == 0 else rho_sub + r
 *   hi = popcount(n >> 1); lo = hi - trailing_ones(n) + 1
 *   n even: ck_r[hi] = r; ck_rho[hi] = rho_sub
 *   n odd:  for i = hi ... lo: sub = (rho_sub - ck_rho[i]) + ck_r[i];
 *                              turn |= dot(ck_r[i], sub) <= 0 or dot(r, sub) <= 0
 *   n_sub += 1
 *   if turn: status = SUBTURN; finish
 *   elif n_sub == 2^j:
 *     if umerge[j] * w_tree < w_sub: prop = cand; moved = 1
 *     w_tree += w_sub; rho_tree += rho_sub; edge[v] = (q, r, g); j += 1
 *     if dot(r_left, rho_tree) <= 0 or dot(r_right, rho_tree) <= 0: status = TURN; finish
 *     elif j == max_depth: status = MAXD; finish
 *     else: v from udir[j]; working = edge[v]; w_sub = 0; n_sub = 0
 *   finish: q_out = prop; tree_depth = j; accept_stat = acc / n_leap; dt_dir = 0;
 *           diverging = (status == DIV); n_divergent += diverging; n_accepted += moved
 *   otherwise dt_dir = v * eps
 * edge_* are [2 x C x D]: slot 0 the left (backward) edge, slot 1 the right one.
 *
 * Every array is caller-owned and distinct; nothing is allocated.  One chain per group of
 * 8 ... 256 lanes.  BINF_E_ARG: struct_size mismatch, a NULL array, C < 0, D < 1, max_depth
 * outside 1 ... 12.  BINF_E_UNSUPPORTED: D > 8192 (one numpy buffer chunk).  BINF_E_ALIAS:
 * any two arrays overlapping.  Refusals come before anything is touched; C == 0 returns 0.
 * ---------------------------------------------------------------------- */
#define BINF_NUTS_RUN     0
#define BINF_NUTS_TURN    1
#define BINF_NUTS_SUBTURN 2
#define BINF_NUTS_MAXD    3
#define BINF_NUTS_DIV     4
#define BINF_NUTS_MAX_DEPTH 12
typedef struct binf_nuts_args {
    uint64_t struct_size;
    /* rows [C x D]: the working state (integrated by the host between leaves) */
    double *q;
    double *r;
    double *g;
    double *edge_q;               /* [2 x C x D] */
    double *edge_r;               /* [2 x C x D] */
    double *edge_g;               /* [2 x C x D] */
    double *cand;                 /* [C x D] the sub-tree's candidate                */
    double *prop;                 /* [C x D] the tree's proposal                     */
    double *q_out;                /* [C x D] written when a chain finishes           */
    double *rho_sub;              /* [C x D] */
    double *rho_tree;             /* [C x D] */
    double *ck_r;                 /* [C x max_depth x D] checkpoints                 */
    double *ck_rho;               /* [C x max_depth x D] */
    /* per chain [C] */
    const double *logp;           /* log p of the working q                          */
    const double *eps;            /* step sizes                                      */
    double *dt_dir;               /* signed step of the next leaf, 0 when finished   */
    double *H0;
    double *href;
    double *w_sub;
    double *w_tree;
    double *acc;
    double *accept_stat;
    const double *u;              /* [C x S] */
    int32_t *j;
    int32_t *n_sub;
    int32_t *n_leap;
    int32_t *v;
    int32_t *status;
    int32_t *tree_depth;
    uint8_t *moved;
    uint8_t *diverging;
    int64_t *n_accepted;          /* += moved at finish                              */
    int64_t *n_divergent;         /* += diverging at finish                          */
    double max_delta;
    int64_t C, D;
    int32_t max_depth;
    int32_t reserved;             /* 0 */
} binf_nuts_args;
int32_t binf_nuts_begin_f64(const binf_nuts_args *args, void *stream);
int32_t binf_nuts_leaf_f64(const binf_nuts_args *args, void *stream);

/* count[0] = number of chains with status == BINF_NUTS_RUN: one workgroup, a fixed order, no
 * atomics.  C == 0 writes 0.  BINF_E_ARG: C < 0, a NULL buffer. */
int32_t binf_nuts_pending(const int32_t *status, int64_t C, int64_t *count, void *stream);

/* Dual averaging of the step sizes (Hoffman & Gelman 2014, algorithm 5), per chain, unfused;
 * the scalars shared by all chains come from the host: w1 = 1 / (t + t0), k1 = sqrt(t) / gamma,
 * eta = t^-kappa.
 *   action 0 (update):   hbar = (1 - w1) * hbar + w1 * (target - accept_stat)
 *                        logeps = mu - k1 * hbar
 *                        logeps_bar = eta * logeps + (1 - eta) * logeps_bar;  eps = exp(logeps)
 *   action 1 (restart):  mu = log(10 * eps); hbar = logeps_bar = 0
 *   action 2 (finalise): eps = exp(logeps_bar)
 * All arrays [C], distinct.  BINF_E_ARG: C < 0, an unknown action, a NULL buffer (accept_stat
 * is read by action 0 only and may be NULL otherwise).  C == 0 returns 0. */
int32_t binf_nuts_adapt_step_f64(double *eps, const double *accept_stat, double *hbar,
                                 double *logeps, double *logeps_bar, double *mu, double target,
                                 double w1, double k1, double eta, int32_t action, int64_t C,
                                 void *stream);

/* ------------------------------------------------------------------------
 * ChEES criterion (Hoffman, Radul & Sountsov 2021): what an adapting ChEESSampler needs from
 * the batch after a trajectory, to learn ONE trajectory length for all chains.  Build-defined
 * (the reference has a fixed nsteps only).  Four entry points, FP64, exact arithmetic whatever
 * the sampler's mode (every product and sum rounded on its own, no contraction), plain stores
 * and launch boundaries only: every output is a pure function of the inputs, whatever the
 * grid or the alignment of the buffers.  Notation: q [C x D] the states before the
 * trajectory, q_prop [C x D] the proposals, v [C x D] the velocities dq/dt at the
 * trajectory's end, alpha [C] the acceptance probabilities.  All arrays contiguous.
 *
 * binf_chees_accept_prob_f64:  alpha[c] = min(1, E(e_before[c] - e_after[c])), E(x) the
 *   accept rule's exponential (binf_clipped_exp_f64: exp of x clipped to [-308, 709]);
 *   exactly +0.0 where e_after[c] is not finite or the difference is NaN.  alpha may be
 *   e_before or e_after itself (element c is read, then written, by one lane).
 *
 * binf_chees_means_f64:  column means over chains of the states and of the EFFECTIVE
 *   proposals (row c of q_prop if alpha[c] > 0, else row c of q: a diverged trajectory's
 *   proposal is never read):
 *     chunk k = chains [k * BINF_CHEES_CHUNK, min(C, (k + 1) * BINF_CHEES_CHUNK)), counted from 0;
 *     partial[k][d] = ((0.0 + x[c0][d]) + x[c0 + 1][d]) + ...      chains ascending
 *     mean[d] = (((0.0 + partial[0][d]) + partial[1][d]) + ...) / C   chunks ascending, one division
 *   A workgroup takes one chunk and a tile of columns, one lane per column (two columns per
 *   lane, 16-byte accesses, where D is even and every base is 16-byte aligned: the same bits);
 *   the partials go to slab [2 x nchunks x D]; a finishing launch adds and divides.
 *
 * binf_chees_terms_f64:  per chain, with x' = the effective proposal's row, m = mean_q,
 *   m' = mean_prop:
 *     a = np.sum((x' - m') * (x' - m')), b = np.sum((q - m) * (q - m)),
 *     s = np.sum((x' - m') * v)          numpy's pairwise order of a contiguous row
 *     g[c] = (a - b) * s;  exactly +0.0 where alpha[c] == 0 (nothing of that chain is read).
 *   One pass: every element of the three rows is loaded once.
 *
 * binf_chees_sums_f64:  with finite(c) = g[c] is finite,
 *     out[0] = sum over finite c of alpha[c] * g[c]      out[1] = sum over finite c of alpha[c]
 *     out[2] = sum over all c of 1 / alpha[c]            (+inf if any alpha is 0)
 *     out[3] = number of chains whose g is not finite, as a double
 *   each sum in this order: chunk k as above, its 64 terms (0.0 for a chain that is not
 *   summed or lies beyond C) joined by the balanced tree over neighbours
 *   t[2i] + t[2i + 1], level by level; then ((0.0 + chunk 0) + chunk 1) + ... ascending in a
 *   finishing launch.  The chunk sums go to slab [nchunks x 4].
 *
 * slab: binf_chees_workspace_bytes(C, D) bytes (serves both), 8-byte aligned, caller-owned;
 * 0 for a shape that is refused.  BINF_E_ARG: C < 1, D < 1, a NULL buffer, a slab that is
 * misaligned.  BINF_E_UNSUPPORTED: D > 8192 (terms: one numpy buffer chunk), C > 2^31 - 1,
 * C * D > 2^53.  BINF_E_ALIAS: an output (or the slab) that overlaps an input, another
 * output or the slab -- except alpha as above.  Refusals come before any launch. */
#define BINF_CHEES_CHUNK 64
int32_t binf_chees_accept_prob_f64(const double *e_before, const double *e_after, double *alpha,
                                   int64_t C, void *stream);
int64_t binf_chees_workspace_bytes(int64_t C, int64_t D);
int32_t binf_chees_means_f64(const double *q, const double *q_prop, const double *alpha,
                             double *slab, double *mean_q, double *mean_prop, int64_t C,
                             int64_t D, void *stream);
int32_t binf_chees_terms_f64(const double *q, const double *q_prop, const double *v,
                             const double *alpha, const double *mean_q, const double *mean_prop,
                             double *g, int64_t C, int64_t D, void *stream);
int32_t binf_chees_sums_f64(const double *alpha, const double *g, double *slab, double *out,
                            int64_t C, void *stream);

/* Host-side evaluation of the generator's block function (known-answer tests). */
int32_t binf_rng_philox4x32_10(const uint32_t counter[4], const uint32_t key[2],
                               uint32_t out[4]);

/* ------------------------------------------------------------------------
 * Host-side helpers exposing the reduction geometry the kernels use, so that
 * CPU tests can check it against numpy's pairwise summation (no GPU needed).
 * ---------------------------------------------------------------------- */

/* Height of numpy's pairwise-sum recursion tree for a length-n vector
 * (0 when n <= 128). */
int32_t binf_pairwise_tree_height(int64_t n);

/* Leaf reached by the root-to-leaf path `path` (bit H-1 = first split, 0 =
 * left) in a tree padded to height H.  Outputs the leaf's offset and length,
 * its depth, and whether `path` is the canonical (lowest) path reaching it.
 * Returns 0, or BINF_E_ARG. */
int32_t binf_pairwise_leaf(int64_t n, int32_t H, int32_t path, int64_t *off,
                           int64_t *len, int32_t *depth, int32_t *canonical);

#ifdef __cplusplus
}
#endif
#endif /* BINF_HIP_H */
