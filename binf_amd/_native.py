"""
ctypes binding of libbinf_hip.so (the C ABI declared in include/binf_hip.h).

The HIP library IS the product path: there is no CPU or PyTorch fallback.  If
the shared object is missing or a call fails, this module raises.
"""
import ctypes
import linecache
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('BINF_LIB_OVERRIDE') or \
    os.path.join(_HERE, 'csrc', 'libbinf_hip.so')   # override: A/B of builds

MODE_EXACT = 0
MODE_FMA = 1
MODE_LANE_PER_CHAIN = 16     # flag for hmc_sample_poly: one lane per chain (N <= 128)
MOVE_HMC = 0
MOVE_RWMC = 1

E_ARG = -1
E_UNSUPPORTED = -2
E_ALIAS = -3


class NativeLibraryError(RuntimeError):
    """libbinf_hip.so is missing, stale or failed."""


_lib = None

_vp = ctypes.c_void_p
_i64 = ctypes.c_int64
_i32 = ctypes.c_int32
_f64 = ctypes.c_double
_u64 = ctypes.c_uint64

# name -> (restype, argtypes); must list every symbol of include/binf_hip.h
SIGNATURES = {
    'binf_abi_version': (_i32, []),
    'binf_last_error': (_i32, [ctypes.c_char_p, ctypes.c_size_t]),
    'binf_hmc_sample_gauss_f64': (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                         _f64, _vp, _i64, _i64, _i32, _f64,
                                         _f64, _i32, _f64, _f64, _i32, _vp]),
    'binf_hmc_sample_n_gauss_f64': (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                           _vp, _vp, _f64, _vp, _i64, _i64,
                                           _i32, _i32, _i32, _f64, _f64, _i32,
                                           _f64, _f64, _i32, _vp]),
    'binf_hmc_gauss_waves_per_chain': (_i32, [_i64, _i64]),
    'binf_hmc_sample_gauss_big_workspace_bytes': (_i64, [_i64, _i64]),
    'binf_hmc_sample_gauss_big_f64': (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                             _f64, _vp, _i64, _i64, _i32, _f64,
                                             _f64, _i32, _f64, _f64, _i32, _vp,
                                             _i64, _vp]),
    'binf_hmc_sample_gauss_big_rng_f64': (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _f64, _vp,
                                                 _i64, _i64, _i32, _f64, _f64, _i32,
                                                 _f64, _f64, _i32, ctypes.c_uint64,
                                                 ctypes.c_uint64, _i64, _vp, _i64, _vp]),
    'binf_hmc_sample_n_gauss_big_workspace_bytes': (_i64, [_i64, _i64]),
    'binf_hmc_sample_n_gauss_big_f64': (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                               _f64, _vp, _i64, _i64, _i32, _i32, _i32, _f64,
                                               _f64, _i32, _f64, _f64, _i32, _vp, _i64, _vp]),
    'binf_hmc_sample_n_gauss_big_rng_f64': (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _f64, _vp,
                                                   _i64, _i64, _i32, _i32, _i32, _f64, _f64,
                                                   _i32, _f64, _f64, _i32, _u64, _u64, _i64,
                                                   _vp, _i64, _vp]),
    'binf_hmc_gauss_big_rng_draws_f64': (_i32, [_vp, _vp, _i64, _i64, ctypes.c_uint64,
                                                ctypes.c_uint64, _i64, _vp]),
    'binf_hmc_sample_n_gauss_rng_f64': (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                               _f64, _vp, _i64, _i64, _i32, _i32,
                                               _i32, _f64, _f64, _i32, _f64, _f64,
                                               _i32, ctypes.c_uint64,
                                               ctypes.c_uint64, _i64, _vp]),
    'binf_hmc_gauss_rng_draws_f64': (_i32, [_vp, _vp, _i64, _i64, _i32,
                                            ctypes.c_uint64, ctypes.c_uint64, _i64, _vp]),
    'binf_hmc_sample_poly_f64': (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                        _vp, _vp, _f64, _vp, _vp, _vp, _i32,
                                        _vp, _vp, _f64, _vp, _i64, _i64, _i64,
                                        _i32, _i32, _f64, _f64, _i32, _vp]),
    'binf_clipped_exp_f64': (_i32, [_vp, _vp, _i64, _vp]),
    'binf_row_sum_f64': (_i32, [_vp, _vp, _i64, _i64, _i32, _f64, _f64, _vp]),
    'binf_hmc_energy_f64': (_i32, [_vp, _vp, _vp, _i64, _i64, _vp]),
    'binf_gamma_logp_f64': (_i32, [_vp, _f64, _f64, _vp, _i64, _vp]),
    'binf_leapfrog_kick_f64': (_i32, [_vp, _vp, _f64, _vp, _i32, _i64, _i64,
                                      _i32, _vp]),
    'binf_leapfrog_drift_f64': (_i32, [_vp, _vp, _f64, _vp, _i64, _i64, _i32,
                                       _vp]),
    'binf_leapfrog_kick_drift_f64': (_i32, [_vp, _vp, _vp, _f64, _vp, _i64, _i64,
                                            _i32, _vp]),
    'binf_gauss_grad_f64': (_i32, [_vp, _vp, _f64, _f64, _i64, _i64, _vp]),
    'binf_accept_select_f64': (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                      _i32, _f64, _f64, _i64, _i64, _vp]),
    'binf_accept_decide_f64': (_i32, [_vp, _vp, _vp, _vp, _i64, _vp]),
    'binf_row_sumsq_diff_f64': (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _f64,
                                       _vp]),
    'binf_poly_forward_f64': (_i32, [_vp, _vp, _vp, _i64, _i64, _i64, _vp]),
    'binf_predictive_density_workspace_bytes': (_i64, [_i64, _i64, _i64]),
    'binf_predictive_density_f64': (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _f64, _vp, _i64, _vp]),
    'binf_gauss_err_grad_f64': (_i32, [_vp, _vp, _f64, _vp, _vp, _i64, _i64,
                                       _vp]),
    'binf_gauss_err_logp_f64': (_i32, [_vp, _vp, _f64, _vp, _vp, _i64, _i64,
                                       _vp]),
    'binf_poly_gauss_logp_f64': (_i32, [_vp, _vp, _vp, _f64, _vp, _vp, _i64,
                                        _i64, _i64, _vp]),
    'binf_poly_gauss_logp_memo_f64': (_i32, [_vp, _vp, _vp, _f64, _vp, _vp, _vp, _vp, _vp,
                                             _i64, _i64, _i64, _vp]),
    'binf_poly_gauss_grad_workspace_bytes': (_i64, [_i64, _i64, _i64]),
    'binf_poly_gauss_grad_f64': (_i32, [_vp, _vp, _vp, _f64, _vp, _vp, _vp,
                                        _i64, _i64, _i64, _i64, _vp]),
    'binf_linear_forward_f64': (_i32, [_vp, _vp, _vp, _i64, _i64, _i64, _vp]),
    'binf_linear_gauss_logp_workspace_bytes': (_i64, [_i64, _i64, _i64]),
    'binf_linear_gauss_logp_f64': (_i32, [_vp, _vp, _vp, _f64, _vp, _vp, _vp,
                                          _i64, _i64, _i64, _i64, _vp]),
    'binf_glm_pointwise_f64': (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _i64, _i64, _vp]),
    'binf_linear_glm_logp_workspace_bytes': (_i64, [_i64, _i64, _i64]),
    'binf_linear_glm_logp_f64': (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _f64, _vp, _vp, _i64,
                                        _i64, _i64, _i64, _vp]),
    'binf_linear_glm_grad_workspace_bytes': (_i64, [_i64, _i64, _i64]),
    'binf_linear_glm_grad_f64': (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _i64, _i64,
                                        _i64, _i64, _vp]),
    'binf_linear_glm_leapfrog_workspace_bytes': (_i64, [_i64, _i64, _i64]),
    'binf_linear_glm_leapfrog_f64': (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _f64, _f64,
                                            _vp, _i64, _i64, _i64, _i64, _f64, _vp, _i32, _i32,
                                            _vp]),
    'binf_negbin_count_term_f64': (_i32, [_vp, _vp, _i64, _f64, _vp, _vp, _i64, _vp, _i64, _vp]),
    'binf_negbin_pointwise_f64': (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64,
                                         _i64, _vp]),
    'binf_linear_negbin_logp_f64': (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64,
                                           _i64, _i64, _vp]),
    'binf_linear_negbin_grad_f64': (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64,
                                           _i64, _vp]),
    'binf_linear_negbin_leapfrog_f64': (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _f64, _f64,
                                               _vp, _i64, _i64, _i64, _i64, _f64, _vp, _i32,
                                               _i32, _vp]),
    'binf_gamma_precision_update_f64': (_i32, [_vp, _vp, _f64, _vp, _i64, _vp]),
    'binf_poly_leapfrog_workspace_bytes': (_i64, [_i64, _i64, _i64]),
    'binf_poly_leapfrog_f64': (_i32, [_vp, _vp, _vp, _vp, _f64, _vp, _vp, _i64, _i64, _i64, _i64,
                                      _f64, _vp, _i32, _i32, _vp]),
    'binf_pairdist_chi2_workspace_bytes': (_i64, [_i64, _i64, _i64]),
    'binf_pairdist_gauss_logp_f64': (_i32, [_vp, _vp, _vp, _vp, _f64, _vp, _vp, _i64,
                                            _i64, _i64, _vp, _i64, _vp]),
    'binf_pairdist_gauss_logp_memo_f64': (_i32, [_vp, _vp, _vp, _vp, _f64, _vp, _vp, _vp, _vp, _vp,
                                                 _i64, _i64, _i64, _vp, _i64, _vp]),
    'binf_pairdist_forward_f64': (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _i64,
                                         _vp]),
    'binf_pairdist_gauss_grad_f64': (_i32, [_vp, _vp, _f64, _vp, _vp, _i64,
                                            _i64, _vp]),
    'binf_pairdist_leapfrog_f64': (_i32, [_vp, _vp, _vp, _f64, _vp, _i32, _f64,
                                          _f64, _i32, _f64, _vp, _i32, _i64,
                                          _i64, _i32, _vp]),
    'binf_pairdist_hmc_energy_f64': (_i32, [_vp, _vp, _vp, _vp, _vp, _f64, _vp, _f64, _f64, _i32,
                                            ctypes.POINTER(_i32), _vp, _f64, _vp, _f64,
                                            _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _i64, _vp]),
    'binf_pairdist_packed_targets_bytes': (_i64, [_i64]),
    'binf_pairdist_pack_targets_f64': (_i32, [_vp, _vp, _i64, _vp]),
    'binf_pairdist_tiles_workspace_bytes': (_i64, [_i64, _i64]),
    'binf_pairdist_gauss_grad_packed_f64': (_i32, [_vp, _vp, _vp, _f64, _vp, _vp, _i64,
                                                   _i64, _vp, _i64, _vp]),
    'binf_pairdist_leapfrog_packed_f64': (_i32, [_vp, _vp, _vp, _vp, _vp, _f64, _vp, _i32, _f64,
                                                 _f64, _i32, _f64, _vp, _i32, _i64,
                                                 _i64, _i32, _vp, _i64, _vp]),
    'binf_rng_uniform_f64': (_i32, [_vp, _i64, ctypes.c_uint64, ctypes.c_uint64,
                                    _i64, _vp]),
    'binf_rng_normal_f64': (_i32, [_vp, _i64, ctypes.c_uint64, ctypes.c_uint64,
                                   _i64, _vp]),
    'binf_rng_normal_zig_uniform_f64': (_i32, [_vp, _i64, _vp, _i64, ctypes.c_uint64, ctypes.c_uint64,
                                               ctypes.c_uint64, _i64, _i64, _vp]),
    'binf_rng_normal_zig_f64': (_i32, [_vp, _i64, ctypes.c_uint64,
                                       ctypes.c_uint64, _i64, _vp]),
    'binf_rng_gamma_f64': (_i32, [_vp, _i64, _f64, ctypes.c_uint64,
                                  ctypes.c_uint64, _i64, _vp]),
    'binf_rwmc_propose_f64': (_i32, [_vp, _vp, _vp, _f64, _i64, _i64, ctypes.c_uint64,
                                     ctypes.c_uint64, _i64, _vp]),
    'binf_rwmc_accept_f64': (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64,
                                    ctypes.c_uint64, ctypes.c_uint64, _i64, _vp]),
    'binf_replica_gather_f64': (_i32, [_vp, _vp, _i64, _i64, _i64, _i32, _vp]),
    'binf_replica_swap_f64': (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64,
                                     _i64, _i32, _u64, _u64, _i64, _vp]),
    'binf_replica_work_f64': (_i32, [_vp, _vp, _vp, _i64, _i64, _i32, _vp]),
    'binf_free_energy_chunk': (_i32, []),
    'binf_free_energy_bar_workspace_bytes': (_i64, [_i64, _i64, _i64, _i64]),
    'binf_free_energy_bar_f64': (_i32, [_vp, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp,
                                        _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    'binf_smc_temper_f64': (_i32, [_vp, _vp, _i64, _i64, _i64, _f64, _i32, _vp, _vp, _vp, _vp, _vp,
                                   _vp, _vp, _vp]),
    'binf_smc_resample_f64': (_i32, [_vp, _vp, _vp, _i64, _i64, _i64, _u64, _u64, _i64, _vp, _vp,
                                     _vp]),
    'binf_smc_gather_f64': (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _i64, _i64, _vp]),
    'binf_chain_moments_f64': (_i32, [_vp, _i64, _i64, _i64, _i64, _i64, _i64, _i32, _vp, _vp, _vp]),
    'binf_chain_autocov_workspace_bytes': (_i64, [_i64, _i64, _i64]),
    'binf_chain_autocov_f64': (_i32, [_vp, _i64, _i64, _i64, _i64, _i64, _i64, _i32, _vp, _i64,
                                      _vp, _i64, _vp]),
    'binf_diag_summary_workspace_bytes': (_i64, [_i64, _i64]),
    'binf_diag_summary_f64': (_i32, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp,
                                     _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    'binf_rank_sort_workspace_bytes': (_i64, [_i64, _i64]),
    'binf_rank_normalise_f64': (_i32, [_vp, _i64, _i64, _i64, _i64, _i64, _i64, _i32, _vp, _vp, _vp,
                                       _vp, _i64, _vp]),
    'binf_sorted_quantiles_f64': (_i32, [_vp, _i64, _i64, ctypes.POINTER(ctypes.c_double), _i32,
                                         _vp, _vp]),
    'binf_draws_map_f64': (_i32, [_vp, _i64, _i64, _i64, _i64, _i64, _i64, _i32, _i32, _vp, _vp, _vp]),
    'binf_rank_diag_combine_f64': (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp,
                                          _vp, _vp]),
    'binf_gauss_pointwise_loglik_f64': (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _f64, _vp]),
    'binf_psis_loo_workspace_bytes': (_i64, [_i64, _i64]),
    'binf_psis_loo_f64': (_i32, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    'binf_pointwise_totals_f64': (_i32, [_vp, _vp, _i64, _i64, _vp, _f64, _vp, _vp]),
    'binf_leapfrog_kick_scaled_f64': (_i32, [_vp, _vp, _vp, _i64, _f64, _vp, _i32, _i64, _i64,
                                             _i32, _vp]),
    'binf_leapfrog_drift_scaled_f64': (_i32, [_vp, _vp, _vp, _i64, _f64, _vp, _i64, _i64, _i32,
                                              _vp]),
    'binf_leapfrog_kick_drift_scaled_f64': (_i32, [_vp, _vp, _vp, _vp, _i64, _f64, _vp, _i64,
                                                   _i64, _i32, _vp]),
    'binf_metric_accumulate_f64': (_i32, [_vp, _vp, _vp, _vp, _i32, _i64, _i64, _vp]),
    'binf_metric_pool_f64': (_i32, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _vp, _vp]),
    'binf_leapfrog_kick_dense_f64': (_i32, [_vp, _vp, _vp, _i64, _f64, _vp, _i32, _i64, _i64,
                                            _i32, _vp]),
    'binf_leapfrog_drift_dense_f64': (_i32, [_vp, _vp, _vp, _i64, _f64, _vp, _i64, _i64, _i32,
                                             _vp]),
    'binf_leapfrog_kick_drift_dense_f64': (_i32, [_vp, _vp, _vp, _vp, _i64, _f64, _vp, _i64,
                                                  _i64, _i32, _vp]),
    'binf_metric_comoments_f64': (_i32, [_vp, _vp, _vp, _vp, _i32, _i64, _i64, _i64, _vp]),
    'binf_metric_factor_f64': (_i32, [_vp, _vp, _i64, _i64, _i64, _i64, _i32, _vp, _vp, _vp, _vp]),
    'binf_gibbs_poly_sample_n_f64': (_i32, [_vp, _vp]),
    'binf_nuts_begin_f64': (_i32, [_vp, _vp]),
    'binf_nuts_leaf_f64': (_i32, [_vp, _vp]),
    'binf_nuts_pending': (_i32, [_vp, _i64, _vp, _vp]),
    'binf_nuts_adapt_step_f64': (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _f64, _f64, _f64, _f64,
                                        _i32, _i64, _vp]),
    'binf_chees_accept_prob_f64': (_i32, [_vp, _vp, _vp, _i64, _vp]),
    'binf_chees_workspace_bytes': (_i64, [_i64, _i64]),
    'binf_chees_means_f64': (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp]),
    'binf_chees_terms_f64': (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp]),
    'binf_chees_sums_f64': (_i32, [_vp, _vp, _vp, _vp, _i64, _vp]),
    'binf_linear_resident_supported': (_i32, [_i64, _i64]),
    'binf_hmc_sample_linear_f64': (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                          _vp, _vp, _f64, _vp, _vp, _vp, _i32,
                                          _vp, _vp, _f64, _vp, _i64, _i64, _i64,
                                          _i32, _i32, _f64, _f64, _i32, _vp]),
    'binf_gibbs_linear_sample_n_f64': (_i32, [_vp, _vp]),
    'binf_jacobian_contract_f64': (_i32, [_vp, _vp, _vp, _i64, _i64, _i64, _i32, _vp]),
    'binf_sum_terms_f64': (_i32, [_vp, _vp, _i32, _vp, _i64, _vp]),
    'binf_sum_terms_bcast_f64': (_i32, [_vp, _vp, _vp, _i32, _vp, _i64, _vp]),
    'binf_rng_philox4x32_10': (_i32, [ctypes.POINTER(ctypes.c_uint32),
                                      ctypes.POINTER(ctypes.c_uint32),
                                      ctypes.POINTER(ctypes.c_uint32)]),
    'binf_pairwise_tree_height': (_i32, [_i64]),
    'binf_pairwise_leaf': (_i32, [_i64, _i32, _i32,
                                  ctypes.POINTER(_i64), ctypes.POINTER(_i64),
                                  ctypes.POINTER(_i32), ctypes.POINTER(_i32)]),
}

ABI_VERSION = 7        # keep in step with BINF_ABI_VERSION (include/binf_hip.h)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeLibraryError(
                '%s not found: build it with `python -c "import '
                '__graft_entry__ as g; g.build()"` (hipcc --offload-arch='
                'gfx950).  binf_amd has no CPU fallback.' % LIB_PATH)
        try:
            L = ctypes.CDLL(LIB_PATH)
        except OSError as e:
            raise NativeLibraryError('cannot load %s: %s' % (LIB_PATH, e))
        for name, (res, args) in SIGNATURES.items():
            try:
                f = getattr(L, name)
            except AttributeError:
                raise NativeLibraryError('%s does not export %s (stale '
                                         'build?)' % (LIB_PATH, name))
            f.restype = res
            f.argtypes = args
        v = L.binf_abi_version()
        if v != ABI_VERSION:
            raise NativeLibraryError('ABI version %d != expected %d'
                                     % (v, ABI_VERSION))
        _lib = L
    return _lib


def last_error():
    buf = ctypes.create_string_buffer(512)
    lib().binf_last_error(buf, 512)
    return buf.value.decode('utf-8', 'replace')


def check(rc, what):
    """Map a C-ABI return code onto the exception classes the reference
    raises for the same mistakes (ValueError / NotImplementedError)."""
    if rc == 0:
        return
    msg = '%s: %s' % (what, last_error())
    if rc in (E_ARG, E_ALIAS):
        raise ValueError(msg)
    if rc == E_UNSUPPORTED:
        raise NotImplementedError(msg)
    raise NativeLibraryError(msg + ' [hipError_t %d]' % rc)


def dptr(t, dtype=torch.float64, numel=None, name='tensor'):
    """Device pointer of a contiguous ROCm tensor, with the shape checks the
    kernels rely on (a wrong size here would be an out-of-bounds access)."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        raise TypeError('%s must be a torch.Tensor' % name)
    if not t.is_cuda:
        raise ValueError('%s must live in GPU memory (got %s)'
                         % (name, t.device))
    if t.dtype != dtype:
        raise ValueError('%s must be %s (got %s)' % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError('%s must be contiguous' % name)
    if numel is not None and t.numel() != numel:
        raise ValueError('%s has %d elements, expected %d'
                         % (name, t.numel(), numel))
    return t.data_ptr()


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def stream_handle(device=None):
    """hipStream_t of torch's current stream on ``device`` (as an integer)."""
    if _raw_stream is not None:
        # the raw handle without building a torch.cuda.Stream object (~4 us less per launch)
        idx = device.index if isinstance(device, torch.device) and device.index is not None \
            else torch.cuda.current_device()
        return _raw_stream(idx)
    return torch.cuda.current_stream(device).cuda_stream


_n_devices = None


def _launcher(fn):
    """Every wrapper that enqueues a kernel: all tensor arguments must live on
    ONE device, and the launch runs with that device current (the stream handle
    passed to the C ABI belongs to it)."""
    import functools

    @functools.wraps(fn)
    def guarded(*args, **kw):
        # a process that sees ONE device cannot mix devices: nothing to check
        # (the check costs ~2 us per launch, a fifth of a small launch's host time)
        global _n_devices
        if _n_devices is None:
            _n_devices = torch.cuda.device_count()
        if _n_devices <= 1:
            return fn(*args, **kw)
        dev = None
        for a in list(args) + list(kw.values()):
            if isinstance(a, torch.Tensor) and a.is_cuda:
                if dev is None:
                    dev = a.device
                elif a.device != dev:
                    raise ValueError('%s: tensors on different devices (%s and %s)'
                                     % (fn.__name__, dev, a.device))
        if dev is None or dev.index == torch.cuda.current_device():
            return fn(*args, **kw)
        with torch.cuda.device(dev):
            return fn(*args, **kw)
    return guarded


def pairwise_tree_height(n):
    return lib().binf_pairwise_tree_height(int(n))


def pairwise_leaf(n, H, path):
    off, ln = _i64(), _i64()
    depth, canon = _i32(), _i32()
    rc = lib().binf_pairwise_leaf(int(n), int(H), int(path),
                                  ctypes.byref(off), ctypes.byref(ln),
                                  ctypes.byref(depth), ctypes.byref(canon))
    check(rc, 'binf_pairwise_leaf')
    return off.value, ln.value, depth.value, canon.value


@_launcher
def hmc_sample_gauss(q0, p0, u, q_out, accepted, n_accepted, e_before, e_after, timestep,
                     dt_chain, nsteps, k, x0, adapt, uprate, downrate,
                     mode=MODE_EXACT):
    """binf_hmc_sample_gauss_f64 on torch's current stream."""
    if q0.dim() != 2:
        raise ValueError('q0 must be [n_chains, n_dims]')
    C, D = q0.shape
    n = C * D
    rc = lib().binf_hmc_sample_gauss_f64(
        dptr(q0, numel=n, name='q0'), dptr(p0, numel=n, name='p0'),
        dptr(u, numel=C, name='u'), dptr(q_out, numel=n, name='q_out'),
        dptr(accepted, torch.uint8, C, 'accepted'),
        dptr(n_accepted, torch.int64, C, 'n_accepted'),
        dptr(e_before, numel=C, name='e_before'),
        dptr(e_after, numel=C, name='e_after'),
        float(timestep), dptr(dt_chain, numel=C, name='dt_chain'),
        C, D, int(nsteps), float(k), float(x0), int(bool(adapt)),
        float(uprate), float(downrate), int(mode), stream_handle(q0.device))
    check(rc, 'binf_hmc_sample_gauss_f64')


ROW_SUM, ROW_SUMSQ, ROW_SUMSQ_SHIFT = 0, 1, 2


def _cd(x):
    if x.dim() != 2:
        raise ValueError('expected a [n_chains, n_dims] tensor, got shape %s'
                         % (tuple(x.shape),))
    return x.shape


@_launcher
def row_sum(x, op=ROW_SUM, shift=0.0, scale=1.0, out=None):
    """scale * np.sum(f(x[c, :])) per chain, numpy pairwise order."""
    C, D = _cd(x)
    if out is None:
        out = torch.empty(C, dtype=torch.float64, device=x.device)
    rc = lib().binf_row_sum_f64(dptr(x, numel=C * D, name='x'),
                                dptr(out, numel=C, name='out'), C, D, int(op),
                                float(shift), float(scale),
                                stream_handle(x.device))
    check(rc, 'binf_row_sum_f64')
    return out


@_launcher
def hmc_energy(p, log_prob):
    """``-log_prob + 0.5 * np.sum(p**2)`` per chain (hmc.py:143,148,150), one
    launch; ``log_prob`` is a contiguous ``[C]`` tensor."""
    C, D = _cd(p)
    out = torch.empty(C, dtype=torch.float64, device=p.device)
    rc = lib().binf_hmc_energy_f64(dptr(p, numel=C * D, name='p'),
                                   dptr(log_prob, numel=C, name='log_prob'), dptr(out), C, D,
                                   stream_handle(p.device))
    check(rc, 'binf_hmc_energy_f64')
    return out


def _groups(t, C, D, k, name, units):
    """``G`` of ``t``, one rank-``k`` block of extent ``D`` per group or a single block without
    the leading ``G`` (``k`` = 1: the rows of a ``[G x D]`` scale; 2: ``[G x D x D]`` factors),
    serving ``C`` chains; ``name`` and ``units`` word the refusals."""
    nd = t.dim()
    if nd not in (k, k + 1) or t.shape[-1] != D or (k == 2 and t.shape[-2] != D):
        dims = 'D, D' if k == 2 else 'D'
        raise ValueError('%s must be [%s] or [G, %s] with D = %d, got shape %s'
                         % (name, dims, dims, D, tuple(t.shape)))
    G = 1 if nd == k else t.shape[0]
    if G < 1 or C % G != 0:
        raise ValueError('%s has %d %s: not a divisor of the %d chains' % (name, G, units, C))
    return G


_SCALE_ROWS = (1, 'scale', 'rows')           # _groups(scale, C, D, *_SCALE_ROWS)
_CHOL_FACTORS = (2, 'chol', 'factors')

# The nine per-step leapfrog launchers -- leapfrog_{kick,drift,kick_drift}[_scaled|_dense] --
# are one body: the piece's [C x D] buffers, the metric with its G where there is one, the
# step, `half` for a kick, sizes, mode, stream.  They are generated from it as straight-line
# code: a launch of a small batch is host-bound, and the same body as one shared function
# (buffers and metric handed over as tuples) cost 1.4 us more per identity launch and 2.6 us
# more per metric launch than the 5 ... 8 us these take.  The signatures:
#     leapfrog_kick[_scaled|_dense](p, grad, [scale|chol,] timestep, dt_chain=None,
#                                   half=False, mode=MODE_EXACT)
#     leapfrog_drift[_scaled|_dense](q, p, [scale|chol,] timestep, dt_chain=None, mode=MODE_EXACT)
#     leapfrog_kick_drift[_scaled|_dense](q, p, grad, [scale|chol,] timestep, dt_chain=None,
#                                         mode=MODE_EXACT)
_LEAPFROG_LAUNCHER = '''
@_launcher
def leapfrog_{piece}{suffix}({bufs}, {metric}timestep, dt_chain=None, {half}mode=MODE_EXACT):
    """{doc}  (``binf_leapfrog_{piece}{suffix}_f64``)."""
    C, D = _cd({first})
    {groups}rc = lib().binf_leapfrog_{piece}{suffix}_f64(
        {ptrs}, {metric_ptr}float(timestep), dptr(dt_chain, numel=C, name='dt_chain'),
        {half_arg}C, D, int(mode), stream_handle({first}.device))
    check(rc, 'binf_leapfrog_{piece}{suffix}_f64')
'''


def _define_leapfrog_launchers():
    pieces = (('kick', ('p', 'grad'), 'p -= h * grad, h = dt * M (``half``: 0.5 * dt first)'),
              ('drift', ('q', 'p'), 'q += p * h, h = dt * M'),
              ('kick_drift', ('q', 'p', 'grad'), 'The kick, then the drift with the new p, in one launch'))
    # suffix, argument, its group check, elements per group, in words
    metrics = (('', None, None, None, 'M the identity'),
               ('_scaled', 'scale', '_SCALE_ROWS', 'D', 'M = scale[c % G], ``[G x D]`` or ``[D]``'),
               ('_dense', 'chol', '_CHOL_FACTORS', 'D * D', 'M = the lower factor chol[c % G] (kick: its transpose), '
                                           '``[G x D x D]`` or ``[D x D]``'))
    for piece, bufs, doc in pieces:
        for suffix, m, kind, per_group, mdoc in metrics:
            source = _LEAPFROG_LAUNCHER.format(
                piece=piece, suffix=suffix, bufs=', '.join(bufs), first=bufs[0], doc='%s; %s' % (doc, mdoc),
                ptrs=', '.join("dptr(%s, numel=C * D, name='%s')" % (b, b) for b in bufs),
                metric='' if m is None else m + ', ',
                groups='' if m is None else 'G = _groups(%s, C, D, *%s)\n    ' % (m, kind),
                metric_ptr='' if m is None else "dptr(%s, numel=G * %s, name='%s'), G, " % (m, per_group, m),
                half='half=False, ' if piece == 'kick' else '',
                half_arg='int(bool(half)), ' if piece == 'kick' else '')
            # a file name of its own, with the text on record: tracebacks and inspect.getsource show it
            name = '<binf_amd._native.leapfrog_%s%s>' % (piece, suffix)
            linecache.cache[name] = (len(source), None, source.splitlines(True), name)
            exec(compile(source, name, 'exec'), globals())


_define_leapfrog_launchers()


@_launcher
def metric_accumulate(x, k0, s1, s2, first):
    """One state ``x [C x D]`` into the running moments ``k0, s1, s2`` (``[C x D]`` each,
    caller-owned; ``first`` starts them) -- ``binf_metric_accumulate_f64``."""
    C, D = _cd(x)
    n = C * D
    rc = lib().binf_metric_accumulate_f64(
        dptr(x, numel=n, name='x'), dptr(k0, numel=n, name='k0'), dptr(s1, numel=n, name='s1'),
        dptr(s2, numel=n, name='s2'), int(bool(first)), C, D, stream_handle(x.device))
    check(rc, 'binf_metric_accumulate_f64')


@_launcher
def metric_pool(k0, s1, s2, n, scale, regularise=True):
    """The pooled per-group standard deviation of ``n`` accumulated draws per chain, written
    into ``scale [G x D]`` in place (``binf_metric_pool_f64``; no host read-back)."""
    C, D = _cd(k0)
    G = _groups(scale, C, D, *_SCALE_ROWS)
    rc = lib().binf_metric_pool_f64(
        dptr(k0, numel=C * D, name='k0'), dptr(s1, numel=C * D, name='s1'),
        dptr(s2, numel=C * D, name='s2'), int(n), C, D, G, int(bool(regularise)),
        dptr(scale, numel=G * D, name='scale'), stream_handle(k0.device))
    check(rc, 'binf_metric_pool_f64')


@_launcher
def metric_comoments(x, k0, s1, s2, first):
    """One state ``x [C x D]`` into the pooled co-moments of each group: ``k0, s1 [G x D]``,
    ``s2 [G x D x D]`` (lower triangle), caller-owned; ``first`` starts them
    (``binf_metric_comoments_f64``)."""
    C, D = _cd(x)
    G = _groups(s2, C, D, *_CHOL_FACTORS)
    rc = lib().binf_metric_comoments_f64(
        dptr(x, numel=C * D, name='x'), dptr(k0, numel=G * D, name='k0'),
        dptr(s1, numel=G * D, name='s1'), dptr(s2, numel=G * D * D, name='s2'),
        int(bool(first)), C, D, G, stream_handle(x.device))
    check(rc, 'binf_metric_comoments_f64')


@_launcher
def metric_factor(s1, s2, n, C, chol, work, status=None, regularise=True):
    """The pooled covariance of ``n`` accumulated states of ``C`` chains and its lower
    Cholesky factor, built in ``work`` and copied into ``chol [G x D x D]`` in place for the
    groups where it exists (``status [G]`` int32: 0 updated, 1 kept) --
    ``binf_metric_factor_f64``; no host read-back."""
    D = s2.shape[-1]
    G = _groups(s2, int(C), D, *_CHOL_FACTORS)
    rc = lib().binf_metric_factor_f64(
        dptr(s1, numel=G * D, name='s1'), dptr(s2, numel=G * D * D, name='s2'), int(n), int(C),
        D, G, int(bool(regularise)), dptr(chol, numel=G * D * D, name='chol'),
        dptr(work, numel=G * D * D, name='work'), dptr(status, torch.int32, G, 'status'),
        stream_handle(s2.device))
    check(rc, 'binf_metric_factor_f64')


@_launcher
def gauss_grad(x, k, x0, out=None):
    C, D = _cd(x)
    if out is None:
        out = torch.empty_like(x)
    rc = lib().binf_gauss_grad_f64(dptr(x, numel=C * D, name='x'),
                                   dptr(out, numel=C * D, name='out'),
                                   float(k), float(x0), C, D,
                                   stream_handle(x.device))
    check(rc, 'binf_gauss_grad_f64')
    return out


@_launcher
def accept_select(q_prop, q_old, e_before, e_after, u, q_out, accepted,
                  n_accepted=None, dt_chain=None, adapt=False, uprate=1.05, downrate=0.95):
    C, D = _cd(q_prop)
    n = C * D
    rc = lib().binf_accept_select_f64(
        dptr(q_prop, numel=n, name='q_prop'), dptr(q_old, numel=n, name='q_old'),
        dptr(e_before, numel=C, name='e_before'),
        dptr(e_after, numel=C, name='e_after'), dptr(u, numel=C, name='u'),
        dptr(q_out, numel=n, name='q_out'),
        dptr(accepted, torch.uint8, C, 'accepted'),
        dptr(n_accepted, torch.int64, C, 'n_accepted'),
        dptr(dt_chain, numel=C, name='dt_chain'), int(bool(adapt)),
        float(uprate), float(downrate), C, D, stream_handle(q_prop.device))
    check(rc, 'binf_accept_select_f64')


@_launcher
def accept_decide(u, x, delta):
    """The three-way accept test of an exponent known to within ``delta`` (int32 per
    element: 0 rejected, 1 accepted, 2 undecided)."""
    require_device(u, 'u')
    n = u.numel()
    out = torch.empty(n, dtype=torch.int32, device=u.device)
    rc = lib().binf_accept_decide_f64(dptr(u, numel=n, name='u'), dptr(x, numel=n, name='x'),
                                      dptr(delta, numel=n, name='delta'),
                                      dptr(out, torch.int32, n, 'out'), n,
                                      stream_handle(u.device))
    check(rc, 'binf_accept_decide_f64')
    return out


@_launcher
def clipped_exp(x):
    """exp(clip(x, -308, 709)) elementwise (csb.numeric.exp)."""
    require_device(x, 'x')
    xc = x.contiguous()
    out = torch.empty_like(xc)
    rc = lib().binf_clipped_exp_f64(dptr(xc), dptr(out), xc.numel(),
                                    stream_handle(x.device))
    check(rc, 'binf_clipped_exp_f64')
    return out


def require_device(x, what):
    """The package computes on the GPU only: ``x`` must be a ROCm tensor.
    Raises TypeError otherwise (there is no numpy / CPU evaluation path)."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda):
        raise TypeError('%s must be a ROCm (cuda) fp64 tensor, got %s; binf_amd '
                        'evaluates on the GPU only (no CPU path)'
                        % (what, type(x).__name__ if not isinstance(x, torch.Tensor)
                           else 'a %s tensor' % x.device.type))
    return x


def _precision_args(precision, C, device):
    """(host scalar, per-chain tensor or None) from a float or a [C] tensor."""
    if isinstance(precision, torch.Tensor):
        if precision.dim() == 0:
            return float(precision), None
        p = precision.reshape(-1)
        if p.numel() != C:
            raise ValueError('precision has %d entries for %d chains'
                             % (p.numel(), C))
        return 0.0, p.contiguous()
    return float(precision), None


@_launcher
def row_sumsq_diff(x, y, scale=1.0, weights=None):
    C, D = _cd(x)
    out = torch.empty(C, dtype=torch.float64, device=x.device)
    rc = lib().binf_row_sumsq_diff_f64(dptr(x, numel=C * D, name='x'),
                                       dptr(y, numel=D, name='y'),
                                       dptr(weights, numel=D, name='weights'),
                                       dptr(out), C, D, float(scale),
                                       stream_handle(x.device))
    check(rc, 'binf_row_sumsq_diff_f64')
    return out


@_launcher
def poly_forward(coeffs, xs):
    C, K = _cd(coeffs)
    N = xs.numel()
    out = torch.empty((C, N), dtype=torch.float64, device=coeffs.device)
    rc = lib().binf_poly_forward_f64(dptr(coeffs, numel=C * K, name='coeffs'),
                                     dptr(xs, numel=N, name='xs'), dptr(out),
                                     C, K, N, stream_handle(coeffs.device))
    check(rc, 'binf_poly_forward_f64')
    return out


@_launcher
def predictive_density(mock, precision, ys, half_log_2pi):
    """binf_predictive_density_f64: ``mock`` [S x nx], ``precision`` [S], ``ys``
    [nx x ny] -> densities [nx x ny] (``binf/example/misc.py:3-16`` for a grid)."""
    S, nx = _cd(mock)
    if ys.dim() != 2 or ys.shape[0] != nx:
        raise ValueError('predictive_density: ys must be [nx x ny] with nx = %d' % nx)
    ny = ys.shape[1]
    out = torch.empty((nx, ny), dtype=torch.float64, device=mock.device)
    need = lib().binf_predictive_density_workspace_bytes(S, nx, ny)
    ws = torch.empty(need // 8, dtype=torch.float64, device=mock.device) if need > 0 else None
    rc = lib().binf_predictive_density_f64(dptr(mock, numel=S * nx, name='mock'),
                                           dptr(precision, numel=S, name='precision'),
                                           dptr(ys, numel=nx * ny, name='ys'), dptr(out),
                                           S, nx, ny, float(half_log_2pi),
                                           None if ws is None else ws.data_ptr(), need,
                                           stream_handle(mock.device))
    check(rc, 'binf_predictive_density_f64')
    return out


@_launcher
def gauss_err_grad(mock, ys, precision):
    C, N = _cd(mock)
    tau, tau_chain = _precision_args(precision, C, mock.device)
    out = torch.empty_like(mock)
    rc = lib().binf_gauss_err_grad_f64(dptr(mock, numel=C * N, name='mock'),
                                       dptr(ys, numel=N, name='ys'), tau,
                                       dptr(tau_chain, numel=C, name='precision'),
                                       dptr(out), C, N,
                                       stream_handle(mock.device))
    check(rc, 'binf_gauss_err_grad_f64')
    return out


@_launcher
def gauss_err_logp(mock, ys, precision):
    C, N = _cd(mock)
    tau, tau_chain = _precision_args(precision, C, mock.device)
    out = torch.empty(C, dtype=torch.float64, device=mock.device)
    rc = lib().binf_gauss_err_logp_f64(dptr(mock, numel=C * N, name='mock'),
                                       dptr(ys, numel=N, name='ys'), tau,
                                       dptr(tau_chain, numel=C, name='precision'),
                                       dptr(out), C, N,
                                       stream_handle(mock.device))
    check(rc, 'binf_gauss_err_logp_f64')
    return out


@_launcher
def poly_gauss_logp(coeffs, xs, ys, precision):
    C, K = _cd(coeffs)
    N = xs.numel()
    tau, tau_chain = _precision_args(precision, C, coeffs.device)
    out = torch.empty(C, dtype=torch.float64, device=coeffs.device)
    rc = lib().binf_poly_gauss_logp_f64(
        dptr(coeffs, numel=C * K, name='coeffs'), dptr(xs, numel=N, name='xs'),
        dptr(ys, numel=N, name='ys'), tau,
        dptr(tau_chain, numel=C, name='precision'), dptr(out), C, K, N,
        stream_handle(coeffs.device))
    check(rc, 'binf_poly_gauss_logp_f64')
    return out


def new_chi2_memo(C, K, device):
    """Buffers of the two-entry per-chain chi^2 memo (include/binf_hip.h,
    binf_poly_gauss_logp_memo_f64): ``(memo_args [2 x C x K] NaN, memo_chi2 [2 x C] NaN,
    memo_state [2 x C] uint8 zero)``; ``memo_state[0]`` = chains the last call reused."""
    nan = float('nan')
    return (torch.full((2, C, K), nan, dtype=torch.float64, device=device),
            torch.full((2, C), nan, dtype=torch.float64, device=device),
            torch.zeros((2, C), dtype=torch.uint8, device=device))


@_launcher
def poly_gauss_logp_memo(coeffs, xs, ys, precision, memo):
    """binf_poly_gauss_logp_memo_f64; ``memo = new_chi2_memo(C, K, device)``."""
    C, K = _cd(coeffs)
    N = xs.numel()
    tau, tau_chain = _precision_args(precision, C, coeffs.device)
    mc, ms, sk = memo
    out = torch.empty(C, dtype=torch.float64, device=coeffs.device)
    rc = lib().binf_poly_gauss_logp_memo_f64(
        dptr(coeffs, numel=C * K, name='coeffs'), dptr(xs, numel=N, name='xs'),
        dptr(ys, numel=N, name='ys'), tau, dptr(tau_chain, numel=C, name='precision'), dptr(out),
        dptr(mc, numel=2 * C * K, name='memo_coeffs'), dptr(ms, numel=2 * C, name='memo_chi2'),
        dptr(sk, torch.uint8, 2 * C, 'memo_state'), C, K, N, stream_handle(coeffs.device))
    check(rc, 'binf_poly_gauss_logp_memo_f64')
    return out


@_launcher
def hmc_sample_poly(q0, p0, u, q_out, accepted, n_accepted, e_before, e_after,
                    xs, ys, precision, prior_means, prior_vars, prior_first,
                    lp_pre, lp_post, timestep, dt_chain, nsteps, adapt, uprate,
                    downrate, mode=MODE_EXACT):
    """binf_hmc_sample_poly_f64 on torch's current stream (K <= 16
    coefficients, <= 1024 data points; ``mode | MODE_LANE_PER_CHAIN``: one lane
    per chain, <= 128 data points)."""
    C, K = _cd(q0)
    N = xs.numel()
    tau, tau_chain = _precision_args(precision, C, q0.device)
    rc = lib().binf_hmc_sample_poly_f64(
        dptr(q0, numel=C * K, name='q0'), dptr(p0, numel=C * K, name='p0'),
        dptr(u, numel=C, name='u'), dptr(q_out, numel=C * K, name='q_out'),
        dptr(accepted, torch.uint8, C, 'accepted'),
        dptr(n_accepted, torch.int64, C, 'n_accepted'),
        dptr(e_before, numel=C, name='e_before'),
        dptr(e_after, numel=C, name='e_after'),
        dptr(xs, numel=N, name='xs'), dptr(ys, numel=N, name='ys'), tau,
        dptr(tau_chain, numel=C, name='precision'),
        dptr(prior_means, numel=K, name='prior_means'),
        dptr(prior_vars, numel=K, name='prior_vars'), int(bool(prior_first)),
        dptr(lp_pre, numel=C, name='lp_pre'), dptr(lp_post, numel=C, name='lp_post'),
        float(timestep), dptr(dt_chain, numel=C, name='dt_chain'), C, K, N,
        int(nsteps), int(bool(adapt)), float(uprate), float(downrate),
        int(mode), stream_handle(q0.device))
    check(rc, 'binf_hmc_sample_poly_f64')


def _gibbs_fields(model):
    return [('struct_size', _u64)] + \
        [(n, _vp) for n in ('coefficients', 'precision', 'coefficients_out', 'precision_out',
                            'rec_coefficients', 'rec_precision', 'accepted', 'n_accepted',
                            'e_before', 'e_after', model, 'ys', 'prior_means', 'prior_vars',
                            'p0', 'u', 'g', 'dt_chain')] + \
        [(n, _f64) for n in ('timestep', 'uprate', 'downrate', 'stepsize', 'gp_shape',
                             'gp_rate', 'gamma_shape', 'gamma_rate')] + \
        [(n, _i64) for n in ('C', 'K', 'N', 'chain_offset')] + \
        [(n, _u64) for n in ('seed_m', 'off_m', 'stride_m', 'seed_u', 'off_u', 'stride_u',
                             'seed_g', 'off_g', 'stride_g')] + \
        [(n, _i32) for n in ('move', 'mode', 'nsteps', 'n', 'thin', 'n_adapt', 'prior_first',
                             'gp_where', 'zig', 'keep_precision')]


class GibbsPolyArgs(ctypes.Structure):
    """``binf_gibbs_poly_args`` of include/binf_hip.h, field for field."""
    _fields_ = _gibbs_fields('xs')


class GibbsLinearArgs(ctypes.Structure):
    """``binf_gibbs_linear_args`` of include/binf_hip.h, field for field."""
    _fields_ = _gibbs_fields('design')


def _gibbs_sample_n(symbol, a, model_field, model, model_numel, N, coefficients, precision,
                    coefficients_out, precision_out, ys, n,
                    thin=1, move=MOVE_HMC, mode=MODE_EXACT, nsteps=1, timestep=0.0,
                    dt_chain=None, n_adapt=0, uprate=1.05, downrate=0.95, stepsize=0.0,
                    prior_means=None, prior_vars=None, prior_first=False, gp_where=0,
                    gp_shape=1.0, gp_rate=0.0, gamma_shape=1.0, gamma_rate=0.0,
                    rec_coefficients=None, rec_precision=None, accepted=None,
                    n_accepted=None, e_before=None, e_after=None, p0=None, u=None, g=None,
                    streams=None, chain_offset=0, zig=True, keep_precision=False):
    """Fill the argument block ``a`` of a multi-sweep entry point and call it."""
    C, K = _cd(coefficients)
    n, thin = int(n), int(thin)
    nrec = n // thin
    a.struct_size = ctypes.sizeof(a)
    a.coefficients = dptr(coefficients, numel=C * K, name='coefficients')
    a.precision = dptr(precision, numel=C, name='precision')
    a.coefficients_out = dptr(coefficients_out, numel=C * K, name='coefficients_out')
    a.precision_out = dptr(precision_out, numel=C, name='precision_out')
    a.rec_coefficients = dptr(rec_coefficients, numel=nrec * C * K, name='rec_coefficients')
    a.rec_precision = dptr(rec_precision, numel=nrec * C, name='rec_precision')
    a.accepted = dptr(accepted, torch.uint8, n * C, 'accepted')
    a.n_accepted = dptr(n_accepted, torch.int64, C, 'n_accepted')
    a.e_before = dptr(e_before, numel=n * C, name='e_before')
    a.e_after = dptr(e_after, numel=n * C, name='e_after')
    setattr(a, model_field, dptr(model, numel=model_numel, name=model_field))
    a.ys = dptr(ys, numel=N, name='ys')
    a.prior_means = dptr(prior_means, numel=K, name='prior_means')
    a.prior_vars = dptr(prior_vars, numel=K, name='prior_vars')
    a.p0 = dptr(p0, numel=n * C * K, name='p0')
    a.u = dptr(u, numel=n * C, name='u')
    a.g = dptr(g, numel=n * C, name='g')
    a.dt_chain = dptr(dt_chain, numel=C, name='dt_chain')
    a.timestep, a.uprate, a.downrate = float(timestep), float(uprate), float(downrate)
    a.stepsize = float(stepsize)
    a.gp_shape, a.gp_rate = float(gp_shape), float(gp_rate)
    a.gamma_shape, a.gamma_rate = float(gamma_shape), float(gamma_rate)
    a.C, a.K, a.N, a.chain_offset = C, K, N, int(chain_offset)
    sm, su, sg = streams if streams is not None else ((0, 0, 0),) * 3
    a.seed_m, a.off_m, a.stride_m = [int(v) for v in sm]
    a.seed_u, a.off_u, a.stride_u = [int(v) for v in su]
    a.seed_g, a.off_g, a.stride_g = [int(v) for v in sg]
    a.move, a.mode, a.nsteps, a.n, a.thin = int(move), int(mode), int(nsteps), n, thin
    a.n_adapt, a.prior_first, a.gp_where = int(n_adapt), int(bool(prior_first)), int(gp_where)
    a.zig = int(bool(zig))
    a.keep_precision = int(bool(keep_precision))
    rc = getattr(lib(), symbol)(ctypes.byref(a), stream_handle(coefficients.device))
    check(rc, symbol)


@_launcher
def gibbs_poly_sample_n(coefficients, precision, coefficients_out, precision_out, xs, ys, n,
                        thin=1, **kw):
    """binf_gibbs_poly_sample_n_f64 on torch's current stream: n sweeps of the
    example's Gibbs loop in one launch.  ``streams`` = ``((seed, offset, stride),) * 3``
    for the momentum / proposal, acceptance and gamma draws that are not supplied.
    Keywords: see :func:`_gibbs_sample_n`."""
    N = xs.numel()
    _gibbs_sample_n('binf_gibbs_poly_sample_n_f64', GibbsPolyArgs(), 'xs', xs, N, N,
                    coefficients, precision, coefficients_out, precision_out, ys, n, thin, **kw)


# -- no-U-turn sampler (csrc/nuts.hip) -----------------------------------------------------
NUTS_RUN, NUTS_TURN, NUTS_SUBTURN, NUTS_MAXD, NUTS_DIV = 0, 1, 2, 3, 4
NUTS_MAX_DEPTH = 12
NUTS_MAX_DIM = 8192
NUTS_ROWS = ('q', 'r', 'g', 'edge_q', 'edge_r', 'edge_g', 'cand', 'prop', 'q_out', 'rho_sub',
             'rho_tree', 'ck_r', 'ck_rho')
NUTS_F64 = ('logp', 'eps', 'dt_dir', 'H0', 'href', 'w_sub', 'w_tree', 'acc', 'accept_stat', 'u')
NUTS_I32 = ('j', 'n_sub', 'n_leap', 'v', 'status', 'tree_depth')
NUTS_U8 = ('moved', 'diverging')
NUTS_I64 = ('n_accepted', 'n_divergent')


class NutsArgs(ctypes.Structure):
    """``binf_nuts_args`` of include/binf_hip.h, field for field."""
    _fields_ = [('struct_size', _u64)] + \
        [(n, _vp) for n in NUTS_ROWS + NUTS_F64 + NUTS_I32 + NUTS_U8 + NUTS_I64] + \
        [('max_delta', _f64), ('C', _i64), ('D', _i64), ('max_depth', _i32), ('reserved', _i32)]


def nuts_uniforms_per_chain(max_depth):
    """S: uniforms a chain consumes per transition (directions, merges, one per leaf)."""
    md = int(max_depth)
    return 2 * md + (1 << md) - 1


def nuts_shapes(C, D, max_depth):
    """{field: (shape, dtype)} of every array of ``binf_nuts_args``."""
    md = int(max_depth)
    shapes = {n: ((C, D), torch.float64) for n in NUTS_ROWS}
    for n in ('edge_q', 'edge_r', 'edge_g'):
        shapes[n] = ((2, C, D), torch.float64)
    for n in ('ck_r', 'ck_rho'):
        shapes[n] = ((C, md, D), torch.float64)
    shapes.update({n: ((C,), torch.float64) for n in NUTS_F64})
    shapes['u'] = ((C, nuts_uniforms_per_chain(md)), torch.float64)
    shapes.update({n: ((C,), torch.int32) for n in NUTS_I32})
    shapes.update({n: ((C,), torch.uint8) for n in NUTS_U8})
    shapes.update({n: ((C,), torch.int64) for n in NUTS_I64})
    return shapes


def nuts_args(arrays, C, D, max_depth, max_delta=1000.0):
    """The argument block over ``arrays`` ({field: contiguous device tensor}, every field of
    ``nuts_shapes``); sizes are checked here, the pointers are frozen into the block."""
    a = NutsArgs()
    a.struct_size = ctypes.sizeof(a)
    for name, (shape, dtype) in nuts_shapes(C, D, max_depth).items():
        n = 1
        for s in shape:
            n *= s
        setattr(a, name, dptr(arrays[name], dtype, n, name))
    a.max_delta, a.C, a.D, a.max_depth, a.reserved = float(max_delta), int(C), int(D), int(max_depth), 0
    return a


def nuts_begin(a, device):
    check(lib().binf_nuts_begin_f64(ctypes.byref(a), stream_handle(device)), 'binf_nuts_begin_f64')


def nuts_leaf(a, device):
    check(lib().binf_nuts_leaf_f64(ctypes.byref(a), stream_handle(device)), 'binf_nuts_leaf_f64')


@_launcher
def nuts_pending(status, count):
    """``count[0]`` (int64, device) = chains whose tree is still growing."""
    C = status.numel()
    rc = lib().binf_nuts_pending(dptr(status, torch.int32, C, 'status'), C,
                                 dptr(count, torch.int64, 1, 'count'), stream_handle(status.device))
    check(rc, 'binf_nuts_pending')


@_launcher
def nuts_adapt_step(eps, accept_stat, hbar, logeps, logeps_bar, mu, target, w1, k1, eta, action):
    """binf_nuts_adapt_step_f64: dual averaging of the per-chain steps; ``action`` 0 update,
    1 restart, 2 finalise."""
    C = eps.numel()
    rc = lib().binf_nuts_adapt_step_f64(
        dptr(eps, numel=C, name='eps'), dptr(accept_stat, numel=C, name='accept_stat'),
        dptr(hbar, numel=C, name='hbar'), dptr(logeps, numel=C, name='logeps'),
        dptr(logeps_bar, numel=C, name='logeps_bar'), dptr(mu, numel=C, name='mu'),
        float(target), float(w1), float(k1), float(eta), int(action), C, stream_handle(eps.device))
    check(rc, 'binf_nuts_adapt_step_f64')


# -- ChEES criterion (csrc/chees.hip) ----------------------------------------------------------
CHEES_CHUNK = 64
CHEES_MAX_DIM = 8192


def chees_workspace(C, D, device):
    """The slab ``binf_chees_means_f64`` and ``binf_chees_sums_f64`` share, for ``C x D``."""
    need = lib().binf_chees_workspace_bytes(int(C), int(D))
    if need <= 0:
        raise NotImplementedError('binf_chees_workspace_bytes: %d x %d is not supported' % (C, D))
    return torch.empty(need // 8, dtype=torch.float64, device=device)


@_launcher
def chees_accept_prob(e_before, e_after, alpha):
    """``alpha[c] = min(1, exp(clip(e_before[c] - e_after[c])))``, +0.0 for a diverged chain
    (``binf_chees_accept_prob_f64``)."""
    C = e_before.numel()
    rc = lib().binf_chees_accept_prob_f64(
        dptr(e_before, numel=C, name='e_before'), dptr(e_after, numel=C, name='e_after'),
        dptr(alpha, numel=C, name='alpha'), C, stream_handle(e_before.device))
    check(rc, 'binf_chees_accept_prob_f64')


@_launcher
def chees_means(q, q_prop, alpha, slab, mean_q, mean_prop):
    """Column means over chains of the states and of the effective proposals
    (``binf_chees_means_f64``)."""
    C, D = _cd(q)
    need = lib().binf_chees_workspace_bytes(C, D)
    if slab.numel() * 8 < need:
        raise ValueError('chees_means: slab of %d bytes, %d needed' % (slab.numel() * 8, need))
    rc = lib().binf_chees_means_f64(
        dptr(q, numel=C * D, name='q'), dptr(q_prop, numel=C * D, name='q_prop'),
        dptr(alpha, numel=C, name='alpha'), dptr(slab, name='slab'),
        dptr(mean_q, numel=D, name='mean_q'), dptr(mean_prop, numel=D, name='mean_prop'), C, D,
        stream_handle(q.device))
    check(rc, 'binf_chees_means_f64')


@_launcher
def chees_terms(q, q_prop, v, alpha, mean_q, mean_prop, g):
    """``g[c]``, the chain's term of the ChEES gradient (``binf_chees_terms_f64``)."""
    C, D = _cd(q)
    rc = lib().binf_chees_terms_f64(
        dptr(q, numel=C * D, name='q'), dptr(q_prop, numel=C * D, name='q_prop'),
        dptr(v, numel=C * D, name='v'), dptr(alpha, numel=C, name='alpha'),
        dptr(mean_q, numel=D, name='mean_q'), dptr(mean_prop, numel=D, name='mean_prop'),
        dptr(g, numel=C, name='g'), C, D, stream_handle(q.device))
    check(rc, 'binf_chees_terms_f64')


@_launcher
def chees_sums(alpha, g, slab, out):
    """``out[0..3]``: sum alpha g, sum alpha (finite g), sum 1 / alpha, chains with a non-finite
    g (``binf_chees_sums_f64``)."""
    C = alpha.numel()
    need = lib().binf_chees_workspace_bytes(C, 1)
    if slab.numel() * 8 < need:
        raise ValueError('chees_sums: slab of %d bytes, %d needed' % (slab.numel() * 8, need))
    rc = lib().binf_chees_sums_f64(
        dptr(alpha, numel=C, name='alpha'), dptr(g, numel=C, name='g'), dptr(slab, name='slab'),
        dptr(out, numel=4, name='out'), C, stream_handle(alpha.device))
    check(rc, 'binf_chees_sums_f64')


def linear_resident_supported(K, N):
    """Do the resident linear kernels cover ``K`` coefficients and ``N`` data points?
    (``binf_linear_resident_supported``: the limits live in the library alone.)"""
    return bool(lib().binf_linear_resident_supported(int(K), int(N)))


@_launcher
def hmc_sample_linear(q0, p0, u, q_out, accepted, n_accepted, e_before, e_after,
                      design, ys, precision, prior_means, prior_vars, prior_first,
                      lp_pre, lp_post, timestep, dt_chain, nsteps, adapt, uprate,
                      downrate, mode=MODE_EXACT):
    """binf_hmc_sample_linear_f64 on torch's current stream: one transition of every
    chain on a linear forward model's posterior (``design`` ``[K x N]``)."""
    C, K = _cd(q0)
    N = ys.numel()
    tau, tau_chain = _precision_args(precision, C, q0.device)
    rc = lib().binf_hmc_sample_linear_f64(
        dptr(q0, numel=C * K, name='q0'), dptr(p0, numel=C * K, name='p0'),
        dptr(u, numel=C, name='u'), dptr(q_out, numel=C * K, name='q_out'),
        dptr(accepted, torch.uint8, C, 'accepted'),
        dptr(n_accepted, torch.int64, C, 'n_accepted'),
        dptr(e_before, numel=C, name='e_before'),
        dptr(e_after, numel=C, name='e_after'),
        dptr(design, numel=K * N, name='design'), dptr(ys, numel=N, name='ys'), tau,
        dptr(tau_chain, numel=C, name='precision'),
        dptr(prior_means, numel=K, name='prior_means'),
        dptr(prior_vars, numel=K, name='prior_vars'), int(bool(prior_first)),
        dptr(lp_pre, numel=C, name='lp_pre'), dptr(lp_post, numel=C, name='lp_post'),
        float(timestep), dptr(dt_chain, numel=C, name='dt_chain'), C, K, N,
        int(nsteps), int(bool(adapt)), float(uprate), float(downrate),
        int(mode), stream_handle(q0.device))
    check(rc, 'binf_hmc_sample_linear_f64')


@_launcher
def gibbs_linear_sample_n(coefficients, precision, coefficients_out, precision_out, design, ys,
                          n, thin=1, **kw):
    """binf_gibbs_linear_sample_n_f64 on torch's current stream: n Gibbs sweeps on a
    linear forward model's posterior in one launch (``design`` ``[K x N]``; keywords as
    :func:`gibbs_poly_sample_n`)."""
    K = _cd(coefficients)[1]
    N = ys.numel()
    _gibbs_sample_n('binf_gibbs_linear_sample_n_f64', GibbsLinearArgs(), 'design', design,
                    K * N, N, coefficients, precision, coefficients_out, precision_out, ys, n,
                    thin, **kw)


@_launcher
def jacobian_contract(jacobian, emgrad):
    """``dfm.dot(emgrad)`` of ``Likelihood._evaluate_gradient``, batched:
    ``jacobian`` ``[K x N]`` (shared) or ``[C x K x N]``, ``emgrad`` ``[C x N]`` or
    ``[N]`` (one chain) -> ``[C x K]`` / ``[K]``."""
    one = emgrad.dim() == 1
    r = emgrad.reshape(1, -1) if one else emgrad
    C, N = r.shape
    batched = jacobian.dim() == 3
    K = jacobian.shape[-2]
    if jacobian.shape[-1] != N or (batched and jacobian.shape[0] != C):
        raise ValueError('jacobi matrix %s does not fit the error-model gradient %s'
                         % (tuple(jacobian.shape), tuple(emgrad.shape)))
    out = torch.empty((C, K), dtype=torch.float64, device=r.device)
    rc = lib().binf_jacobian_contract_f64(
        dptr(jacobian, numel=(C if batched else 1) * K * N, name='jacobi matrix'),
        dptr(r, numel=C * N, name='error-model gradient'), dptr(out), C, K, N, int(batched),
        stream_handle(r.device))
    check(rc, 'binf_jacobian_contract_f64')
    return out.reshape(-1) if one else out


@_launcher
def sum_terms(terms, like=None):
    """``((t0 + t1) + t2) + ...`` in one launch (at most 16 terms); a term is a device
    vector (all of one shape), a 0-dim device tensor (ONE device double, broadcast --
    never read back to the host) or a Python / numpy scalar.  ``like``: a tensor of the
    result's shape when no vector is among the terms."""
    tens = [t for t in terms if isinstance(t, torch.Tensor) and t.dim() > 0]
    if not tens and like is None:
        raise TypeError('sum_terms: no device vector among the terms')
    ref = tens[0] if tens else like
    n = ref.numel()
    T = len(terms)
    ptrs = (_vp * T)()
    scal = (_f64 * T)()
    bc = (ctypes.c_uint8 * T)()
    any_bc = False
    for i, t in enumerate(terms):
        if isinstance(t, torch.Tensor) and t.dim() > 0:
            if t.shape != ref.shape:
                raise ValueError('sum_terms: term shapes differ (%s, %s)'
                                 % (tuple(t.shape), tuple(ref.shape)))
            ptrs[i] = dptr(t, numel=n, name='term %d' % i)
        elif isinstance(t, torch.Tensor):
            ptrs[i] = dptr(t, numel=1, name='term %d' % i)
            bc[i] = 1
            any_bc = True
        else:
            ptrs[i] = None
            scal[i] = float(t)
    out = torch.empty_like(ref)
    if any_bc:
        rc = lib().binf_sum_terms_bcast_f64(ptrs, scal, bc, T, dptr(out), n, stream_handle(ref.device))
        check(rc, 'binf_sum_terms_bcast_f64')
    else:
        rc = lib().binf_sum_terms_f64(ptrs, scal, T, dptr(out), n, stream_handle(ref.device))
        check(rc, 'binf_sum_terms_f64')
    return out


_grad_ws = {}


@_launcher
def poly_gauss_grad(coeffs, design, ys, precision):
    C, K = _cd(coeffs)
    N = ys.numel()
    if design.shape != (K, N):
        raise ValueError('design matrix must be [%d x %d], got %s'
                         % (K, N, tuple(design.shape)))
    tau, tau_chain = _precision_args(precision, C, coeffs.device)
    need = lib().binf_poly_gauss_grad_workspace_bytes(C, K, N)
    ws = None
    st = stream_handle(coeffs.device)
    if need > 0:
        # one scratch buffer per (device, stream, size): calls on the same stream
        # are ordered, calls on different streams must not share it
        key = (coeffs.device, st, need)
        ws = _grad_ws.get(key)
        if ws is None:
            ws = torch.empty(need // 8, dtype=torch.float64,
                             device=coeffs.device)
            while len(_grad_ws) >= 4:
                _grad_ws.pop(next(iter(_grad_ws)))
            _grad_ws[key] = ws
    out = torch.empty((C, K), dtype=torch.float64, device=coeffs.device)
    rc = lib().binf_poly_gauss_grad_f64(
        dptr(coeffs, numel=C * K, name='coeffs'),
        dptr(design, numel=K * N, name='design'), dptr(ys, numel=N, name='ys'),
        tau, dptr(tau_chain, numel=C, name='precision'), dptr(out),
        ws.data_ptr() if ws is not None else None, need, C, K, N, st)
    check(rc, 'binf_poly_gauss_grad_f64')
    return out


@_launcher
def poly_leapfrog(q, p, design, ys, precision, timestep, dt_chain, nsteps, mode=MODE_EXACT):
    """binf_poly_leapfrog_f64: the whole ``_leapfrog`` under the polynomial
    likelihood's force, in place on ``q`` and ``p`` (``[C x K]``)."""
    C, K = _cd(q)
    N = ys.numel()
    if design.shape != (K, N):
        raise ValueError('design matrix must be [%d x %d], got %s' % (K, N, tuple(design.shape)))
    tau, tau_chain = _precision_args(precision, C, q.device)
    need = lib().binf_poly_leapfrog_workspace_bytes(C, K, N)
    st = stream_handle(q.device)
    key = (q.device, st, 'leap', need)
    ws = _grad_ws.get(key)
    if ws is None:
        ws = torch.empty(max(1, need // 8), dtype=torch.float64, device=q.device)
        while len(_grad_ws) >= 4:
            _grad_ws.pop(next(iter(_grad_ws)))
        _grad_ws[key] = ws
    rc = lib().binf_poly_leapfrog_f64(
        dptr(q, numel=C * K, name='q'), dptr(p, numel=C * K, name='p'),
        dptr(design, numel=K * N, name='design'), dptr(ys, numel=N, name='ys'), tau,
        dptr(tau_chain, numel=C, name='precision'), ws.data_ptr(), need, C, K, N,
        float(timestep), dptr(dt_chain, numel=C, name='dt_chain'), int(nsteps), int(mode), st)
    check(rc, 'binf_poly_leapfrog_f64')


@_launcher
def linear_forward(coeffs, design):
    """binf_linear_forward_f64: ``coeffs`` [C x K] times ``design`` [K x N] -> [C x N]."""
    C, K = _cd(coeffs)
    if design.dim() != 2 or design.shape[0] != K:
        raise ValueError('design matrix must be [%d x N], got %s' % (K, tuple(design.shape)))
    N = design.shape[1]
    out = torch.empty((C, N), dtype=torch.float64, device=coeffs.device)
    rc = lib().binf_linear_forward_f64(dptr(coeffs, numel=C * K, name='coeffs'),
                                       dptr(design, numel=K * N, name='design'), dptr(out),
                                       C, K, N, stream_handle(coeffs.device))
    check(rc, 'binf_linear_forward_f64')
    return out


@_launcher
def linear_gauss_logp(coeffs, design, ys, precision):
    """binf_linear_gauss_logp_f64: the Gaussian error model's log-prob of
    ``coeffs . design`` against ``ys``, the mock data never written to memory."""
    C, K = _cd(coeffs)
    N = ys.numel()
    if design.shape != (K, N):
        raise ValueError('design matrix must be [%d x %d], got %s' % (K, N, tuple(design.shape)))
    tau, tau_chain = _precision_args(precision, C, coeffs.device)
    need = lib().binf_linear_gauss_logp_workspace_bytes(C, K, N)
    ws = None
    st = stream_handle(coeffs.device)
    if need > 0:
        # one scratch buffer per (device, stream, size), as in poly_gauss_grad
        key = (coeffs.device, st, 'linlp', need)
        ws = _grad_ws.get(key)
        if ws is None:
            ws = torch.empty(need // 8, dtype=torch.float64, device=coeffs.device)
            while len(_grad_ws) >= 4:
                _grad_ws.pop(next(iter(_grad_ws)))
            _grad_ws[key] = ws
    out = torch.empty(C, dtype=torch.float64, device=coeffs.device)
    rc = lib().binf_linear_gauss_logp_f64(
        dptr(coeffs, numel=C * K, name='coeffs'), dptr(design, numel=K * N, name='design'),
        dptr(ys, numel=N, name='ys'), tau, dptr(tau_chain, numel=C, name='precision'), dptr(out),
        ws.data_ptr() if ws is not None else None, need, C, K, N, st)
    check(rc, 'binf_linear_gauss_logp_f64')
    return out


GLM_BINOMIAL_LOGIT, GLM_POISSON_LOG = 0, 1


def _scratch(device, st, tag, need):
    """The scratch buffer of ``need`` bytes kept per (device, stream, tag, size), as in
    poly_gauss_grad; None when none is needed."""
    if need <= 0:
        return None
    key = (device, st, tag, need)
    ws = _grad_ws.get(key)
    if ws is None:
        ws = torch.empty(need // 8, dtype=torch.float64, device=device)
        while len(_grad_ws) >= 4:
            _grad_ws.pop(next(iter(_grad_ws)))
        _grad_ws[key] = ws
    return ws


@_launcher
def glm_pointwise(mock, ys, trials, offset, family, lconst=None, want_ll=True, want_grad=False):
    """binf_glm_pointwise_f64: ``(ll, grad)`` ``[S x N]`` of ``mock`` ``[S x N]`` (None for
    an output that is not wanted); ``lconst`` ``[N]`` is added to each ``ll``."""
    S, N = _cd(mock)
    ll = torch.empty_like(mock) if want_ll else None
    g = torch.empty_like(mock) if want_grad else None
    rc = lib().binf_glm_pointwise_f64(
        dptr(mock, numel=S * N, name='mock'), dptr(ys, numel=N, name='ys'),
        dptr(trials, numel=N, name='trials'), dptr(offset, numel=N, name='offset'),
        dptr(lconst, numel=N, name='lconst'), int(family), dptr(ll), dptr(g), S, N,
        stream_handle(mock.device))
    check(rc, 'binf_glm_pointwise_f64')
    return ll, g


def _glm_shapes(coeffs, design, ys):
    C, K = _cd(coeffs)
    N = ys.numel()
    if design.shape != (K, N):
        raise ValueError('design matrix must be [%d x %d], got %s' % (K, N, tuple(design.shape)))
    return C, K, N


@_launcher
def linear_glm_logp(coeffs, design, ys, trials, offset, family, log_norm):
    """binf_linear_glm_logp_f64: the GLM log-prob of ``coeffs . design``, the mock data
    never written to memory."""
    C, K, N = _glm_shapes(coeffs, design, ys)
    need = lib().binf_linear_glm_logp_workspace_bytes(C, K, N)
    st = stream_handle(coeffs.device)
    ws = _scratch(coeffs.device, st, 'glmlp', need)
    out = torch.empty(C, dtype=torch.float64, device=coeffs.device)
    rc = lib().binf_linear_glm_logp_f64(
        dptr(coeffs, numel=C * K, name='coeffs'), dptr(design, numel=K * N, name='design'),
        dptr(ys, numel=N, name='ys'), dptr(trials, numel=N, name='trials'),
        dptr(offset, numel=N, name='offset'), int(family), float(log_norm), dptr(out),
        ws.data_ptr() if ws is not None else None, need, C, K, N, st)
    check(rc, 'binf_linear_glm_logp_f64')
    return out


@_launcher
def linear_glm_grad(coeffs, design, ys, trials, offset, family):
    """binf_linear_glm_grad_f64: the GLM likelihood's force ``[C x K]``."""
    C, K, N = _glm_shapes(coeffs, design, ys)
    need = lib().binf_linear_glm_grad_workspace_bytes(C, K, N)
    st = stream_handle(coeffs.device)
    ws = _scratch(coeffs.device, st, 'glmgrad', need)
    out = torch.empty((C, K), dtype=torch.float64, device=coeffs.device)
    rc = lib().binf_linear_glm_grad_f64(
        dptr(coeffs, numel=C * K, name='coeffs'), dptr(design, numel=K * N, name='design'),
        dptr(ys, numel=N, name='ys'), dptr(trials, numel=N, name='trials'),
        dptr(offset, numel=N, name='offset'), int(family), dptr(out),
        ws.data_ptr() if ws is not None else None, need, C, K, N, st)
    check(rc, 'binf_linear_glm_grad_f64')
    return out


@_launcher
def linear_glm_leapfrog(q, p, design, ys, trials, offset, family, prior, timestep, dt_chain,
                        nsteps, mode=MODE_EXACT):
    """binf_linear_glm_leapfrog_f64: the whole ``_leapfrog`` under one GLM likelihood's
    force, in place on ``q`` and ``p`` (``[C x K]``); ``prior``: None or ``(k, x0)`` of
    one isotropic Gaussian prior on the same variable."""
    C, K, N = _glm_shapes(q, design, ys)
    need = lib().binf_linear_glm_leapfrog_workspace_bytes(C, K, N)
    st = stream_handle(q.device)
    ws = _scratch(q.device, st, 'glmleap', max(8, need))
    k, x0 = (0.0, 0.0) if prior is None else prior
    rc = lib().binf_linear_glm_leapfrog_f64(
        dptr(q, numel=C * K, name='q'), dptr(p, numel=C * K, name='p'),
        dptr(design, numel=K * N, name='design'), dptr(ys, numel=N, name='ys'),
        dptr(trials, numel=N, name='trials'), dptr(offset, numel=N, name='offset'), int(family),
        int(prior is not None), float(k), float(x0), ws.data_ptr(), need, C, K, N,
        float(timestep), dptr(dt_chain, numel=C, name='dt_chain'), int(nsteps), int(mode), st)
    check(rc, 'binf_linear_glm_leapfrog_f64')


GLM_NEGBIN_LOG = 2
NEGBIN_LAM_MIN, NEGBIN_LAM_MAX = -708.0, 709.0     # the regular range of log_dispersion
NEGBIN_MAX_COUNT = 1 << 20


@_launcher
def negbin_count_term(log_dispersion, tail_counts, log_norm, values=None, want_chain=True):
    """binf_negbin_count_term_f64: ``(log_norm_chain [C], prefix [C x J])`` under
    ``log_dispersion`` ``[C]``; ``tail_counts`` ``[ymax]`` (None: no count above zero),
    ``values`` ``[J]`` the distinct counts ascending (None: no prefix)."""
    C = log_dispersion.numel()
    dev = log_dispersion.device
    ymax = 0 if tail_counts is None else tail_counts.numel()
    J = 0 if values is None else values.numel()
    chain = torch.empty(C, dtype=torch.float64, device=dev) if want_chain else None
    prefix = torch.empty((C, J), dtype=torch.float64, device=dev) if values is not None else None
    rc = lib().binf_negbin_count_term_f64(
        dptr(log_dispersion, numel=C, name='log_dispersion'),
        dptr(tail_counts, numel=ymax, name='tail_counts') if ymax else None, ymax,
        float(log_norm), dptr(chain), dptr(values, numel=J, name='values') if J else None, J,
        dptr(prefix), C, stream_handle(dev))
    check(rc, 'binf_negbin_count_term_f64')
    return chain, prefix


@_launcher
def negbin_pointwise(mock, ys, offset, log_dispersion, prefix=None, prefix_index=None, lconst=None,
                     want_ll=True, want_grad=False):
    """binf_negbin_pointwise_f64: ``(ll, grad)`` ``[S x N]``, row ``s`` of ``mock`` under
    ``log_dispersion[s]``; ``prefix`` ``[S x J]`` with ``prefix_index`` ``[N]`` (int32) and
    ``lconst`` ``[N]`` are added to each ``ll``."""
    S, N = _cd(mock)
    J = 0 if prefix is None else prefix.shape[1]
    if prefix_index is not None and prefix_index.dtype != torch.int32:
        raise TypeError('prefix_index must be int32')
    ll = torch.empty_like(mock) if want_ll else None
    g = torch.empty_like(mock) if want_grad else None
    rc = lib().binf_negbin_pointwise_f64(
        dptr(mock, numel=S * N, name='mock'), dptr(ys, numel=N, name='ys'),
        dptr(offset, numel=N, name='offset'),
        dptr(log_dispersion, numel=S, name='log_dispersion'),
        dptr(prefix, numel=S * J, name='prefix'),
        prefix_index.data_ptr() if prefix_index is not None else None,
        dptr(lconst, numel=N, name='lconst'), dptr(ll), dptr(g), S, N, J,
        stream_handle(mock.device))
    check(rc, 'binf_negbin_pointwise_f64')
    return ll, g


@_launcher
def linear_negbin_logp(coeffs, design, ys, offset, log_dispersion, log_norm_chain):
    """binf_linear_negbin_logp_f64: the fused negative-binomial log-prob ``[C]``."""
    C, K, N = _glm_shapes(coeffs, design, ys)
    need = lib().binf_linear_glm_logp_workspace_bytes(C, K, N)
    st = stream_handle(coeffs.device)
    ws = _scratch(coeffs.device, st, 'glmlp', need)
    out = torch.empty(C, dtype=torch.float64, device=coeffs.device)
    rc = lib().binf_linear_negbin_logp_f64(
        dptr(coeffs, numel=C * K, name='coeffs'), dptr(design, numel=K * N, name='design'),
        dptr(ys, numel=N, name='ys'), dptr(offset, numel=N, name='offset'),
        dptr(log_dispersion, numel=C, name='log_dispersion'),
        dptr(log_norm_chain, numel=C, name='log_norm_chain'), dptr(out),
        ws.data_ptr() if ws is not None else None, need, C, K, N, st)
    check(rc, 'binf_linear_negbin_logp_f64')
    return out


@_launcher
def linear_negbin_grad(coeffs, design, ys, offset, log_dispersion):
    """binf_linear_negbin_grad_f64: the negative-binomial likelihood's force ``[C x K]``."""
    C, K, N = _glm_shapes(coeffs, design, ys)
    need = lib().binf_linear_glm_grad_workspace_bytes(C, K, N)
    st = stream_handle(coeffs.device)
    ws = _scratch(coeffs.device, st, 'glmgrad', need)
    out = torch.empty((C, K), dtype=torch.float64, device=coeffs.device)
    rc = lib().binf_linear_negbin_grad_f64(
        dptr(coeffs, numel=C * K, name='coeffs'), dptr(design, numel=K * N, name='design'),
        dptr(ys, numel=N, name='ys'), dptr(offset, numel=N, name='offset'),
        dptr(log_dispersion, numel=C, name='log_dispersion'), dptr(out),
        ws.data_ptr() if ws is not None else None, need, C, K, N, st)
    check(rc, 'binf_linear_negbin_grad_f64')
    return out


@_launcher
def linear_negbin_leapfrog(q, p, design, ys, offset, log_dispersion, prior, timestep, dt_chain,
                           nsteps, mode=MODE_EXACT):
    """binf_linear_negbin_leapfrog_f64: ``linear_glm_leapfrog`` under the negative-binomial
    likelihood with ``log_dispersion`` ``[C]``."""
    C, K, N = _glm_shapes(q, design, ys)
    need = lib().binf_linear_glm_leapfrog_workspace_bytes(C, K, N)
    st = stream_handle(q.device)
    ws = _scratch(q.device, st, 'glmleap', max(8, need))
    k, x0 = (0.0, 0.0) if prior is None else prior
    rc = lib().binf_linear_negbin_leapfrog_f64(
        dptr(q, numel=C * K, name='q'), dptr(p, numel=C * K, name='p'),
        dptr(design, numel=K * N, name='design'), dptr(ys, numel=N, name='ys'),
        dptr(offset, numel=N, name='offset'),
        dptr(log_dispersion, numel=C, name='log_dispersion'),
        int(prior is not None), float(k), float(x0), ws.data_ptr(), need, C, K, N,
        float(timestep), dptr(dt_chain, numel=C, name='dt_chain'), int(nsteps), int(mode), st)
    check(rc, 'binf_linear_negbin_leapfrog_f64')


@_launcher
def gamma_precision_update(g, lp_unit, prior_rate):
    C = g.numel()
    out = torch.empty(C, dtype=torch.float64, device=g.device)
    rc = lib().binf_gamma_precision_update_f64(
        dptr(g, numel=C, name='g'), dptr(lp_unit, numel=C, name='lp_unit'),
        float(prior_rate), dptr(out), C, stream_handle(g.device))
    check(rc, 'binf_gamma_precision_update_f64')
    return out


@_launcher
def gamma_logp(precision, shape, rate):
    """``(shape - 1) * log(precision) - precision * rate`` per chain
    (priors.py:10-25), one launch."""
    C = precision.numel()
    out = torch.empty(precision.shape, dtype=torch.float64, device=precision.device)
    rc = lib().binf_gamma_logp_f64(dptr(precision, numel=C, name='precision'), float(shape),
                                   float(rate), dptr(out), C, stream_handle(precision.device))
    check(rc, 'binf_gamma_logp_f64')
    return out


@_launcher
def hmc_sample_n_gauss(q0, p0, u, q_out, samples, accepted, n_accepted,
                       e_before, e_after, timestep, dt_chain, nsteps, n, thin,
                       k, x0, n_adapt, uprate, downrate, mode=MODE_EXACT):
    """binf_hmc_sample_n_gauss_f64 on torch's current stream."""
    C, D = _cd(q0)
    n = int(n)
    thin = int(thin)
    nrec = n // thin
    rc = lib().binf_hmc_sample_n_gauss_f64(
        dptr(q0, numel=C * D, name='q0'),
        dptr(p0, numel=n * C * D, name='p0'), dptr(u, numel=n * C, name='u'),
        dptr(q_out, numel=C * D, name='q_out'),
        dptr(samples, numel=nrec * C * D, name='samples'),
        dptr(accepted, torch.uint8, n * C, 'accepted'),
        dptr(n_accepted, torch.int64, C, 'n_accepted'),
        dptr(e_before, numel=n * C, name='e_before'),
        dptr(e_after, numel=n * C, name='e_after'), float(timestep),
        dptr(dt_chain, numel=C, name='dt_chain'), C, D, int(nsteps), n, thin,
        float(k), float(x0), int(n_adapt), float(uprate), float(downrate),
        int(mode), stream_handle(q0.device))
    check(rc, 'binf_hmc_sample_n_gauss_f64')


def gauss_waves_per_chain(C, D):
    """Waves the persistent kernel spreads a chain over for a [C x D] batch."""
    return lib().binf_hmc_gauss_waves_per_chain(int(C), int(D))


def gauss_persist_covers(D):
    """Shapes the persistent kernel (binf_hmc_sample_[n_]gauss_f64) accepts."""
    return 1 <= D <= 8192 and pairwise_tree_height(D) <= 6


@_launcher
def hmc_sample_gauss_big(q0, p0, u, q_out, accepted, n_accepted, e_before, e_after,
                         timestep, dt_chain, nsteps, k, x0, adapt, uprate, downrate,
                         mode=MODE_EXACT):
    """binf_hmc_sample_gauss_big_f64 (chains of any length) on torch's current
    stream; the chunk-sum scratch is allocated here (stream-ordered by torch's
    caching allocator)."""
    C, D = _cd(q0)
    nbytes = lib().binf_hmc_sample_gauss_big_workspace_bytes(C, D)
    ws = torch.empty(max(1, nbytes // 8), dtype=torch.float64, device=q0.device)
    rc = lib().binf_hmc_sample_gauss_big_f64(
        dptr(q0, numel=C * D, name='q0'), dptr(p0, numel=C * D, name='p0'),
        dptr(u, numel=C, name='u'), dptr(q_out, numel=C * D, name='q_out'),
        dptr(accepted, torch.uint8, C, 'accepted'),
        dptr(n_accepted, torch.int64, C, 'n_accepted'),
        dptr(e_before, numel=C, name='e_before'), dptr(e_after, numel=C, name='e_after'),
        float(timestep), dptr(dt_chain, numel=C, name='dt_chain'), C, D, int(nsteps),
        float(k), float(x0), int(bool(adapt)), float(uprate), float(downrate), int(mode),
        dptr(ws), nbytes, stream_handle(q0.device))
    check(rc, 'binf_hmc_sample_gauss_big_f64')


@_launcher
def hmc_sample_gauss_big_rng(q0, q_out, accepted, n_accepted, e_before, e_after, timestep,
                             dt_chain, nsteps, k, x0, adapt, uprate, downrate, mode, seed,
                             offset, chain_offset=0):
    """binf_hmc_sample_gauss_big_rng_f64 (long chains, draws generated in the
    kernels) on torch's current stream."""
    C, D = _cd(q0)
    nbytes = lib().binf_hmc_sample_gauss_big_workspace_bytes(C, D)
    ws = torch.empty(max(1, nbytes // 8), dtype=torch.float64, device=q0.device)
    rc = lib().binf_hmc_sample_gauss_big_rng_f64(
        dptr(q0, numel=C * D, name='q0'), dptr(q_out, numel=C * D, name='q_out'),
        dptr(accepted, torch.uint8, C, 'accepted'),
        dptr(n_accepted, torch.int64, C, 'n_accepted'),
        dptr(e_before, numel=C, name='e_before'), dptr(e_after, numel=C, name='e_after'),
        float(timestep), dptr(dt_chain, numel=C, name='dt_chain'), C, D, int(nsteps),
        float(k), float(x0), int(bool(adapt)), float(uprate), float(downrate), int(mode),
        int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), int(chain_offset), dptr(ws),
        nbytes, stream_handle(q0.device))
    check(rc, 'binf_hmc_sample_gauss_big_rng_f64')


_big_n_ws = {}


@_launcher
def hmc_sample_n_gauss_big(q0, p0, u, q_out, samples, accepted, n_accepted, e_before, e_after,
                           timestep, dt_chain, nsteps, n, thin, k, x0, n_adapt, uprate, downrate,
                           mode=MODE_EXACT, rng=None):
    """binf_hmc_sample_n_gauss_big_f64 (draws supplied: ``p0`` [n, C, D], ``u``
    [n, C]) or, with ``rng = (seed, offset, chain_offset)``, its _rng form."""
    C, D = _cd(q0)
    n, thin = int(n), int(thin)
    nrec = n // thin
    need = lib().binf_hmc_sample_n_gauss_big_workspace_bytes(C, D)
    st = stream_handle(q0.device)
    key = (q0.device, st, need)
    ws = _big_n_ws.get(key)
    if ws is None:
        ws = torch.empty(need // 8, dtype=torch.float64, device=q0.device)
        _big_n_ws.clear()                      # one long-chain scratch at a time
        _big_n_ws[key] = ws
    common = (dptr(samples, numel=nrec * C * D, name='samples'),
              dptr(accepted, torch.uint8, n * C, 'accepted'),
              dptr(n_accepted, torch.int64, C, 'n_accepted'),
              dptr(e_before, numel=n * C, name='e_before'), dptr(e_after, numel=n * C, name='e_after'),
              float(timestep), dptr(dt_chain, numel=C, name='dt_chain'), C, D, int(nsteps), n, thin,
              float(k), float(x0), int(n_adapt), float(uprate), float(downrate), int(mode))
    if rng is None:
        rc = lib().binf_hmc_sample_n_gauss_big_f64(
            dptr(q0, numel=C * D, name='q0'), dptr(p0, numel=n * C * D, name='p0'),
            dptr(u, numel=n * C, name='u'), dptr(q_out, numel=C * D, name='q_out'), *common,
            ws.data_ptr(), need, st)
        check(rc, 'binf_hmc_sample_n_gauss_big_f64')
    else:
        seed, offset, coff = rng
        rc = lib().binf_hmc_sample_n_gauss_big_rng_f64(
            dptr(q0, numel=C * D, name='q0'), dptr(q_out, numel=C * D, name='q_out'), *common,
            int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), int(coff), ws.data_ptr(), need, st)
        check(rc, 'binf_hmc_sample_n_gauss_big_rng_f64')


def hmc_gauss_big_rng_draws(C, D, seed, offset, device, chain_offset=0):
    """(p0 [C, D], u [C]): the draws hmc_sample_gauss_big_rng consumes for global
    chains ``chain_offset .. chain_offset + C - 1``."""
    C, D = int(C), int(D)
    p0 = torch.empty((C, D), dtype=torch.float64, device=device)
    u = torch.empty(C, dtype=torch.float64, device=device)
    with torch.cuda.device(p0.device):
        rc = lib().binf_hmc_gauss_big_rng_draws_f64(
            dptr(p0), dptr(u), C, D, int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1),
            int(chain_offset), stream_handle(p0.device))
    check(rc, 'binf_hmc_gauss_big_rng_draws_f64')
    return p0, u


@_launcher
def hmc_sample_n_gauss_rng(q0, q_out, samples, accepted, n_accepted, e_before,
                           e_after, timestep, dt_chain, nsteps, n, thin, k, x0,
                           n_adapt, uprate, downrate, mode, seed, offset, chain_offset=0):
    """binf_hmc_sample_n_gauss_rng_f64 (draws generated in the kernel) on
    torch's current stream."""
    C, D = _cd(q0)
    n = int(n)
    thin = int(thin)
    nrec = n // thin
    rc = lib().binf_hmc_sample_n_gauss_rng_f64(
        dptr(q0, numel=C * D, name='q0'),
        dptr(q_out, numel=C * D, name='q_out'),
        dptr(samples, numel=nrec * C * D, name='samples'),
        dptr(accepted, torch.uint8, n * C, 'accepted'),
        dptr(n_accepted, torch.int64, C, 'n_accepted'),
        dptr(e_before, numel=n * C, name='e_before'),
        dptr(e_after, numel=n * C, name='e_after'), float(timestep),
        dptr(dt_chain, numel=C, name='dt_chain'), C, D, int(nsteps), n, thin,
        float(k), float(x0), int(n_adapt), float(uprate), float(downrate),
        int(mode), int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1),
        int(chain_offset), stream_handle(q0.device))
    check(rc, 'binf_hmc_sample_n_gauss_rng_f64')


def hmc_gauss_rng_draws(n, C, D, seed, offset, device, chain_offset=0, out=None):
    """(p0 [n, C, D], u [n, C]): the draws the fused-generator kernel consumes
    for (seed, offset) and global chains ``chain_offset .. chain_offset + C - 1``
    (``out = (p0, u)``: fill the caller's buffers instead of new ones)."""
    n, C, D = int(n), int(C), int(D)
    if out is None:
        p0 = torch.empty((n, C, D), dtype=torch.float64, device=device)
        u = torch.empty((n, C), dtype=torch.float64, device=device)
    else:
        p0, u = out
    with torch.cuda.device(p0.device):
        rc = lib().binf_hmc_gauss_rng_draws_f64(
            dptr(p0, numel=n * C * D, name='p0'), dptr(u, numel=n * C, name='u'), C, D, n,
            int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), int(chain_offset),
            stream_handle(p0.device))
    check(rc, 'binf_hmc_gauss_rng_draws_f64')
    return p0, u


@_launcher
def pairdist_forward(x, pair_i, pair_j):
    C, D = _cd(x)
    if D % 3:
        raise ValueError('coordinates must be [n_chains, 3 * n_beads]')
    P = pair_i.numel()
    out = torch.empty((C, P), dtype=torch.float64, device=x.device)
    rc = lib().binf_pairdist_forward_f64(
        dptr(x, numel=C * D, name='x'), dptr(pair_i, torch.int32, P, 'pair_i'),
        dptr(pair_j, torch.int32, P, 'pair_j'), dptr(out), C, D // 3, P,
        stream_handle(x.device))
    check(rc, 'binf_pairdist_forward_f64')
    return out


_chi2_ws = {}


def _pairdist_chi2_workspace(C, n, P, device):
    """(pointer, bytes) of the scratch for chi^2 by chunks (few chains, or more than 2048 beads:
    binf_pairdist_chi2_workspace_bytes), one buffer per device and stream, grown on demand;
    ``(None, 0)`` when the library does not ask for one."""
    need = lib().binf_pairdist_chi2_workspace_bytes(C, n, P)
    if need <= 0:
        return None, 0
    key = (device, stream_handle(device))
    ws = _chi2_ws.get(key)
    if ws is None or ws.numel() * 8 < need:
        ws = _chi2_ws[key] = torch.empty(need // 8, dtype=torch.float64, device=device)
    return ws.data_ptr(), ws.numel() * 8


@_launcher
def pairdist_gauss_logp(x, pair_i, pair_j, ys, precision):
    """Gaussian log-likelihood of the pair distances, fused (no [C x n_pairs]
    intermediate)."""
    C, D = _cd(x)
    if D % 3:
        raise ValueError('coordinates must be [n_chains, 3 * n_beads]')
    P = pair_i.numel()
    tau, tau_chain = _precision_args(precision, C, x.device)
    out = torch.empty(C, dtype=torch.float64, device=x.device)
    rc = lib().binf_pairdist_gauss_logp_f64(
        dptr(x, numel=C * D, name='x'), dptr(pair_i, torch.int32, P, 'pair_i'),
        dptr(pair_j, torch.int32, P, 'pair_j'), dptr(ys, numel=P, name='ys'), tau,
        dptr(tau_chain, numel=C, name='precision'), dptr(out), C, D // 3, P,
        *_pairdist_chi2_workspace(C, D // 3, P, x.device), stream_handle(x.device))
    check(rc, 'binf_pairdist_gauss_logp_f64')
    return out


@_launcher
def pairdist_gauss_logp_memo(x, pair_i, pair_j, ys, precision, memo):
    """binf_pairdist_gauss_logp_memo_f64; ``memo = new_chi2_memo(C, 3 * n_beads, device)``."""
    C, D = _cd(x)
    if D % 3:
        raise ValueError('coordinates must be [n_chains, 3 * n_beads]')
    P = pair_i.numel()
    tau, tau_chain = _precision_args(precision, C, x.device)
    mx, ms, sk = memo
    out = torch.empty(C, dtype=torch.float64, device=x.device)
    rc = lib().binf_pairdist_gauss_logp_memo_f64(
        dptr(x, numel=C * D, name='x'), dptr(pair_i, torch.int32, P, 'pair_i'),
        dptr(pair_j, torch.int32, P, 'pair_j'), dptr(ys, numel=P, name='ys'), tau,
        dptr(tau_chain, numel=C, name='precision'), dptr(out), dptr(mx, numel=2 * C * D, name='memo_x'),
        dptr(ms, numel=2 * C, name='memo_chi2'), dptr(sk, torch.uint8, 2 * C, 'memo_state'), C, D // 3, P,
        *_pairdist_chi2_workspace(C, D // 3, P, x.device), stream_handle(x.device))
    check(rc, 'binf_pairdist_gauss_logp_memo_f64')
    return out


@_launcher
@_launcher
def pairdist_hmc_energy(x, p, pair_i, pair_j, ys, precision, prior, prior_first, memo=None,
                        want_log_prob=False, terms=None):
    """binf_pairdist_hmc_energy_f64: ``0.5 * sum(p**2) - log_prob`` of the restraint
    posterior in one launch.  ``prior`` = ``(k, x0)`` of an isotropic Gaussian or None;
    the components are added in the order ``terms`` gives -- a list of ``'prior'``,
    ``'lik'`` and up to two constants of the move (``[C]`` device tensors or floats) --
    default: prior and likelihood as ``prior_first`` says.  ``memo = new_chi2_memo(C,
    3 * n_beads, device)`` or None.  Returns the energy, or ``(energy, log_prob)``."""
    C, D = _cd(x)
    if D % 3:
        raise ValueError('coordinates must be [n_chains, 3 * n_beads]')
    P = pair_i.numel()
    tau, tau_chain = _precision_args(precision, C, x.device)
    k, x0 = prior if prior is not None else (0.0, 0.0)
    if terms is None:
        terms = ['lik'] if prior is None else (['prior', 'lik'] if prior_first else ['lik', 'prior'])
    kinds, extras = [], []
    for t in terms:
        if isinstance(t, str):
            if t not in ('prior', 'lik') or (t == 'prior' and prior is None):
                raise ValueError('pairdist_hmc_energy: unknown term %r' % (t,))
            kinds.append(0 if t == 'prior' else 1)
        else:
            if len(extras) == 2:
                raise ValueError('pairdist_hmc_energy: at most two constant terms')
            kinds.append(2 + len(extras))
            extras.append(t)
    ptrs, scalars = [None, None], [0.0, 0.0]
    for n_, e in enumerate(extras):
        if isinstance(e, torch.Tensor) and e.dim() > 0:
            ptrs[n_] = dptr(e, numel=C, name='constant term')
        else:
            scalars[n_] = float(e)
    kind_arr = (_i32 * 4)(*(kinds + [1] * (4 - len(kinds))))
    mx, ms, st = memo if memo is not None else (None, None, None)
    energy = torch.empty(C, dtype=torch.float64, device=x.device)
    lp = torch.empty(C, dtype=torch.float64, device=x.device) if want_log_prob else None
    rc = lib().binf_pairdist_hmc_energy_f64(
        dptr(x, numel=C * D, name='x'), dptr(p, numel=C * D, name='p'),
        dptr(pair_i, torch.int32, P, 'pair_i'), dptr(pair_j, torch.int32, P, 'pair_j'),
        dptr(ys, numel=P, name='ys'), tau, dptr(tau_chain, numel=C, name='precision'),
        float(k), float(x0), len(kinds), kind_arr, ptrs[0], scalars[0], ptrs[1], scalars[1],
        dptr(energy), dptr(lp),
        dptr(mx, numel=2 * C * D, name='memo_x'), dptr(ms, numel=2 * C, name='memo_chi2'),
        dptr(st, torch.uint8, 2 * C, 'memo_state'), C, D // 3, P,
        *_pairdist_chi2_workspace(C, D // 3, P, x.device), stream_handle(x.device))
    check(rc, 'binf_pairdist_hmc_energy_f64')
    return (energy, lp) if want_log_prob else energy


@_launcher
def pairdist_pack_targets(ymat):
    """binf_pairdist_pack_targets_f64: the targets in the order the 32..256-bead force
    kernels hold them (pass as ``packed=`` to the two functions below); None for bead
    counts that have no packed form."""
    n = ymat.shape[0]
    nbytes = lib().binf_pairdist_packed_targets_bytes(n)
    if nbytes <= 0:
        return None
    out = torch.empty(nbytes // 8, dtype=torch.float64, device=ymat.device)
    rc = lib().binf_pairdist_pack_targets_f64(dptr(ymat, numel=n * n, name='ymat'), dptr(out), n,
                                              stream_handle(ymat.device))
    check(rc, 'binf_pairdist_pack_targets_f64')
    return out


def _packed_ptr(packed, n):
    if packed is None:
        return None
    return dptr(packed, numel=lib().binf_pairdist_packed_targets_bytes(n) // 8, name='packed')


_tiles_ws = {}


def _pairdist_tiles_workspace(C, n, packed, device):
    """(pointer, bytes) of the scratch for the tiles' partial sums (few chains of 257..1024 beads:
    binf_pairdist_tiles_workspace_bytes), one buffer per device and stream, grown on demand;
    ``(None, 0)`` when the library does not ask for one."""
    if packed is None:
        return None, 0
    need = lib().binf_pairdist_tiles_workspace_bytes(C, n)
    if need <= 0:
        return None, 0
    key = (device, stream_handle(device))
    ws = _tiles_ws.get(key)
    if ws is None or ws.numel() * 8 < need:
        # scratch, not state: never more than a quarter of what is free (many chains of several
        # thousand beads would ask for tens of GB) -- without it the library takes its other kernels
        _tiles_ws.pop(key, None)
        if need > torch.cuda.mem_get_info(device)[0] // 4:
            return None, 0
        ws = _tiles_ws[key] = torch.empty(need // 8, dtype=torch.float64, device=device)
    return ws.data_ptr(), ws.numel() * 8


@_launcher
def pairdist_gauss_grad(x, ymat, precision, packed=None):
    C, D = _cd(x)
    if D % 3:
        raise ValueError('coordinates must be [n_chains, 3 * n_beads]')
    n = D // 3
    tau, tau_chain = _precision_args(precision, C, x.device)
    out = torch.empty_like(x)
    ws, ws_bytes = _pairdist_tiles_workspace(C, n, packed, x.device)
    rc = lib().binf_pairdist_gauss_grad_packed_f64(
        dptr(x, numel=C * D, name='x'), dptr(ymat, numel=n * n, name='ymat'),
        _packed_ptr(packed, n), tau, dptr(tau_chain, numel=C, name='precision'), dptr(out), C, n,
        ws, ws_bytes, stream_handle(x.device))
    check(rc, 'binf_pairdist_gauss_grad_packed_f64')
    return out


@_launcher
def rwmc_propose(state, stepsize, change=None, seed=0, offset=0, chain_offset=0, out=None):
    """``state + uniform(-stepsize, stepsize)`` (samplers.py:81-83); ``change``
    supplied, or drawn on the device from the Philox stream (seed, offset)."""
    C, K = _cd(state)
    if out is None:
        out = torch.empty_like(state)
    rc = lib().binf_rwmc_propose_f64(
        dptr(state, numel=C * K, name='state'), dptr(change, numel=C * K, name='change'),
        dptr(out, numel=C * K, name='proposal'), float(stepsize), C, K,
        int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), int(chain_offset),
        stream_handle(state.device))
    check(rc, 'binf_rwmc_propose_f64')
    return out


@_launcher
def rwmc_accept(proposal, state, lp_old, lp_new, state_out, accepted=None, n_accepted=None,
                u=None, seed=0, offset=0, chain_offset=0):
    """Metropolis test with numpy's exp + select + counters (samplers.py:84-90);
    ``u`` supplied or drawn on the device."""
    C, K = _cd(proposal)
    rc = lib().binf_rwmc_accept_f64(
        dptr(proposal, numel=C * K, name='proposal'), dptr(state, numel=C * K, name='state'),
        dptr(lp_old, numel=C, name='lp_old'), dptr(lp_new, numel=C, name='lp_new'),
        dptr(u, numel=C, name='u'), dptr(state_out, numel=C * K, name='state_out'),
        dptr(accepted, torch.uint8, C, 'accepted'),
        dptr(n_accepted, torch.int64, C, 'n_accepted'), C, K,
        int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), int(chain_offset),
        stream_handle(proposal.device))
    check(rc, 'binf_rwmc_accept_f64')


@_launcher
def replica_gather(x, n_replicas, parity, out=None):
    """``out[c] = x[partner(c)]`` for the swap round of ``parity`` over ladders of
    ``n_replicas`` slots (unpaired chains copy themselves); ``x`` is ``[C x D]``."""
    C, D = _cd(x)
    if out is None:
        out = torch.empty_like(x)
    rc = lib().binf_replica_gather_f64(
        dptr(x, numel=C * D, name='x'), dptr(out, numel=C * D, name='out'), C, D,
        int(n_replicas), int(parity), stream_handle(x.device))
    check(rc, 'binf_replica_gather_f64')
    return out


@_launcher
def replica_swap(x, lp_own, lp_swapped, n_replicas, parity, accepted, u=None, out=None,
                 n_attempted=None, n_accepted=None, walker=None, seed=0, offset=0, chain_offset=0):
    """The exchange test of every pair of the round, the row exchange, flags, counters and
    walker ids in one launch (``binf_replica_swap_f64``); ``u`` supplied (the pair reads its
    lower member's entry) or drawn on the device from the Philox stream (seed, offset)."""
    C, D = _cd(x)
    if out is None:
        out = torch.empty_like(x)
    rc = lib().binf_replica_swap_f64(
        dptr(x, numel=C * D, name='x'), dptr(lp_own, numel=C, name='lp_own'),
        dptr(lp_swapped, numel=C, name='lp_swapped'), dptr(u, numel=C, name='u'),
        dptr(out, numel=C * D, name='out'), dptr(accepted, torch.uint8, C, 'accepted'),
        dptr(n_attempted, torch.int64, C, 'n_attempted'),
        dptr(n_accepted, torch.int64, C, 'n_accepted'), dptr(walker, torch.int64, C, 'walker'),
        C, D, int(n_replicas), int(parity), int(seed) & (2 ** 64 - 1),
        int(offset) & (2 ** 64 - 1), int(chain_offset), stream_handle(x.device))
    check(rc, 'binf_replica_swap_f64')
    return out


@_launcher
def replica_work(lp_own, lp_swapped, n_replicas, parity, out=None):
    """One ``[C]`` row of the work record of a swap round (``binf_replica_work_f64``):
    ``lp_swapped[c] - lp_own[partner(c)]`` for a paired chain, NaN for an unpaired one.
    ``out`` may be a row of a larger record."""
    C = lp_own.numel()
    if out is None:
        out = torch.empty(C, dtype=torch.float64, device=lp_own.device)
    rc = lib().binf_replica_work_f64(
        dptr(lp_own, numel=C, name='lp_own'), dptr(lp_swapped, numel=C, name='lp_swapped'),
        dptr(out, numel=C, name='out'), C, int(n_replicas), int(parity),
        stream_handle(lp_own.device))
    check(rc, 'binf_replica_work_f64')
    return out


FE_OK, FE_INVALID, FE_NO_FINITE, FE_EMPTY, FE_NOT_CONVERGED, FE_ONE_SIDED, FE_NO_OVERLAP = \
    0, 1, 2, 3, 4, 5, 6


def free_energy_chunk():
    """Samples per chunk of the estimator's sums (``binf_free_energy_chunk``)."""
    return int(lib().binf_free_energy_chunk())


@_launcher
def free_energy_bar(work, n_replicas, first_round=0, groups=1):
    """Bennett's acceptance ratio over a ``[T x C]`` work record, a view with unit inner
    stride included (read through its row stride, never copied): a dict of ``[G x (R - 1)]``
    device tensors ``delta, delta_forward, delta_reverse, info, n, n_invalid, status``
    (``binf_free_energy_bar_f64``)."""
    if not isinstance(work, torch.Tensor):
        raise TypeError('work must be a torch.Tensor')
    if not work.is_cuda:
        raise ValueError('work must live in GPU memory (got %s)' % work.device)
    if work.dtype != torch.float64:
        raise ValueError('work must be torch.float64 (got %s)' % work.dtype)
    if work.dim() != 2:
        raise ValueError('work must be [T x C] (got %d dimensions)' % work.dim())
    T, C = (int(s) for s in work.shape)
    st, sc = (int(s) for s in work.stride())
    if C > 1 and sc != 1:
        raise ValueError('work must have unit inner stride (got %d)' % sc)
    if T <= 1:
        st = C                      # never applied; torch reports any value for a size-1 axis
    R, G = int(n_replicas), int(groups)
    dev = work.device
    shape = (max(G, 0), max(R - 1, 0))
    out = {k: torch.empty(shape, dtype=torch.float64, device=dev)
           for k in ('delta', 'delta_forward', 'delta_reverse', 'info')}
    out['n'] = torch.empty(shape, dtype=torch.int64, device=dev)
    out['n_invalid'] = torch.empty(shape, dtype=torch.int64, device=dev)
    out['status'] = torch.empty(shape, dtype=torch.int32, device=dev)
    need = lib().binf_free_energy_bar_workspace_bytes(T, C, R, G)
    ws = torch.empty(max(need // 8, 1), dtype=torch.float64, device=dev)
    P = shape[0] * shape[1]
    # (the record is a view read through its row stride: checked above, not by dptr)
    rc = lib().binf_free_energy_bar_f64(
        work.data_ptr(), st, T, C, R, int(first_round), G,
        dptr(out['delta'], numel=P, name='delta'),
        dptr(out['delta_forward'], numel=P, name='delta_forward'),
        dptr(out['delta_reverse'], numel=P, name='delta_reverse'),
        dptr(out['info'], numel=P, name='info'), dptr(out['n'], torch.int64, P, 'n'),
        dptr(out['n_invalid'], torch.int64, P, 'n_invalid'),
        dptr(out['status'], torch.int32, P, 'status'), dptr(ws, name='workspace'), need,
        stream_handle(dev))
    check(rc, 'binf_free_energy_bar_f64')
    return out


# -- tempered sequential Monte Carlo (csrc/smc.hip) -----------------------------------------
SMC_OK, SMC_FINISHED, SMC_NO_FINITE, SMC_INVALID, SMC_STALLED = 0, 1, 2, 3, 4
SMC_MAX_P = 65536


@_launcher
def smc_temper(ll, beta, beta_chain, ess_fraction=0.5, n_bisect=60):
    """The next temperature of every population and the weights that lead there
    (``binf_smc_temper_f64``): ``ll`` is ``[C]``, ``beta`` ``[G]`` (updated in place),
    ``beta_chain`` ``[C]`` (set to the population's new beta -- the pdf's tensor).  A dict of
    fresh device tensors ``delta, w, log_z_inc, ess, n_invalid, status``."""
    C, G = ll.numel(), beta.numel()
    if G < 1 or C % G != 0:
        raise ValueError('smc_temper: %d chains are no whole number of %d populations' % (C, G))
    dev = ll.device
    out = {k: torch.empty(G, dtype=torch.float64, device=dev) for k in ('delta', 'log_z_inc', 'ess')}
    out['w'] = torch.empty(C, dtype=torch.float64, device=dev)
    out['n_invalid'] = torch.empty(G, dtype=torch.int64, device=dev)
    out['status'] = torch.empty(G, dtype=torch.int32, device=dev)
    rc = lib().binf_smc_temper_f64(
        dptr(ll, numel=C, name='ll'), dptr(beta, numel=G, name='beta'), C, C // G, G,
        float(ess_fraction), int(n_bisect), dptr(out['delta'], numel=G, name='delta'),
        dptr(beta_chain, numel=C, name='beta_chain'), dptr(out['w'], numel=C, name='w'),
        dptr(out['log_z_inc'], numel=G, name='log_z_inc'), dptr(out['ess'], numel=G, name='ess'),
        dptr(out['n_invalid'], torch.int64, G, 'n_invalid'),
        dptr(out['status'], torch.int32, G, 'status'), stream_handle(dev))
    check(rc, 'binf_smc_temper_f64')
    return out


@_launcher
def smc_resample(w, n_populations, u=None, status=None, seed=0, offset=0, chain_offset=0):
    """Systematic resampling of every population (``binf_smc_resample_f64``): ``(ancestor
    [C] int64, n_unique [G] int64)``.  ``u`` ``[G]`` supplied, or drawn in the kernel from
    the Philox stream (seed, offset), keyed by the global index of the population's first
    particle."""
    C, G = w.numel(), int(n_populations)
    if G < 1 or C % G != 0:
        raise ValueError('smc_resample: %d chains are no whole number of %d populations' % (C, G))
    ancestor = torch.empty(C, dtype=torch.int64, device=w.device)
    n_unique = torch.empty(G, dtype=torch.int64, device=w.device)
    rc = lib().binf_smc_resample_f64(
        dptr(w, numel=C, name='w'), dptr(u, numel=G, name='u'),
        dptr(status, torch.int32, G, 'status'), C, C // G, G, int(seed) & (2 ** 64 - 1),
        int(offset) & (2 ** 64 - 1), int(chain_offset),
        dptr(ancestor, torch.int64, C, 'ancestor'), dptr(n_unique, torch.int64, G, 'n_unique'),
        stream_handle(w.device))
    check(rc, 'binf_smc_resample_f64')
    return ancestor, n_unique


@_launcher
def smc_gather(x, ancestor, side=None, out=None, side_out=None):
    """``out[c] = x[ancestor[c]]`` for ``x`` ``[C x D]`` and, alike, the rows of ``side``
    (``[K x C]``, K <= 4) (``binf_smc_gather_f64``); returns ``(out, side_out)``, fresh
    tensors unless given."""
    C, D = _cd(x)
    K = 0
    if side is not None:
        if side.dim() != 2 or side.shape[1] != C:
            raise ValueError('smc_gather: side must be [K x %d] (got %s)' % (C, tuple(side.shape)))
        K = int(side.shape[0])
        if side_out is None:
            side_out = torch.empty_like(side)
    if out is None:
        out = torch.empty_like(x)
    rc = lib().binf_smc_gather_f64(
        dptr(x, numel=C * D, name='x'), dptr(ancestor, torch.int64, C, 'ancestor'),
        dptr(out, numel=C * D, name='out'), dptr(side, numel=K * C, name='side'),
        dptr(side_out if K else None, numel=K * C, name='side_out'), K, C, D,
        stream_handle(x.device))
    check(rc, 'binf_smc_gather_f64')
    return out, (side_out if K else None)


def _draws_layout(draws):
    """(pointer, stride_t, stride_c, stride_i, T, C, D) of a ``[T x C x D]`` fp64 device tensor,
    a view included: it is read through its strides, never copied."""
    if not isinstance(draws, torch.Tensor):
        raise TypeError('draws must be a torch.Tensor')
    if not draws.is_cuda:
        raise ValueError('draws must live in GPU memory (got %s)' % draws.device)
    if draws.dtype != torch.float64:
        raise ValueError('draws must be torch.float64 (got %s)' % draws.dtype)
    if draws.dim() != 3:
        raise ValueError('draws must be [T x C x D] (got %d dimensions)' % draws.dim())
    T, C, D = (int(s) for s in draws.shape)
    st, sc, si = (int(s) for s in draws.stride())
    if D == 1:
        si = 1                      # never applied; torch reports any value for a size-1 axis
    return draws.data_ptr(), st, sc, si, T, C, D


@_launcher
def chain_moments(draws, split=1):
    """``(mean, m2)``, each ``[split * C x D]``, of every split chain and dimension in one
    pass over ``draws`` (``binf_chain_moments_f64``); split chain ``m = s * C + c``."""
    p, st, sc, si, T, C, D = _draws_layout(draws)
    M = int(split) * C if int(split) in (1, 2) else C
    mean = torch.empty((M, D), dtype=torch.float64, device=draws.device)
    m2 = torch.empty_like(mean)
    rc = lib().binf_chain_moments_f64(p, st, sc, si, T, C, D, int(split), mean.data_ptr(),
                                      m2.data_ptr(), stream_handle(draws.device))
    check(rc, 'binf_chain_moments_f64')
    return mean, m2


@_launcher
def chain_autocov(draws, mean, split, max_lag):
    """``[ceil(M / 64) x (max_lag + 1) x D]`` block sums over the split chains of the lagged
    autocovariances around ``mean`` (``binf_chain_autocov_f64``)."""
    p, st, sc, si, T, C, D = _draws_layout(draws)
    M, K = int(split) * C, int(max_lag)
    part = torch.empty(((M + 63) // 64, max(K, 0) + 1, D), dtype=torch.float64, device=draws.device)
    rc = lib().binf_chain_autocov_f64(p, st, sc, si, T, C, D, int(split),
                                      dptr(mean, numel=M * D, name='mean'), K, part.data_ptr(),
                                      part.numel() * 8, stream_handle(draws.device))
    check(rc, 'binf_chain_autocov_f64')
    return part


@_launcher
def diag_summary(mean, m2, autocov, n):
    """The across-chain step (``binf_diag_summary_f64``): a dict of ``[D]`` tensors
    ``post_mean, varplus, sd, W, rhat`` and, with ``autocov`` (the result of
    :func:`chain_autocov`), ``ess, mcse, truncated`` (uint8)."""
    M, D = _cd(mean)
    dev = mean.device
    K = int(autocov.shape[1]) - 1 if autocov is not None else 0
    out = {k: torch.empty(D, dtype=torch.float64, device=dev)
           for k in ('post_mean', 'varplus', 'sd', 'W', 'rhat')}
    if autocov is not None:
        out['ess'] = torch.empty(D, dtype=torch.float64, device=dev)
        out['mcse'] = torch.empty(D, dtype=torch.float64, device=dev)
        out['truncated'] = torch.empty(D, dtype=torch.uint8, device=dev)
    need = lib().binf_diag_summary_workspace_bytes(M, D)
    ws = torch.empty(max(need // 8, 1), dtype=torch.float64, device=dev)
    rc = lib().binf_diag_summary_f64(
        dptr(mean, numel=M * D, name='mean'), dptr(m2, numel=M * D, name='m2'),
        dptr(autocov, numel=((M + 63) // 64) * (K + 1) * D, name='autocov'), int(n), M, D, K,
        out['post_mean'].data_ptr(), out['varplus'].data_ptr(), out['sd'].data_ptr(),
        out['W'].data_ptr(), out['rhat'].data_ptr(),
        out['ess'].data_ptr() if autocov is not None else None,
        out['mcse'].data_ptr() if autocov is not None else None,
        out['truncated'].data_ptr() if autocov is not None else None,
        ws.data_ptr(), need, stream_handle(dev))
    check(rc, 'binf_diag_summary_f64')
    return out


DRAWS_MAP_FOLD, DRAWS_MAP_LE = 0, 1


def _pooled(draws, split):
    """(split * n, C, D): the shape of the split record of ``draws``."""
    T, C, D = (int(s) for s in draws.shape)
    s = int(split)
    return (s * (T // s) if s in (1, 2) else T), C, D


@_launcher
def rank_normalise(draws, split, ztab=None, want_sorted=False, z=None, sorted_out=None):
    """``(sorted, z)`` of ``binf_rank_normalise_f64``: ``sorted [D x S]`` (``want_sorted`` or a
    buffer ``sorted_out``) and ``z [split * n x C x D]`` (``ztab`` given; into ``z`` if supplied);
    what was not asked for is ``None``."""
    p, st, sc, si, T, C, D = _draws_layout(draws)
    Tp, _, _ = _pooled(draws, split)
    S = Tp * C
    dev = draws.device
    need = lib().binf_rank_sort_workspace_bytes(S, D)
    if need == 0:                   # a record the library refuses: let it say why, allocate nothing
        check(lib().binf_rank_normalise_f64(p, st, sc, si, T, C, D, int(split), None, None, None, None, 0,
                                            stream_handle(dev)), 'binf_rank_normalise_f64')
    if ztab is not None and z is None:
        z = torch.empty((Tp, C, D), dtype=torch.float64, device=dev)
    if want_sorted and sorted_out is None:
        sorted_out = torch.empty((D, S), dtype=torch.float64, device=dev)
    ws = torch.empty(max(need // 8, 1), dtype=torch.float64, device=dev)
    rc = lib().binf_rank_normalise_f64(
        p, st, sc, si, T, C, D, int(split), dptr(ztab, numel=2 * S + 1, name='ztab'),
        dptr(sorted_out, numel=D * S, name='sorted'), dptr(z, numel=S * D, name='z'),
        ws.data_ptr(), need, stream_handle(dev))
    check(rc, 'binf_rank_normalise_f64')
    return sorted_out, z


@_launcher
def sorted_quantiles(sorted_values, probs):
    """``[Q x D]`` quantiles (numpy's linear method) of ``sorted_values [D x S]``
    (``binf_sorted_quantiles_f64``); ``probs``: host numbers in [0, 1], 16 at the most."""
    D, S = _cd(sorted_values)
    probs = [float(q) for q in probs]
    Q = len(probs)
    out = torch.empty((Q, D), dtype=torch.float64, device=sorted_values.device)
    rc = lib().binf_sorted_quantiles_f64(
        dptr(sorted_values, numel=D * S, name='sorted'), S, D, (ctypes.c_double * max(Q, 1))(*probs), Q,
        out.data_ptr(), stream_handle(sorted_values.device))
    check(rc, 'binf_sorted_quantiles_f64')
    return out


@_launcher
def draws_map(draws, split, op, param, out=None):
    """``[split * n x C x D]``: ``|x - param[i]|`` (``DRAWS_MAP_FOLD``) or ``x <= param[i]`` as
    1.0 / 0.0 (``DRAWS_MAP_LE``) of the split record (``binf_draws_map_f64``)."""
    p, st, sc, si, T, C, D = _draws_layout(draws)
    Tp, _, _ = _pooled(draws, split)
    if out is None:
        out = torch.empty((Tp, C, D), dtype=torch.float64, device=draws.device)
    rc = lib().binf_draws_map_f64(p, st, sc, si, T, C, D, int(split), int(op),
                                  dptr(param, numel=D, name='param'),
                                  dptr(out, numel=Tp * C * D, name='out'), stream_handle(draws.device))
    check(rc, 'binf_draws_map_f64')
    return out


@_launcher
def rank_diag_combine(rhat_bulk, rhat_folded, ess_lo, ess_hi, trunc_mean, trunc_bulk, trunc_lo, trunc_hi):
    """``(rhat, ess_tail, truncated)``: the larger R^, the smaller tail ESS (NaN if either is)
    and the OR of the four flags, on the device (``binf_rank_diag_combine_f64``)."""
    D = int(rhat_bulk.numel())
    dev = rhat_bulk.device
    rhat = torch.empty(D, dtype=torch.float64, device=dev)
    ess_tail = torch.empty(D, dtype=torch.float64, device=dev)
    truncated = torch.empty(D, dtype=torch.uint8, device=dev)
    f64 = lambda t, name: dptr(t, numel=D, name=name)
    u8 = lambda t, name: dptr(t, torch.uint8, D, name)
    rc = lib().binf_rank_diag_combine_f64(
        f64(rhat_bulk, 'rhat_bulk'), f64(rhat_folded, 'rhat_folded'), f64(ess_lo, 'ess_lo'),
        f64(ess_hi, 'ess_hi'), u8(trunc_mean, 'trunc_mean'), u8(trunc_bulk, 'trunc_bulk'),
        u8(trunc_lo, 'trunc_lo'), u8(trunc_hi, 'trunc_hi'), D, rhat.data_ptr(), ess_tail.data_ptr(),
        truncated.data_ptr(), stream_handle(dev))
    check(rc, 'binf_rank_diag_combine_f64')
    return rhat, ess_tail, truncated


@_launcher
def gauss_pointwise_loglik(mock, precision, ys, half_log_2pi):
    """binf_gauss_pointwise_loglik_f64: ``mock`` [S x N], ``precision`` [S], ``ys`` [N] -> the
    pointwise log-likelihood record [S x N] of the Gaussian error model."""
    S, N = _cd(mock)
    out = torch.empty((S, N), dtype=torch.float64, device=mock.device)
    rc = lib().binf_gauss_pointwise_loglik_f64(dptr(mock, numel=S * N, name='mock'),
                                               dptr(precision, numel=S, name='precision'),
                                               dptr(ys, numel=N, name='ys'), dptr(out), S, N,
                                               float(half_log_2pi), stream_handle(mock.device))
    check(rc, 'binf_gauss_pointwise_loglik_f64')
    return out


@_launcher
def psis_loo(sorted_ll):
    """binf_psis_loo_f64 of ``sorted_ll [N x S]`` (per observation its log-likelihoods ascending,
    the ``sorted`` of :func:`rank_normalise`): a dict of ``[N]`` device tensors ``elpd_loo, khat,
    n_eff, lppd, p_waic`` (fp64) and ``tail_len`` (int32)."""
    N, S = _cd(sorted_ll)
    dev = sorted_ll.device
    out = {k: torch.empty(N, dtype=torch.float64, device=dev)
           for k in ('elpd_loo', 'khat', 'n_eff', 'lppd', 'p_waic')}
    out['tail_len'] = torch.empty(N, dtype=torch.int32, device=dev)
    need = lib().binf_psis_loo_workspace_bytes(S, N)
    ws = torch.empty(max(need // 8, 1), dtype=torch.float64, device=dev)
    rc = lib().binf_psis_loo_f64(
        dptr(sorted_ll, numel=N * S, name='sorted_ll'), S, N, out['elpd_loo'].data_ptr(),
        out['khat'].data_ptr(), out['n_eff'].data_ptr(), out['lppd'].data_ptr(),
        out['p_waic'].data_ptr(), out['tail_len'].data_ptr(), ws.data_ptr(), need, stream_handle(dev))
    check(rc, 'binf_psis_loo_f64')
    return out


@_launcher
def pointwise_totals(x, y=None, khat=None, threshold=0.7):
    """binf_pointwise_totals_f64 of the rows of ``x [R x N]`` (of ``x - y`` with ``y``): a device
    tensor of ``2 R`` doubles, row r's sum and its sum of squared deviations from its mean; with
    ``khat [N]`` one more, the number of ``khat > threshold``."""
    R, N = _cd(x)
    out = torch.empty(2 * R + (1 if khat is not None else 0), dtype=torch.float64, device=x.device)
    rc = lib().binf_pointwise_totals_f64(dptr(x, numel=R * N, name='x'), dptr(y, numel=R * N, name='y'),
                                         R, N, dptr(khat, numel=N, name='khat'), float(threshold),
                                         out.data_ptr(), stream_handle(x.device))
    check(rc, 'binf_pointwise_totals_f64')
    return out


def philox4x32_10(counter, key):
    c = (ctypes.c_uint32 * 4)(*[int(x) & 0xffffffff for x in counter])
    k = (ctypes.c_uint32 * 2)(*[int(x) & 0xffffffff for x in key])
    o = (ctypes.c_uint32 * 4)()
    check(lib().binf_rng_philox4x32_10(c, k, o), 'binf_rng_philox4x32_10')
    return [int(x) for x in o]


@_launcher
def rng_fill(kind, out, seed, offset, shape=None, elem_offset=0):
    """Fill the contiguous f64 device tensor `out` with uniform / normal /
    gamma(shape) draws of the Philox stream (seed, offset); ``out[l]`` receives
    global element ``elem_offset + l`` of the stream."""
    n = out.numel()
    p = dptr(out, numel=n, name='out')
    st = stream_handle(out.device)
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    e0 = int(elem_offset)
    if kind == 'uniform':
        rc = lib().binf_rng_uniform_f64(p, n, seed, offset, e0, st)
    elif kind == 'normal':
        rc = lib().binf_rng_normal_f64(p, n, seed, offset, e0, st)
    elif kind == 'normal_zig':
        rc = lib().binf_rng_normal_zig_f64(p, n, seed, offset, e0, st)
    elif kind == 'gamma':
        rc = lib().binf_rng_gamma_f64(p, n, float(shape), seed, offset, e0, st)
    else:
        raise ValueError('unknown draw kind %r' % (kind,))
    check(rc, 'binf_rng_%s_f64' % kind)
    return out


@_launcher
def rng_fill_normal_zig_uniform(normals, uniforms, seed, offset_normals, offset_uniforms,
                                elem_offset_normals=0, elem_offset_uniforms=0):
    """binf_rng_normal_zig_uniform_f64: ``rng_fill('normal_zig', normals, ...)`` and
    ``rng_fill('uniform', uniforms, ...)`` in one launch."""
    m = 2 ** 64 - 1
    rc = lib().binf_rng_normal_zig_uniform_f64(
        dptr(normals, numel=normals.numel(), name='normals'), normals.numel(),
        dptr(uniforms, numel=uniforms.numel(), name='uniforms'), uniforms.numel(),
        int(seed) & m, int(offset_normals) & m, int(offset_uniforms) & m,
        int(elem_offset_normals), int(elem_offset_uniforms), stream_handle(normals.device))
    check(rc, 'binf_rng_normal_zig_uniform_f64')


@_launcher
def pairdist_leapfrog(q, p, ymat, precision, prior, prior_first, timestep,
                      dt_chain, nsteps, mode=MODE_EXACT, packed=None, q_from=None):
    """In-place leapfrog of (q, p) for the restraint posterior; prior is None
    or (k, x0) of an isotropic Gaussian on the coordinates.  ``q_from``: start positions
    read from there instead of ``q`` (which then only receives the end positions)."""
    C, D = _cd(q)
    if D % 3:
        raise ValueError('coordinates must be [n_chains, 3 * n_beads]')
    n = D // 3
    tau, tau_chain = _precision_args(precision, C, q.device)
    k, x0 = prior if prior is not None else (0.0, 0.0)
    ws, ws_bytes = _pairdist_tiles_workspace(C, n, packed, q.device)
    rc = lib().binf_pairdist_leapfrog_packed_f64(
        dptr(q, numel=C * D, name='q'), dptr(q_from, numel=C * D, name='q_from'),
        dptr(p, numel=C * D, name='p'),
        dptr(ymat, numel=n * n, name='ymat'), _packed_ptr(packed, n), tau,
        dptr(tau_chain, numel=C, name='precision'), int(prior is not None),
        float(k), float(x0), int(bool(prior_first)), float(timestep),
        dptr(dt_chain, numel=C, name='dt_chain'), int(nsteps), C, n, int(mode),
        ws, ws_bytes, stream_handle(q.device))
    check(rc, 'binf_pairdist_leapfrog_packed_f64')
