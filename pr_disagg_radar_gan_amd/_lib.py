"""ctypes binding of librdgan_hip.so (C ABI: include/rdgan.h).

The product path has NO CPU fallback: if the library is missing or no MI355X is visible,
every compute entry point raises.  (The CPU oracle lives in /oracle and is test-only.)
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librdgan_hip.so")

c_f32p = ctypes.c_void_p      # device pointers travel as integers
c_stream = ctypes.c_void_p

# every symbol include/rdgan.h declares: name -> (restype, argtypes)
class LaunchStat(ctypes.Structure):
    """rdgan_launch_stat (include/rdgan.h)"""
    _fields_ = [("plan", ctypes.c_int), ("kind", ctypes.c_int), ("batch", ctypes.c_int), ("launches", ctypes.c_int),
                ("gflop", ctypes.c_double), ("ms", ctypes.c_double), ("name", ctypes.c_char * 48), ("kernel", ctypes.c_char * 48)]


SIGNATURES = {
    "rdgan_create": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "rdgan_destroy": (None, [ctypes.c_void_p]),
    "rdgan_last_error": (ctypes.c_char_p, [ctypes.c_void_p]),
    "rdgan_gen_param_count": (ctypes.c_long, [ctypes.c_void_p]),
    "rdgan_critic_param_count": (ctypes.c_long, [ctypes.c_void_p]),
    "rdgan_workspace_bytes": (ctypes.c_long, [ctypes.c_void_p]),
    "rdgan_gen_forward": (ctypes.c_int, [ctypes.c_void_p, c_f32p, c_f32p, c_f32p, c_f32p, ctypes.c_int, c_stream]),
    "rdgan_check_numerics": (ctypes.c_int, [ctypes.c_void_p, c_stream]),
    "rdgan_critic_forward": (ctypes.c_int, [ctypes.c_void_p, c_f32p, c_f32p, c_f32p, c_f32p, ctypes.c_int,
                                            ctypes.c_uint64, c_stream]),
    "rdgan_critic_grad": (ctypes.c_int, [ctypes.c_void_p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, ctypes.c_uint64,
                                         c_f32p, ctypes.c_int, c_stream]),
    "rdgan_gen_grad": (ctypes.c_int, [ctypes.c_void_p, c_f32p, c_f32p, c_f32p, c_f32p, ctypes.c_uint64, c_f32p,
                                      ctypes.c_int, c_stream]),
    "rdgan_critic_grad_after": (ctypes.c_int, [ctypes.c_void_p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, ctypes.c_uint64,
                                               c_f32p, ctypes.c_int, ctypes.c_void_p, c_stream]),
    "rdgan_critic_grad_ahead": (ctypes.c_int, [ctypes.c_void_p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, ctypes.c_uint64,
                                               c_f32p, ctypes.c_int, ctypes.c_void_p, c_f32p, c_f32p, ctypes.c_int, c_stream]),
    "rdgan_gen_grad_after": (ctypes.c_int, [ctypes.c_void_p, c_f32p, c_f32p, c_f32p, c_f32p, ctypes.c_uint64, c_f32p,
                                            ctypes.c_int, ctypes.c_void_p, c_stream]),
    "rdgan_adam": (ctypes.c_int, [c_f32p, c_f32p, c_f32p, ctypes.c_long, ctypes.c_int, ctypes.c_float, ctypes.c_float,
                                  ctypes.c_float, ctypes.c_float, c_stream]),
    "rdgan_set_weight_versions": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64]),
    "rdgan_form_builds": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_long), ctypes.POINTER(ctypes.c_long)]),
    "rdgan_gen_param_layout": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_long), ctypes.POINTER(ctypes.c_long)]),
    "rdgan_critic_param_layout": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_long), ctypes.POINTER(ctypes.c_long)]),
    "rdgan_set_option": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]),
    "rdgan_profile": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint]),
    "rdgan_flop_count": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_int]),
    "rdgan_profile_read": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double),
                                          ctypes.POINTER(ctypes.c_long)]),
    "rdgan_profile_launches": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "rdgan_launch_table": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(LaunchStat), ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
    "rdgan_data_gather": (ctypes.c_int, [c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                         ctypes.c_int, ctypes.c_float, c_f32p, c_f32p, ctypes.c_void_p, c_stream]),
    "rdgan_data_valid_tiles": (ctypes.c_int, [c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_float, ctypes.c_int, ctypes.c_void_p, c_stream]),
    "rdgan_data_radar_hourly": (ctypes.c_int, [ctypes.c_void_p, c_f32p, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                               c_f32p, c_f32p, ctypes.c_void_p, c_stream]),
    "rdgan_data_daily_sum": (ctypes.c_int, [c_f32p, ctypes.c_long, ctypes.c_int, ctypes.c_int, c_f32p, c_stream]),
    "rdgan_data_valid_tiles_daily": (ctypes.c_int, [c_f32p, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                    ctypes.c_float, ctypes.c_int, ctypes.c_void_p, c_stream]),
    "rdgan_crps_ensemble": (ctypes.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, ctypes.c_int, ctypes.c_long, c_stream]),
    "rdgan_crps_fixed_ensemble": (ctypes.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, ctypes.c_int, ctypes.c_long, ctypes.c_int,
                                                 c_stream]),
    "rdgan_bootstrap_means": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_uint64, ctypes.c_long, ctypes.c_long,
                                             ctypes.c_void_p, c_stream]),
    "rdgan_moments_f64": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, c_stream]),
    "rdgan_ks_2samp": (ctypes.c_int, [c_f32p, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_long, ctypes.c_void_p,
                                      ctypes.c_void_p, c_stream]),
    "rdgan_box_stats": (ctypes.c_int, [c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_long, ctypes.c_void_p, c_f32p, c_stream]),
    "rdgan_ecdf_workspace_bytes": (ctypes.c_long, [ctypes.c_int]),
    "rdgan_ecdf_grid": (ctypes.c_int, [c_f32p, ctypes.c_long, c_f32p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long,
                                       c_stream]),
    "rdgan_field_scan": (ctypes.c_int, [c_f32p, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                        c_stream]),
    "rdgan_field_cond": (ctypes.c_int, [c_f32p, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                        ctypes.c_long, ctypes.c_double, c_f32p, c_stream]),
    "rdgan_field_blend": (ctypes.c_int, [c_f32p, ctypes.c_long, ctypes.c_void_p, ctypes.c_long, ctypes.c_long, ctypes.c_void_p, c_f32p,
                                         ctypes.c_void_p, c_f32p, c_f32p, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_int, c_f32p, c_stream]),
    "rdgan_hourly_peaks": (ctypes.c_int, [c_f32p, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, c_f32p,
                                          ctypes.c_void_p, c_stream]),
    "rdgan_field_blend_peaks": (ctypes.c_int, [c_f32p, ctypes.c_long, ctypes.c_void_p, ctypes.c_long, ctypes.c_long, ctypes.c_void_p,
                                               c_f32p, ctypes.c_void_p, c_f32p, c_f32p, ctypes.c_long, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, c_f32p, ctypes.c_void_p,
                                               c_stream]),
    "rdgan_member_stats": (ctypes.c_int, [c_f32p, ctypes.c_int, ctypes.c_long, ctypes.c_long, ctypes.c_void_p, ctypes.c_int,
                                          ctypes.c_void_p, ctypes.c_int, c_f32p, c_f32p, c_f32p, ctypes.c_void_p, c_stream]),
    "rdgan_verify_accumulate": (ctypes.c_int, [c_f32p, ctypes.c_int, ctypes.c_long, ctypes.c_long, c_f32p, ctypes.c_void_p, ctypes.c_int,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_stream]),
    "rdgan_verify_reduce": (ctypes.c_int, [c_f32p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long,
                                           ctypes.c_long, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_uint64,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_stream]),
    "rdgan_verify_fss_workspace_bytes": (ctypes.c_long, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "rdgan_verify_fss": (ctypes.c_int, [c_f32p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_long, c_stream]),
    "rdgan_temporal_workspace_bytes": (ctypes.c_long, [ctypes.c_long, ctypes.c_long, ctypes.c_int, ctypes.c_int]),
    "rdgan_temporal_accumulate": (ctypes.c_int, [c_f32p, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_void_p, ctypes.c_int,
                                                 ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long,
                                                 c_stream]),
    "rdgan_cells_workspace_bytes": (ctypes.c_long, [ctypes.c_long, ctypes.c_long, ctypes.c_long]),
    "rdgan_cells_accumulate": (ctypes.c_int, [c_f32p, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_void_p,
                                              ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                              ctypes.c_void_p, ctypes.c_long, c_stream]),
    "rdgan_sal_workspace_bytes": (ctypes.c_long, [ctypes.c_long, ctypes.c_long, ctypes.c_long]),
    "rdgan_sal_records": (ctypes.c_int, [c_f32p, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_void_p,
                                         ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_long, c_stream]),
    "rdgan_iss_workspace_bytes": (ctypes.c_long, [ctypes.c_long, ctypes.c_long, ctypes.c_int, ctypes.c_long]),
    "rdgan_iss_accumulate": (ctypes.c_int, [c_f32p, ctypes.c_int, ctypes.c_long, c_f32p, ctypes.c_long, ctypes.c_long, ctypes.c_long,
                                            ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_long, c_stream]),
    "rdgan_dm_workspace_bytes": (ctypes.c_long, [ctypes.c_long, ctypes.c_long, ctypes.c_long]),
    "rdgan_dm_maps": (ctypes.c_int, [c_f32p, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_void_p, ctypes.c_int,
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, c_stream]),
    "rdgan_dm_records": (ctypes.c_int, [c_f32p, ctypes.c_int, ctypes.c_long, c_f32p, ctypes.c_void_p, ctypes.c_long, ctypes.c_long,
                                        ctypes.c_long, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_long, c_stream]),
    "rdgan_storms_state_count": (ctypes.c_long, [ctypes.c_int]),
    "rdgan_storms_workspace_bytes": (ctypes.c_long, [ctypes.c_long, ctypes.c_long, ctypes.c_long]),
    "rdgan_storms_accumulate": (ctypes.c_int, [c_f32p, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_void_p,
                                               ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                               ctypes.c_void_p, ctypes.c_long, c_stream]),
    "rdgan_areal_state_count": (ctypes.c_long, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "rdgan_areal_workspace_bytes": (ctypes.c_long, [ctypes.c_long, ctypes.c_long, ctypes.c_long]),
    "rdgan_areal_accumulate": (ctypes.c_int, [c_f32p, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_void_p,
                                              ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, c_stream]),
    "rdgan_scaling_state_count": (ctypes.c_long, [ctypes.c_int]),
    "rdgan_scaling_workspace_bytes": (ctypes.c_long, [ctypes.c_long, ctypes.c_long, ctypes.c_int]),
    "rdgan_scaling_accumulate": (ctypes.c_int, [c_f32p, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_int,
                                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, c_stream]),
    "rdgan_catchment_state_count": (ctypes.c_long, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "rdgan_catchment_workspace_bytes": (ctypes.c_long, [ctypes.c_int, ctypes.c_long]),
    "rdgan_catchment_accumulate": (ctypes.c_int, [c_f32p, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_void_p,
                                                  ctypes.c_long, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_int,
                                                  ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, c_stream]),
    "rdgan_spacetime_state_count":(ctypes.c_long, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "rdgan_spacetime_workspace_bytes": (ctypes.c_long, [ctypes.c_long, ctypes.c_long, ctypes.c_int, ctypes.c_long]),
    "rdgan_spacetime_accumulate": (ctypes.c_int, [c_f32p, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_void_p,
                                                  ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long,
                                                  c_stream]),
    "rdgan_analog_workspace_bytes": (ctypes.c_long, [ctypes.c_long, ctypes.c_int, ctypes.c_long]),
    "rdgan_analog_features": (ctypes.c_int, [c_f32p, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_int, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_stream]),
    "rdgan_analog_search": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_long, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, c_stream]),
    "rdgan_analog_apply": (ctypes.c_int, [c_f32p, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_long, c_f32p, ctypes.c_long,
                                          ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_long,
                                          ctypes.c_uint64, ctypes.c_int, c_f32p, ctypes.c_void_p, c_stream]),
    "rdgan_seq_workspace_bytes": (ctypes.c_long, [ctypes.c_long, ctypes.c_long]),
    "rdgan_seq_edges": (ctypes.c_int, [c_f32p, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_int,
                                       ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, c_stream]),
    "rdgan_seq_costs": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long,
                                       ctypes.c_long, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, c_stream]),
    "rdgan_seq_minplus": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, c_stream]),
    "rdgan_seq_match": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, c_stream]),
    "rdgan_assign": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                    ctypes.c_void_p, c_stream]),
    "rdgan_red_workspace_bytes": (ctypes.c_long, [ctypes.c_long, ctypes.c_long]),
    "rdgan_red_features": (ctypes.c_int, [c_f32p, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_int,
                                          ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, c_stream]),
    "rdgan_red_distances": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_int,
                                           ctypes.c_void_p, ctypes.c_void_p, c_stream]),
    "rdgan_red_select": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, c_stream]),
    "rdgan_mvr_ranks_workspace_bytes": (ctypes.c_long, [ctypes.c_long, ctypes.c_long, ctypes.c_int]),
    "rdgan_mvr_ranks": (ctypes.c_int, [c_f32p, c_f32p, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, c_stream]),
    "rdgan_mvr_mst": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, c_stream]),
    "rdgan_mv_energy_workspace_bytes": (ctypes.c_long, [ctypes.c_long, ctypes.c_long, ctypes.c_int]),
    "rdgan_mv_energy": (ctypes.c_int, [c_f32p, c_f32p, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_int, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, c_stream]),
    "rdgan_mv_variogram_workspace_bytes": (ctypes.c_long, [ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "rdgan_mv_variogram": (ctypes.c_int, [c_f32p, c_f32p, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_int, ctypes.c_double,
                                          ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, c_stream]),
    "rdgan_cascade_state_size": (ctypes.c_long, [ctypes.c_int]),
    "rdgan_cascade_accumulate": (ctypes.c_int, [c_f32p, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_void_p,
                                                ctypes.c_int, ctypes.c_void_p, c_stream]),
    "rdgan_cascade_generate": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, c_f32p, ctypes.c_long, ctypes.c_long,
                                              ctypes.c_long, ctypes.c_long, ctypes.c_int, ctypes.c_long, ctypes.c_uint64, ctypes.c_int,
                                              c_f32p, ctypes.c_void_p, c_stream]),
    "rdgan_block_maxima_accumulate": (ctypes.c_int, [c_f32p, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_void_p,
                                                     ctypes.c_long, ctypes.c_uint, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                     ctypes.c_void_p, c_stream]),
    "rdgan_lmoment_sums": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_int, ctypes.c_long,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_stream]),
    "rdgan_spectra_bins": (ctypes.c_int, [ctypes.c_int]),
    "rdgan_radial_spectra": (ctypes.c_int, [c_f32p, c_f32p, ctypes.c_long, ctypes.c_int, ctypes.c_int, c_stream]),
    "rdgan_lsd_workspace_bytes": (ctypes.c_long, [ctypes.c_long, ctypes.c_long]),
    "rdgan_lsd_pairwise": (ctypes.c_int, [c_f32p, c_f32p, ctypes.c_long, ctypes.c_long, ctypes.c_int, ctypes.c_int, c_f32p,
                                          ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_long, c_stream]),
    "rdgan_rainfarm_classes": (ctypes.c_int, [ctypes.c_int]),
    "rdgan_rainfarm_stats_workspace_bytes": (ctypes.c_long, [ctypes.c_long, ctypes.c_int]),
    "rdgan_rainfarm_slope_stats": (ctypes.c_int, [c_f32p, ctypes.c_long, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_void_p, ctypes.c_long, c_stream]),
    "rdgan_rainfarm_gen_workspace_bytes": (ctypes.c_long, [ctypes.c_long]),
    "rdgan_rainfarm_generate": (ctypes.c_int, [c_f32p, c_f32p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64,
                                               ctypes.c_long, c_f32p, ctypes.c_long, ctypes.c_int, ctypes.c_void_p, ctypes.c_long,
                                               c_stream]),
    "rdgan_op_conv3d": (ctypes.c_int, [c_f32p, c_f32p, c_f32p, c_f32p] + [ctypes.c_int] * 14 + [c_stream]),
    "rdgan_op_conv3d_bf16": (ctypes.c_int, [c_f32p, c_f32p, c_f32p, c_f32p] + [ctypes.c_int] * 14 + [c_stream]),
    "rdgan_op_conv3d_dgrad": (ctypes.c_int, [c_f32p, c_f32p, c_f32p] + [ctypes.c_int] * 13 + [c_stream]),
    "rdgan_op_conv3d_wgrad_bf16": (ctypes.c_int, [c_f32p, c_f32p, c_f32p] + [ctypes.c_int] * 13 + [c_stream]),
    "rdgan_op_conv3d_dgrad_bf16": (ctypes.c_int, [c_f32p, c_f32p, c_f32p] + [ctypes.c_int] * 13 + [c_stream]),
    "rdgan_op_conv3d_wgrad": (ctypes.c_int, [c_f32p, c_f32p, c_f32p] + [ctypes.c_int] * 14 + [c_stream]),
    "rdgan_op_fastd_wgrad": (ctypes.c_int, [c_f32p, c_f32p, c_f32p] + [ctypes.c_int] * 8 + [c_stream]),
    "rdgan_op_g9_wgrad": (ctypes.c_int, [c_f32p, c_f32p, c_f32p] + [ctypes.c_int] * 4 + [c_stream]),
    "rdgan_op_upconv_slab16": (ctypes.c_int, [c_f32p] * 6 + [ctypes.c_int, c_stream]),
    "rdgan_op_upconv_slab_t16": (ctypes.c_int, [c_f32p] * 6 + [ctypes.c_int] * 3 + [c_stream]),
    "rdgan_op_upconv2_slab16": (ctypes.c_int, [c_f32p] * 5 + [ctypes.c_int, c_stream]),
    "rdgan_op_upconv_wgrad_slab16": (ctypes.c_int, [c_f32p] * 3 + [ctypes.c_int, c_stream]),
    "rdgan_op_d2_fwd_slab16": (ctypes.c_int, [c_f32p] * 4 + [ctypes.c_int, ctypes.c_uint64, c_stream]),
    "rdgan_op_d3_wgrad_slab16": (ctypes.c_int, [c_f32p] * 3 + [ctypes.c_int, c_stream]),
    "rdgan_op_d2_wgrad_slab16": (ctypes.c_int, [c_f32p] * 3 + [ctypes.c_int, c_stream]),
    "rdgan_op_d2_wgrad_slab_t16": (ctypes.c_int, [c_f32p] * 3 + [ctypes.c_int] * 3 + [c_stream]),
    "rdgan_op_d2_dgrad_slab16": (ctypes.c_int, [c_f32p] * 4 + [ctypes.c_int, ctypes.c_int, c_stream]),
    "rdgan_op_d2_dgrad_slab_t16": (ctypes.c_int, [c_f32p] * 4 + [ctypes.c_int] * 4 + [c_stream]),
    "rdgan_op_pixelnorm_lrelu": (ctypes.c_int, [c_f32p, c_f32p, c_f32p, ctypes.c_long, ctypes.c_int, c_stream]),
    "rdgan_op_pixelnorm_lrelu_bwd": (ctypes.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, ctypes.c_long, ctypes.c_int, c_stream]),
    "rdgan_op_softmax_tail": (ctypes.c_int, [ctypes.c_int, c_f32p, c_f32p, c_f32p, ctypes.c_void_p] + [ctypes.c_int] * 3 + [c_stream]),
    "rdgan_op_softmax_bwd": (ctypes.c_int, [c_f32p] * 3 + [ctypes.c_int] * 3 + [c_stream]),
    "rdgan_op_gp_norm": (ctypes.c_int, [c_f32p] + [ctypes.c_int] * 4 + [c_f32p, c_f32p, c_stream]),
    "rdgan_op_loss_tail": (ctypes.c_int, [ctypes.c_int, c_f32p, c_f32p, ctypes.c_int, ctypes.c_int, c_f32p, c_stream]),
    "rdgan_op_critic_dense": (ctypes.c_int, [ctypes.c_void_p, c_f32p, c_f32p, c_f32p, ctypes.c_void_p] + [ctypes.c_int] * 4 +
                              [ctypes.c_uint64, ctypes.c_int, c_stream]),
    "rdgan_op_critic_dense_wgrad": (ctypes.c_int, [ctypes.c_void_p, c_f32p] + [ctypes.c_int] * 5 + [c_stream]),
    "rdgan_op_weight_forms": (ctypes.c_int, [ctypes.c_int, c_f32p, c_f32p, ctypes.c_long, c_stream]),
    "rdgan_op_weight_forms_adj": (ctypes.c_int, [ctypes.c_int, c_f32p, c_f32p, ctypes.c_long, c_stream]),
    "rdgan_op_critic_input": (ctypes.c_int, [c_f32p] * 4 + [ctypes.c_int] * 6 + [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, c_stream]),
    "rdgan_op_pool_lrelu_bwd": (ctypes.c_int, [c_f32p] * 3 + [ctypes.c_int] * 5 + [c_stream]),
    "rdgan_op_lrelu_bwd": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, c_f32p, ctypes.c_long, ctypes.c_int, c_stream]),
    "rdgan_op_colsum": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_int, c_f32p, ctypes.c_int, c_stream]),
    "rdgan_op_diff_combine": (ctypes.c_int, [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_int, ctypes.c_long, ctypes.c_int, c_stream]),
    "rdgan_debug_activation": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_f32p, ctypes.c_long, c_stream]),
    "rdgan_debug_d1_input_grad": (ctypes.c_int, [ctypes.c_void_p, c_f32p, c_f32p, ctypes.c_int, ctypes.c_int, c_f32p, c_f32p, c_f32p,
                                                 c_stream]),
    "rdgan_op_rng": (ctypes.c_int, [ctypes.c_uint64, ctypes.c_uint32, c_f32p, c_f32p, ctypes.c_long, c_stream]),
}

TAG_GCONV_FWD, TAG_GCONV_DGRAD, TAG_GCONV_WGRAD, TAG_CRITIC_GEMM, TAG_ELEMENTWISE, TAG_GCONV3_FWD = range(6)

_lib = None


class RdganError(RuntimeError):
    pass


class NumericsError(RdganError, ArithmeticError):
    """tf.debugging.check_numerics behind the generator's softmax (reference T:349-350) fired: NaN/Inf in the output."""


def load():
    """Load the HIP library and bind every declared symbol.  Raises (never falls back)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RdganError(
            f"{LIB_PATH} is missing: build it with `python -m pr_disagg_radar_gan_amd.build` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback for the product path.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)      # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, handle=None, what=""):
    if rc == 0:
        return
    msg = ""
    if handle is not None and _lib is not None:
        m = _lib.rdgan_last_error(handle)
        msg = m.decode() if m else ""
    raise RdganError(f"{what} failed with code {rc}" + (f": {msg}" if msg else ""))
