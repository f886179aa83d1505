"""ctypes plumbing over the C-ABI (include/boom_amd.h, boom_amd/libboomamd.so).

This is NOT a compute path: every call goes straight into the HIP library and
fails loudly when the library or a GPU is missing.  There is no CPU fallback.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# BOOM_AMD_LIB selects another build of the SAME library (e.g. the -DBA_STAMPS
# diagnostic build); it is never a different backend
LIB_PATH = os.environ.get("BOOM_AMD_LIB", os.path.join(_HERE, "libboomamd.so"))

_dp = C.POINTER(C.c_double)
_u8p = C.POINTER(C.c_uint8)

SUMMARY_SCALARS = 16


class BoomAmdError(RuntimeError):
    """The C-ABI returned an error; mirrors BOOM's report_error ->
    std::runtime_error (cpputil/report_error.cpp:30-32)."""

    def __init__(self, code, message):
        super().__init__(message)
        self.code = code


class BaConfig(C.Structure):
    _fields_ = [("device", C.c_int32), ("chains", C.c_int32),
                ("chain_offset", C.c_int64), ("seed", C.c_uint64),
                ("max_model_size_hint", C.c_int32), ("reserved", C.c_int32)]


_lib = None

# name -> (restype, argtypes); must list every symbol include/boom_amd.h declares
SIGNATURES = {
    "ba_last_error": (C.c_char_p, []),
    "ba_engine_create": (C.c_int, [C.POINTER(BaConfig), C.POINTER(C.c_void_p)]),
    "ba_engine_destroy": (None, [C.c_void_p]),
    "ba_engine_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32),
                                 C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ba_build_suf_from_xy": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, _dp, _dp]),
    "ba_build_suf_from_xy_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32,
                                              C.c_void_p, C.c_void_p]),
    "ba_suf_block_size": (C.c_size_t, [C.c_int32]),
    "ba_suf_partial_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "ba_set_suf_from_block_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]),
    "ba_upload_regression_suf": (C.c_int, [C.c_void_p, C.c_int32, _dp, _dp,
                                           C.c_double, C.c_double, C.c_double, _dp]),
    "ba_get_regression_suf": (C.c_int, [C.c_void_p, _dp, _dp, _dp, _dp, _dp, _dp]),
    "ba_set_slab": (C.c_int, [C.c_void_p, _dp, _dp]),
    "ba_set_spike": (C.c_int, [C.c_void_p, _dp, C.c_int64]),
    "ba_set_sigma_prior": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double]),
    "ba_set_priors_ctor1": (C.c_int, [C.c_void_p, C.c_double, C.c_double,
                                      C.c_double, C.c_int32]),
    "ba_set_priors_ctor2": (C.c_int, [C.c_void_p, C.c_double, C.c_double,
                                      C.c_double, C.c_double, C.c_double, C.c_int32]),
    "ba_get_priors": (C.c_int, [C.c_void_p, _dp, _dp, _dp, _dp, _dp]),
    "ba_set_options": (C.c_int, [C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.c_int32]),
    "ba_set_tuning": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "ba_set_rebuild_policy": (C.c_int, [C.c_void_p, C.c_int32]),
    "ba_set_lookahead": (C.c_int, [C.c_void_p, C.c_int32]),
    "ba_draw_next": (C.c_int, [C.c_void_p]),
    "ba_set_state": (C.c_int, [C.c_void_p, C.c_int64, _u8p, _dp, C.c_double]),
    "ba_get_state": (C.c_int, [C.c_void_p, C.c_int64, _u8p, _dp, _dp]),
    "ba_get_states": (C.c_int, [C.c_void_p, _u8p, _dp, _dp]),
    "ba_logpri": (C.c_int, [C.c_void_p, C.c_int64, _dp]),
    "ba_seed": (C.c_int, [C.c_void_p, C.c_uint64]),
    "ba_sweep": (C.c_int, [C.c_void_p, C.c_int32]),
    "ba_sync": (C.c_int, [C.c_void_p]),
    "ba_log_model_prob": (C.c_int, [C.c_void_p, C.c_int32, _u8p, _dp]),
    "ba_set_sigsq": (C.c_int, [C.c_void_p, C.c_int64, C.c_double]),
    "ba_sss_set_slab": (C.c_int, [C.c_void_p, _dp, _dp, C.c_int32, C.c_int32]),
    "ba_sss_sweep": (C.c_int, [C.c_void_p, C.c_int32]),
    "ba_adaptive_set_options": (C.c_int, [C.c_void_p, C.c_int32, C.c_double, C.c_double]),
    "ba_adaptive_sweep": (C.c_int, [C.c_void_p, C.c_int32]),
    "ba_adaptive_get_rates": (C.c_int, [C.c_void_p, C.c_int64, _dp, _dp,
                                        C.POINTER(C.c_uint64)]),
    "ba_reset_summaries": (C.c_int, [C.c_void_p]),
    "ba_get_summaries": (C.c_int, [C.c_void_p, _dp, _dp, _dp, _dp]),
    "ba_summaries_device": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ba_enable_traces": (C.c_int, [C.c_void_p, C.c_int32]),
    "ba_get_traces": (C.c_int, [C.c_void_p, C.c_int32, _dp, _dp, _dp]),
    "ba_enable_draws": (C.c_int, [C.c_void_p, C.c_int32]),
    "ba_get_draws": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, _u8p, _dp, _dp]),
    "ba_predict": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, _dp, _dp]),
    "ba_get_coefficient_traces": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32,
                                            C.POINTER(C.c_int32), _dp]),
    "ba_stream": (C.c_void_p, [C.c_void_p]),
    "ba_kernel_classes": (C.c_int32, []),
    "ba_kernel_class_name": (C.c_char_p, [C.c_int32]),
    "ba_set_kernel_timing": (C.c_int, [C.c_void_p, C.c_int32]),
    "ba_get_kernel_times": (C.c_int, [C.c_void_p, _dp, C.POINTER(C.c_int64), C.c_int32]),
    "ba_group_last_error": (C.c_char_p, []),
    "ba_group_rccl_available": (C.c_int32, []),
    "ba_group_create": (C.c_int, [C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_uint64,
                                  C.POINTER(C.c_void_p)]),
    "ba_group_destroy": (None, [C.c_void_p]),
    "ba_group_size": (C.c_int32, [C.c_void_p]),
    "ba_group_engine": (C.c_void_p, [C.c_void_p, C.c_int32]),
    "ba_group_locate": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "ba_group_build_suf_from_xy": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, _dp, _dp]),
    "ba_group_set_priors": (C.c_int, [C.c_void_p, _dp, _dp, _dp, C.c_int64, C.c_double, C.c_double,
                                      C.c_double]),
    "ba_group_set_state": (C.c_int, [C.c_void_p, _u8p, _dp, C.c_double]),
    "ba_group_sweep": (C.c_int, [C.c_void_p, C.c_int32]),
    "ba_group_sync": (C.c_int, [C.c_void_p]),
    "ba_group_call": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "ba_group_ss_sweep": (C.c_int, [C.c_void_p, C.c_int32]),
    "ba_group_ss_draw_next": (C.c_int, [C.c_void_p]),
    "ba_group_logit_sweep": (C.c_int, [C.c_void_p, C.c_int32]),
    "ba_group_poisson_sweep": (C.c_int, [C.c_void_p, C.c_int32]),
    "ba_group_reset_summaries": (C.c_int, [C.c_void_p]),
    "ba_group_get_summaries": (C.c_int, [C.c_void_p, _dp, _dp, _dp, _dp, _dp]),
    "ba_ss_set_data": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _dp, _dp, _u8p]),
    "ba_ss_set_local_level": (C.c_int, [C.c_void_p] + [C.c_double] * 6),
    "ba_probit_set_data": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, _dp, _dp, _dp, C.c_int32]),
    "ba_probit_sweep": (C.c_int, [C.c_void_p, C.c_int32]),
    "ba_logit_set_data": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, _dp, _dp, _dp, C.c_int32]),
    "ba_logit_sweep": (C.c_int, [C.c_void_p, C.c_int32]),
    "ba_logit_set_imputer": (C.c_int, [C.c_void_p, C.c_int32]),
    "ba_poisson_set_data": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, _dp, _dp, _dp]),
    "ba_poisson_set_mixtures": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64),
                                          C.POINTER(C.c_int32), _dp, _dp, _dp, C.c_int64]),
    "ba_poisson_sweep": (C.c_int, [C.c_void_p, C.c_int32]),
    "ba_ss_student_set_data": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _dp, _dp, _u8p]),
    "ba_ss_student_sweep": (C.c_int, [C.c_void_p, C.c_int32]),
    "ba_ss_student_get_weights": (C.c_int, [C.c_void_p, C.c_int64, _dp]),
    "ba_ss_student_set_weights": (C.c_int, [C.c_void_p, C.c_int64, _dp]),
    "ba_ss_student_impute_state": (C.c_int, [C.c_void_p]),
    "ba_ss_poisson_set_data": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _dp, _dp, _dp, _u8p]),
    "ba_ss_poisson_sweep": (C.c_int, [C.c_void_p, C.c_int32]),
    "ba_ss_poisson_impute_state": (C.c_int, [C.c_void_p]),
    "ba_ss_poisson_get_latent": (C.c_int, [C.c_void_p, C.c_int64, _dp, _dp]),
    "ba_ss_poisson_set_latent": (C.c_int, [C.c_void_p, C.c_int64, _dp, _dp]),
    "ba_ss_logit_set_data": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _dp, _dp, _dp, _u8p, C.c_int32]),
    "ba_ss_logit_sweep": (C.c_int, [C.c_void_p, C.c_int32]),
    "ba_ss_logit_impute_state": (C.c_int, [C.c_void_p]),
    "ba_ss_logit_get_latent": (C.c_int, [C.c_void_p, C.c_int64, _dp, _dp]),
    "ba_ss_logit_set_latent": (C.c_int, [C.c_void_p, C.c_int64, _dp, _dp]),
    "ba_student_set_data": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, _dp, _dp]),
    "ba_student_set_nu_prior": (C.c_int, [C.c_void_p, C.c_int32, C.c_double, C.c_double]),
    "ba_student_set_nu": (C.c_int, [C.c_void_p, C.c_int64, C.c_double]),
    "ba_student_get_nu": (C.c_int, [C.c_void_p, C.c_int64, _dp]),
    "ba_student_sweep": (C.c_int, [C.c_void_p, C.c_int32]),
    "ba_student_get_weights": (C.c_int, [C.c_void_p, C.c_int64, _dp]),
    "ba_student_get_nu_draws": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, _dp]),
    "ba_student_get_margin": (C.c_int, [C.c_void_p, C.c_int64, _dp]),
    "ba_student_allow_model_selection": (C.c_int, [C.c_void_p, C.c_int32]),
    "ba_quantile_set_data": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, _dp, _dp, C.c_double]),
    "ba_quantile_sweep": (C.c_int, [C.c_void_p, C.c_int32]),
    "ba_quantile_get_weights": (C.c_int, [C.c_void_p, C.c_int64, _dp]),
    "ba_mlogit_set_data": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                     C.POINTER(C.c_int32), _dp, _dp]),
    "ba_mlogit_set_flip_order": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "ba_mlogit_allow_model_selection": (C.c_int, [C.c_void_p, C.c_int32]),
    "ba_mlogit_sweep": (C.c_int, [C.c_void_p, C.c_int32]),
    "ba_mlogit_get_latent": (C.c_int, [C.c_void_p, C.c_int64, _dp, _dp]),
    "ba_mlogit_get_wss": (C.c_int, [C.c_void_p, C.c_int64, _dp]),
    "ba_ss_set_structural": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32] + [_dp] * 6),
    "ba_ss_get_structural": (C.c_int, [C.c_void_p, C.c_int64, _dp, _dp, _dp, _dp]),
    "ba_ss_add_ar": (C.c_int, [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_double,
                               C.c_double, _dp, _dp, _dp]),
    "ba_ss_get_ar": (C.c_int, [C.c_void_p, C.c_int64, _dp, _dp, _dp, _dp, _dp, _dp]),
    "ba_ss_clear_state_models": (C.c_int, [C.c_void_p]),
    "ba_ss_set_tuning": (C.c_int, [C.c_void_p, C.c_int32]),
    "ba_set_slot_limit": (C.c_int, [C.c_void_p, C.c_int32]),
    "ba_ss_add_state_model": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32)] + [_dp] * 7),
    "ba_ss_state_dimension": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ba_ss_get_state_model": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32] + [_dp] * 8),
    "ba_ss_get_state_draw": (C.c_int, [C.c_void_p, C.c_int64, _dp]),
    "ba_ss_sweep": (C.c_int, [C.c_void_p, C.c_int32]),
    "ba_ss_set_lookahead": (C.c_int, [C.c_void_p, C.c_int32]),
    "ba_ss_lookahead_chains": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64)]),
    "ba_ss_draw_next": (C.c_int, [C.c_void_p]),
    "ba_ss_impute_state": (C.c_int, [C.c_void_p]),
    "ba_ss_trend_get_weights": (C.c_int, [C.c_void_p, C.c_int64, _dp, _dp]),
    "ba_ss_trend_set_weights": (C.c_int, [C.c_void_p, C.c_int64, _dp, _dp]),
    "ba_ss_trend_get_weight_suf": (C.c_int, [C.c_void_p, C.c_int64, _dp]),
    "ba_ss_trend_draw_parameters": (C.c_int, [C.c_void_p]),
    "ba_ss_autoar_draw_parameters": (C.c_int, [C.c_void_p]),
    "ba_ss_get_ar_inclusion": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_uint8)]),
    "ba_ss_set_holiday_calendar": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_int64]),
    "ba_ss_get_holiday_calendar": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "ba_ss_set_season_calendar": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_uint8), C.c_int64]),
    "ba_ss_get_season_calendar": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_uint8), C.POINTER(C.c_int64)]),
    "ba_monthly_cycle_calendar": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_uint8)]),
    "ba_ss_add_dynamic_regression": (C.c_int, [C.c_void_p, C.c_int32, _dp, C.c_int64, _dp, _dp, _dp, _dp, _dp, _dp]),
    "ba_ss_add_dynamic_regression_ar": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _dp, C.c_int64, _dp, _dp, _dp, _dp, _dp, _dp, _dp,
                                                  C.POINTER(C.c_int32)]),
    "ba_ss_set_dynamic_predictors": (C.c_int, [C.c_void_p, C.c_int32, _dp, C.c_int64]),
    "ba_ss_get_dynamic_predictors": (C.c_int, [C.c_void_p, C.c_int32, _dp, C.POINTER(C.c_int64)]),
    "ba_ss_add_regression_holiday": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_double, C.c_double, _dp,
                                               C.POINTER(C.c_int32)]),
    "ba_ss_set_regression_holiday_calendar": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_int64]),
    "ba_ss_get_regression_holiday_calendar": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "ba_ss_get_regression_holiday": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, _dp, _dp, _dp]),
    "ba_ss_set_regression_holiday": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, _dp]),
    "ba_ss_add_hierarchical_regression_holiday": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _dp, _dp, _dp, C.c_double, _dp,
                                                            C.POINTER(C.c_int32)]),
    "ba_ss_get_hierarchical_regression_holiday": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, _dp, _dp]),
    "ba_ss_set_hierarchical_regression_holiday": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, _dp, _dp]),
    "ba_ss_forecast": (C.c_int, [C.c_void_p, C.c_int32, _dp, _dp]),
    "ba_ss_prediction_errors": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, _dp, _dp, _dp]),
    "ba_ss_holdout_prediction_errors": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, _dp, _dp, _dp, _dp]),
    "ba_ss_student_forecast": (C.c_int, [C.c_void_p, C.c_int32, _dp, _dp]),
    "ba_ss_poisson_forecast": (C.c_int, [C.c_void_p, C.c_int32, _dp, _dp, _dp]),
    "ba_ss_logit_forecast": (C.c_int, [C.c_void_p, C.c_int32, _dp, _dp, _dp]),
    "ba_ss_get_state": (C.c_int, [C.c_void_p, C.c_int64, _dp, _dp, _dp, _dp]),
    "ba_ss_set_level_sigsq": (C.c_int, [C.c_void_p, C.c_int64, C.c_double]),
    "ba_ss_get_chain_suf": (C.c_int, [C.c_void_p, C.c_int64, _dp, _dp, _dp]),
}


def load_library():
    """Load libboomamd.so (no GPU needed just to load it)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "boom_amd/libboomamd.so is missing: run `python -c 'import "
                "__graft_entry__ as g; g.build()'` (hipcc, gfx950).  There is "
                "no CPU fallback.")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def monthly_cycle_calendar(year, month, day, count):
    """MonthlyAnnualCycle's calendar (ba_monthly_cycle_calendar; host only, no device): `count` flags,
    entry t is 1 where the day t days after the date of the first observation is the first of a month"""
    lib = load_library()
    out = np.zeros(max(int(count), 1), np.uint8)
    rc = lib.ba_monthly_cycle_calendar(int(year), int(month), int(day), int(count),
                                       out.ctypes.data_as(C.POINTER(C.c_uint8)))
    if rc != 0:
        raise BoomAmdError(rc, lib.ba_last_error().decode())
    return out[:int(count)]


def _f64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def _fcol(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).T).ravel()


def _p(a):
    return None if a is None else a.ctypes.data_as(_dp)


def _b(a):
    return None if a is None else a.ctypes.data_as(_u8p)


class Engine:
    """One engine = `chains` independent chains on one HIP device."""

    def __init__(self, chains, seed=8675309, device=0, chain_offset=0,
                 max_model_size_hint=0, _borrowed=None):
        self.lib = load_library()
        self._owned = _borrowed is None
        self._h = None
        if _borrowed is None:
            cfg = BaConfig(device, chains, chain_offset, seed, max_model_size_hint, 0)
            h = C.c_void_p()
            self._check(self.lib.ba_engine_create(C.byref(cfg), C.byref(h)))
            self._h = h
        else:
            self._h = C.c_void_p(_borrowed)   # an engine of a Group: the group owns it
        self.chains = chains
        self.p = 0

    def _check(self, rc):
        if rc != 0:
            raise BoomAmdError(rc, self.lib.ba_last_error().decode())

    def close(self):
        if self._h is not None:
            if self._owned:
                self.lib.ba_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- data ---------------------------------------------------------------
    def build_suf_from_xy(self, X, y):
        n, p = X.shape
        self._check(self.lib.ba_build_suf_from_xy(self._h, n, p, _p(_fcol(X)), _p(_f64(y))))
        self.p = p

    def build_suf_from_xy_device(self, n, p, x_ptr, y_ptr):
        self._check(self.lib.ba_build_suf_from_xy_device(self._h, n, p, x_ptr, y_ptr))
        self.p = p

    def suf_block_size(self, p):
        return int(self.lib.ba_suf_block_size(p))

    def suf_partial_device(self, n_rows, p, x_ptr, y_ptr, block_ptr):
        self._check(self.lib.ba_suf_partial_device(self._h, n_rows, p, x_ptr, y_ptr, block_ptr))

    def set_suf_from_block_device(self, n_total, p, block_ptr):
        self._check(self.lib.ba_set_suf_from_block_device(self._h, n_total, p, block_ptr))
        self.p = p

    def upload_suf(self, xtx, xty, yty, n, ybar, xbar):
        p = len(xty)
        self._check(self.lib.ba_upload_regression_suf(
            self._h, p, _p(_fcol(xtx)), _p(_f64(xty)), yty, n, ybar, _p(_f64(xbar))))
        self.p = p

    def get_suf(self):
        p = self.p
        xtx = np.zeros(p * p)
        xty = np.zeros(p)
        xbar = np.zeros(p)
        yty, n, ybar = C.c_double(), C.c_double(), C.c_double()
        self._check(self.lib.ba_get_regression_suf(self._h, _p(xtx), _p(xty), C.byref(yty),
                                                   C.byref(n), C.byref(ybar), _p(xbar)))
        return dict(xtx=xtx.reshape(p, p).T.copy(), xty=xty, yty=yty.value,
                    n=n.value, ybar=ybar.value, xbar=xbar)

    # ---- priors -------------------------------------------------------------
    def set_priors(self, b, ominv, pi, prior_df, sigma_guess,
                   max_model_size=-1, sigma_upper_limit=float("inf")):
        self._check(self.lib.ba_set_slab(self._h, _p(_f64(b)), _p(_fcol(ominv))))
        self._check(self.lib.ba_set_spike(self._h, _p(_f64(pi)), int(max_model_size)))
        self._check(self.lib.ba_set_sigma_prior(self._h, prior_df, sigma_guess,
                                                sigma_upper_limit))

    def set_priors_ctor1(self, prior_nobs, expected_rsq, expected_model_size,
                         first_term_is_intercept=True):
        self._check(self.lib.ba_set_priors_ctor1(self._h, prior_nobs, expected_rsq,
                                                 expected_model_size,
                                                 int(first_term_is_intercept)))

    def set_priors_ctor2(self, prior_sigma_nobs, prior_sigma_guess, prior_beta_nobs,
                         diagonal_shrinkage, prior_inclusion_probability,
                         force_intercept=True):
        self._check(self.lib.ba_set_priors_ctor2(
            self._h, prior_sigma_nobs, prior_sigma_guess, prior_beta_nobs,
            diagonal_shrinkage, prior_inclusion_probability, int(force_intercept)))

    def get_priors(self):
        p = self.p
        b, om, pi = np.zeros(p), np.zeros(p * p), np.zeros(p)
        df, ss = C.c_double(), C.c_double()
        self._check(self.lib.ba_get_priors(self._h, _p(b), _p(om), _p(pi),
                                           C.byref(df), C.byref(ss)))
        return dict(b=b, ominv=om.reshape(p, p).T.copy(), pi=pi, df=df.value, ss=ss.value)

    def set_options(self, max_flips=-1, swap_threshold=0.8, draw_beta=True,
                    draw_sigma=True):
        self._check(self.lib.ba_set_options(self._h, max_flips, swap_threshold,
                                            int(draw_beta), int(draw_sigma)))

    def set_tuning(self, waves_per_chain=0, walk_policy=-1, kcap_start=0):
        """overrides of choices the engine makes itself (the same chains whatever is set).
        walk_policy: -1 default (1); 0 batch mode only; 1 adaptive, 2 always the table -- with
        helper wavefronts both run EVERY table walk beside the master's tail, the one a sweep
        starts with and the ones resumed after a stop; 3 adaptive, no walk forked; 4 adaptive,
        forking at a sweep's start only (what 1 did before resumed walks forked: A/B, tests)"""
        self._check(self.lib.ba_set_tuning(self._h, waves_per_chain, walk_policy, kcap_start))

    def set_rebuild_policy(self, policy):
        """how an accepted (or exactly evaluated) single flip rebuilds the factors: 0 keeps
        the columns the flip leaves unchanged, 1 factors from scratch; same draws either way"""
        self._check(self.lib.ba_set_rebuild_policy(self._h, int(policy)))

    # ---- state --------------------------------------------------------------
    def set_state(self, gamma, beta=None, sigsq=1.0, chain=-1):
        g = np.ascontiguousarray(gamma, dtype=np.uint8)
        bb = None if beta is None else _f64(beta)
        self._check(self.lib.ba_set_state(self._h, chain, _b(g), _p(bb), sigsq))

    def get_state(self, chain):
        p = self.p
        g = np.zeros(p, np.uint8)
        b = np.zeros(p)
        s = C.c_double()
        self._check(self.lib.ba_get_state(self._h, chain, _b(g), _p(b), C.byref(s)))
        return g, b, s.value

    def get_states(self):
        p, c = self.p, self.chains
        g = np.zeros((c, p), np.uint8)
        b = np.zeros((c, p))
        s = np.zeros(c)
        self._check(self.lib.ba_get_states(self._h, _b(g), _p(b), _p(s)))
        return g, b, s

    def seed(self, seed):
        self._check(self.lib.ba_seed(self._h, seed))

    # ---- sampling -----------------------------------------------------------
    def sweep(self, nsweeps=1, sync=True):
        self._check(self.lib.ba_sweep(self._h, nsweeps))
        if sync:
            self.sync()

    def sync(self):
        self._check(self.lib.ba_sync(self._h))

    def set_lookahead(self, n):
        self._check(self.lib.ba_set_lookahead(self._h, n))

    def draw_next(self):
        self._check(self.lib.ba_draw_next(self._h))

    def log_model_prob(self, gammas):
        G = np.ascontiguousarray(gammas, dtype=np.uint8)
        out = np.zeros(len(G))
        self._check(self.lib.ba_log_model_prob(self._h, len(G), _b(G), _p(out)))
        return out

    # ---- SpikeSlabSampler (sigma^2 given) --------------------------------------
    def set_sigsq(self, sigsq, chain=-1):
        self._check(self.lib.ba_set_sigsq(self._h, chain, float(sigsq)))

    def sss_set_slab(self, mu, precision, scales_with_sigsq=True, max_flips=-1):
        self._check(self.lib.ba_sss_set_slab(self._h, _p(_f64(mu)), _p(_fcol(precision)),
                                             int(scales_with_sigsq), int(max_flips)))

    def set_spike(self, pi, max_model_size=-1):
        self._check(self.lib.ba_set_spike(self._h, _p(_f64(pi)), int(max_model_size)))

    def sss_sweep(self, nsweeps=1, sync=True):
        self._check(self.lib.ba_sss_sweep(self._h, nsweeps))
        if sync:
            self.sync()

    # ---- AdaptiveSpikeSlabRegressionSampler ---------------------------------------
    def adaptive_set_options(self, max_flips=-1, step_size=-1.0, target=-1.0):
        self._check(self.lib.ba_adaptive_set_options(self._h, max_flips, step_size, target))

    def adaptive_sweep(self, nsweeps=1, sync=True):
        self._check(self.lib.ba_adaptive_sweep(self._h, nsweeps))
        if sync:
            self.sync()

    def adaptive_get_rates(self, chain):
        b, d = np.zeros(self.p), np.zeros(self.p)
        it = C.c_uint64()
        self._check(self.lib.ba_adaptive_get_rates(self._h, chain, _p(b), _p(d), C.byref(it)))
        return b, d, it.value

    # ---- summaries ----------------------------------------------------------
    def reset_summaries(self):
        self._check(self.lib.ba_reset_summaries(self._h))

    def get_summaries(self):
        p = self.p
        inc, bs, bs2 = np.zeros(p), np.zeros(p), np.zeros(p)
        sc = np.zeros(SUMMARY_SCALARS)
        self._check(self.lib.ba_get_summaries(self._h, _p(inc), _p(bs), _p(bs2), _p(sc)))
        return dict(inclusion_count=inc, beta_sum=bs, beta_sumsq=bs2,
                    sweeps=sc[0], sigsq_sum=sc[1], sigsq_sumsq=sc[2], k_sum=sc[3],
                    accepts=sc[4], proposals=sc[5], min_margin=sc[6],
                    # scalar 7: accepted flips served from a chain's other slot
                    # (diagnostic stamp builds reuse it for the slowest chain's cycles)
                    slot_hits=float(sc[7]), phase_cycles=sc[8:16].copy(),
                    # after adaptive sweeps: closest approach of a weighted-draw
                    # uniform to a boundary of the cumulative rates
                    min_multi_margin=float(sc[8]),
                    # after plain sweeps of the product library: rebuilds that kept the
                    # leading factor columns, and how many columns they kept (the
                    # diagnostic stamp builds use these slots for cycles)
                    partial_rebuilds=float(sc[9]), columns_kept=float(sc[10]),
                    # ... table walks resumed after a stop (or started unforked) that ran
                    # beside the master's tail, and those that found a stop and rolled it back
                    reforks=float(sc[11]), refork_rollbacks=float(sc[12]))

    def summaries_device(self, ptr):
        self._check(self.lib.ba_summaries_device(self._h, ptr))

    def enable_traces(self, max_sweeps):
        self._check(self.lib.ba_enable_traces(self._h, max_sweeps))

    def logpri(self, chain=0):
        out = C.c_double()
        self._check(self.lib.ba_logpri(self._h, chain, C.byref(out)))
        return out.value

    def enable_draws(self, max_sweeps):
        self._check(self.lib.ba_enable_draws(self._h, max_sweeps))

    def get_draws(self, chain, nsweeps):
        """the recorded draws of one chain (local index) of the last sweep() call"""
        p = self.p
        g = np.zeros((nsweeps, p), np.uint8)
        b = np.zeros((nsweeps, p))
        s = np.zeros(nsweeps)
        self._check(self.lib.ba_get_draws(self._h, chain, nsweeps, _b(g), _p(b), _p(s)))
        return g, b, s

    def predict(self, newX, first_draw, ndraws):
        """posterior predictive means newX beta for the recorded draws [first_draw,
        first_draw + ndraws) of every chain: chains x ndraws x len(newX)"""
        Xn = np.asfortranarray(np.atleast_2d(newX), dtype=np.float64)
        out = np.zeros((self.chains, ndraws, Xn.shape[0]))
        self._check(self.lib.ba_predict(self._h, first_draw, ndraws, Xn.shape[0],
                                        Xn.ctypes.data_as(_dp), _p(out)))
        return out

    def get_coefficient_traces(self, nsweeps, variables):
        v = np.ascontiguousarray(variables, dtype=np.int32)
        out = np.zeros((self.chains, len(v), nsweeps))
        self._check(self.lib.ba_get_coefficient_traces(
            self._h, nsweeps, len(v), v.ctypes.data_as(C.POINTER(C.c_int32)), _p(out)))
        return out

    def get_traces(self, nsweeps):
        c = self.chains
        s, l, k = (np.zeros((c, nsweeps)) for _ in range(3))
        self._check(self.lib.ba_get_traces(self._h, nsweeps, _p(s), _p(l), _p(k)))
        return dict(sigsq=s, logp=l, model_size=k)

    def stream(self):
        return self.lib.ba_stream(self._h)

    # ---- measurement ----------------------------------------------------------
    def set_kernel_timing(self, enabled=True, overlap=False):
        """overlap=True: consecutive sweep launches still overlap while timed (mode 2)"""
        self._check(self.lib.ba_set_kernel_timing(self._h, 2 if (enabled and overlap) else int(enabled)))

    def kernel_times(self, reset=True):
        """{kernel class: (milliseconds, launches)} since the last reset"""
        n = self.lib.ba_kernel_classes()
        ms = np.zeros(n)
        cnt = np.zeros(n, np.int64)
        self._check(self.lib.ba_get_kernel_times(
            self._h, _p(ms), cnt.ctypes.data_as(C.POINTER(C.c_int64)), int(reset)))
        return {self.lib.ba_kernel_class_name(i).decode(): (float(ms[i]), int(cnt[i]))
                for i in range(n) if cnt[i] > 0}

    # ---- state space --------------------------------------------------------
    def ss_set_data(self, y, X, observed=None):
        T, p = X.shape
        obs = None if observed is None else np.ascontiguousarray(observed, np.uint8)
        self._check(self.lib.ba_ss_set_data(self._h, T, p, _p(_f64(y)), _p(_fcol(X)), _b(obs)))
        self.p = p
        self.T = T

    def ss_set_local_level(self, level_df, level_sigma_guess, level_sigma_upper_limit,
                           initial_state_mean, initial_state_variance,
                           initial_level_sigma):
        self._check(self.lib.ba_ss_set_local_level(
            self._h, level_df, level_sigma_guess, level_sigma_upper_limit,
            initial_state_mean, initial_state_variance, initial_level_sigma))

    def probit_set_data(self, X, y, ntrials, clt_threshold=5):
        X = np.asfortranarray(X, dtype=np.float64)
        self.p = X.shape[1]
        y = np.ascontiguousarray(y, dtype=np.float64)
        nt = np.ascontiguousarray(ntrials, dtype=np.float64)
        self._check(self.lib.ba_probit_set_data(self._h, X.shape[0], X.shape[1], _p(X), _p(y),
                                                _p(nt), int(clt_threshold)))

    def probit_sweep(self, nsweeps=1, sync=True):
        self._check(self.lib.ba_probit_sweep(self._h, nsweeps))
        if sync:
            self.sync()

    def logit_set_data(self, X, y, ntrials, clt_threshold=5):
        X = np.asfortranarray(X, dtype=np.float64)
        self.p = X.shape[1]
        y = np.ascontiguousarray(y, dtype=np.float64)
        nt = np.ascontiguousarray(ntrials, dtype=np.float64)
        self._check(self.lib.ba_logit_set_data(self._h, X.shape[0], X.shape[1], _p(X), _p(y),
                                               _p(nt), int(clt_threshold)))

    def poisson_set_data(self, X, y, exposure, mix):
        """mix: dict(counts, ncomp, mu, sigma, weight, largest_index) -- the reference
        table's mixtures for 1 and the positive counts in y"""
        X = np.asfortranarray(X, dtype=np.float64)
        self.p = X.shape[1]
        self._check(self.lib.ba_poisson_set_data(self._h, X.shape[0], X.shape[1], _p(X), _p(_f64(y)),
                                                 _p(_f64(exposure))))
        self._poisson_set_mixtures(mix)

    def _poisson_set_mixtures(self, mix):
        counts = np.ascontiguousarray(mix["counts"], dtype=np.int64)
        ncomp = np.ascontiguousarray(mix["ncomp"], dtype=np.int32)
        self._check(self.lib.ba_poisson_set_mixtures(
            self._h, len(counts), counts.ctypes.data_as(C.POINTER(C.c_int64)),
            ncomp.ctypes.data_as(C.POINTER(C.c_int32)), _p(_f64(mix["mu"])), _p(_f64(mix["sigma"])),
            _p(_f64(mix["weight"])), int(mix["largest_index"])))

    def poisson_sweep(self, nsweeps=1, sync=True):
        self._check(self.lib.ba_poisson_sweep(self._h, nsweeps))
        if sync:
            self.sync()

    # ---- TRegressionSpikeSlabSampler ---------------------------------------------
    def student_set_data(self, X, y):
        X = np.asfortranarray(X, dtype=np.float64)
        self.p = X.shape[1]
        self.n = X.shape[0]
        self._check(self.lib.ba_student_set_data(self._h, X.shape[0], X.shape[1], _p(X), _p(_f64(y))))

    def set_sigma_prior(self, prior_df, sigma_guess, sigma_upper_limit=float("inf")):
        self._check(self.lib.ba_set_sigma_prior(self._h, float(prior_df), float(sigma_guess),
                                                float(sigma_upper_limit)))

    def student_set_nu_prior(self, kind, a, b):
        """kind 0: Uniform(a, b); kind 1: Gamma(a, b) (shape, rate)"""
        self._check(self.lib.ba_student_set_nu_prior(self._h, int(kind), float(a), float(b)))

    def student_set_nu(self, nu, chain=-1):
        self._check(self.lib.ba_student_set_nu(self._h, int(chain), float(nu)))

    def student_get_nu(self, chain=-1):
        out = np.zeros(self.chains if chain < 0 else 1)
        self._check(self.lib.ba_student_get_nu(self._h, int(chain), _p(out)))
        return out if chain < 0 else float(out[0])

    def student_get_margin(self, chain=-1):
        out = np.zeros(self.chains if chain < 0 else 1)
        self._check(self.lib.ba_student_get_margin(self._h, int(chain), _p(out)))
        return out if chain < 0 else float(out[0])

    def student_allow_model_selection(self, allow=True):
        self._check(self.lib.ba_student_allow_model_selection(self._h, int(bool(allow))))

    def student_sweep(self, nsweeps=1, sync=True):
        self._check(self.lib.ba_student_sweep(self._h, nsweeps))
        if sync:
            self.sync()

    def student_get_weights(self, chain):
        out = np.zeros(self.n)
        self._check(self.lib.ba_student_get_weights(self._h, int(chain), _p(out)))
        return out

    def student_get_nu_draws(self, chain, nsweeps):
        out = np.zeros(int(nsweeps))
        self._check(self.lib.ba_student_get_nu_draws(self._h, int(chain), int(nsweeps), _p(out)))
        return out

    # ---- StateSpaceStudentPosteriorSampler (bsts family = "student") ---------------
    def ss_student_set_data(self, y, X, observed=None):
        T, p = X.shape
        obs = None if observed is None else np.ascontiguousarray(observed, np.uint8)
        self._check(self.lib.ba_ss_student_set_data(self._h, T, p, _p(_f64(y)), _p(_fcol(X)), _b(obs)))
        self.p = p
        self.T = T

    def ss_student_sweep(self, nsweeps=1, sync=True):
        self._check(self.lib.ba_ss_student_sweep(self._h, nsweeps))
        if sync:
            self.sync()

    def ss_student_get_weights(self, chain):
        out = np.zeros(getattr(self, "T", 1))   # (without the family's data the call is refused before it writes)
        self._check(self.lib.ba_ss_student_get_weights(self._h, int(chain), _p(out)))
        return out

    def ss_student_set_weights(self, w, chain=-1):
        self._check(self.lib.ba_ss_student_set_weights(self._h, int(chain), _p(_f64(w))))

    def ss_student_impute_state(self):
        self._check(self.lib.ba_ss_student_impute_state(self._h))
        self.sync()

    def ss_student_forecast(self, newX):
        """one predictive draw of the next len(newX) observations per chain (Student-t noise)"""
        h = newX.shape[0]
        out = np.zeros((self.chains, h))
        self._check(self.lib.ba_ss_student_forecast(self._h, h, _p(_fcol(newX)), _p(out)))
        return out

    # ---- StateSpacePoissonPosteriorSampler (bsts family = "poisson") ---------------
    def ss_poisson_set_data(self, counts, exposure, X, mix, observed=None):
        """mix: the dict poisson_set_data takes (the mixtures of 1 and of the positive counts at
        the observed steps)"""
        T, p = X.shape
        obs = None if observed is None else np.ascontiguousarray(observed, np.uint8)
        self._check(self.lib.ba_ss_poisson_set_data(self._h, T, p, _p(_f64(counts)), _p(_f64(exposure)),
                                                    _p(_fcol(X)), _b(obs)))
        self.p = p
        self.T = T
        self._poisson_set_mixtures(mix)

    def ss_poisson_sweep(self, nsweeps=1, sync=True):
        self._check(self.lib.ba_ss_poisson_sweep(self._h, nsweeps))
        if sync:
            self.sync()

    def ss_poisson_impute_state(self):
        self._check(self.lib.ba_ss_poisson_impute_state(self._h))
        self.sync()

    def ss_poisson_get_latent(self, chain):
        n = getattr(self, "T", 1)   # (without the family's data the call is refused before it writes)
        value, precision = np.zeros(n), np.zeros(n)
        self._check(self.lib.ba_ss_poisson_get_latent(self._h, int(chain), _p(value), _p(precision)))
        return value, precision

    def ss_poisson_set_latent(self, value, precision, chain=-1):
        self._check(self.lib.ba_ss_poisson_set_latent(self._h, int(chain), _p(_f64(value)), _p(_f64(precision))))

    def ss_poisson_forecast(self, newX, exposure=None):
        """one predictive draw of the next len(newX) counts per chain; exposure: len(newX) numbers
        (default: ones)"""
        h = newX.shape[0]
        out = np.zeros((self.chains, h))
        ex = None if exposure is None else _f64(exposure)
        if ex is not None and ex.shape != (h,):
            raise ValueError("exposure must have one entry per row of newX")
        self._check(self.lib.ba_ss_poisson_forecast(self._h, h, _p(_fcol(newX)), _p(ex), _p(out)))
        return out

    # ---- StateSpaceLogitPosteriorSampler (bsts family = "logit") -------------------
    def ss_logit_set_data(self, successes, trials, X, observed=None, clt_threshold=5):
        T, p = X.shape
        obs = None if observed is None else np.ascontiguousarray(observed, np.uint8)
        self._check(self.lib.ba_ss_logit_set_data(self._h, T, p, _p(_f64(successes)), _p(_f64(trials)),
                                                  _p(_fcol(X)), _b(obs), int(clt_threshold)))
        self.p = p
        self.T = T

    def ss_logit_sweep(self, nsweeps=1, sync=True):
        self._check(self.lib.ba_ss_logit_sweep(self._h, nsweeps))
        if sync:
            self.sync()

    def ss_logit_impute_state(self):
        self._check(self.lib.ba_ss_logit_impute_state(self._h))
        self.sync()

    def ss_logit_get_latent(self, chain):
        n = getattr(self, "T", 1)   # (without the family's data the call is refused before it writes)
        value, precision = np.zeros(n), np.zeros(n)
        self._check(self.lib.ba_ss_logit_get_latent(self._h, int(chain), _p(value), _p(precision)))
        return value, precision

    def ss_logit_set_latent(self, value, precision, chain=-1):
        self._check(self.lib.ba_ss_logit_set_latent(self._h, int(chain), _p(_f64(value)), _p(_f64(precision))))

    def ss_logit_forecast(self, newX, trials=None):
        """one predictive draw of the next len(newX) success counts per chain; trials: len(newX)
        numbers (default: ones)"""
        h = newX.shape[0]
        out = np.zeros((self.chains, h))
        nt = None if trials is None else _f64(trials)
        if nt is not None and nt.shape != (h,):
            raise ValueError("trials must have one entry per row of newX")
        self._check(self.lib.ba_ss_logit_forecast(self._h, h, _p(_fcol(newX)), _p(nt), _p(out)))
        return out

    # ---- QuantileRegressionSpikeSlabSampler --------------------------------------
    def quantile_set_data(self, X, y, quantile):
        X = np.asfortranarray(X, dtype=np.float64)
        self.p = X.shape[1]
        self.n = X.shape[0]
        self._check(self.lib.ba_quantile_set_data(self._h, X.shape[0], X.shape[1], _p(X), _p(_f64(y)),
                                                  float(quantile)))

    def quantile_sweep(self, nsweeps=1, sync=True):
        self._check(self.lib.ba_quantile_sweep(self._h, nsweeps))
        if sync:
            self.sync()

    def quantile_get_weights(self, chain):
        """the last imputation's weights lambda_inv of one chain (0 where the residual was 0)"""
        out = np.zeros(getattr(self, "n", 1))   # (without quantile data the call is refused before it writes)
        self._check(self.lib.ba_quantile_get_weights(self._h, int(chain), _p(out)))
        return out

    # ---- MLVS (multinomial logit spike and slab) -----------------------------------
    def mlogit_set_data(self, y, Xsubject, Xchoice, nchoices):
        """y n in 0 .. nchoices - 1; Xsubject n x psub or None; Xchoice (n nchoices) x pch, row
        i nchoices + m, or None"""
        y = np.ascontiguousarray(y, dtype=np.int32)
        n = y.shape[0]
        xs = None if Xsubject is None else np.asfortranarray(Xsubject, dtype=np.float64)
        xc = None if Xchoice is None else np.asfortranarray(Xchoice, dtype=np.float64)
        psub = 0 if xs is None else xs.shape[1]
        pch = 0 if xc is None else xc.shape[1]
        if xs is not None and xs.shape[0] != n:
            raise ValueError("Xsubject must have one row per observation")
        if xc is not None and xc.shape[0] != n * int(nchoices):
            raise ValueError("Xchoice must have nchoices rows per observation")
        self._check(self.lib.ba_mlogit_set_data(self._h, n, int(nchoices), psub, pch,
                                                y.ctypes.data_as(C.POINTER(C.c_int32)),
                                                None if xs is None else _p(xs), None if xc is None else _p(xc)))
        self.n = n * int(nchoices)
        self.p = (int(nchoices) - 1) * psub + pch

    def mlogit_set_flip_order(self, order):
        o = np.ascontiguousarray(order, dtype=np.int32)
        if o.ndim != 1:
            raise ValueError("the flip order is a vector, one entry per coefficient")
        self._check(self.lib.ba_mlogit_set_flip_order(self._h, o.ctypes.data_as(C.POINTER(C.c_int32))))

    def mlogit_allow_model_selection(self, allow=True):
        self._check(self.lib.ba_mlogit_allow_model_selection(self._h, 1 if allow else 0))

    def mlogit_sweep(self, nsweeps=1, sync=True):
        self._check(self.lib.ba_mlogit_sweep(self._h, nsweeps))
        if sync:
            self.sync()

    def mlogit_get_latent(self, chain):
        """(u, w) of the last imputation of one chain, n nchoices each, row i nchoices + m"""
        N = getattr(self, "n", 1)   # (without multinomial logit data the call is refused before it writes)
        u, w = np.zeros(N), np.zeros(N)
        self._check(self.lib.ba_mlogit_get_latent(self._h, int(chain), _p(u), _p(w)))
        return u, w

    def mlogit_get_wss(self, chain):
        out = np.zeros(1)
        self._check(self.lib.ba_mlogit_get_wss(self._h, int(chain), _p(out)))
        return float(out[0])

    def logit_set_imputer(self, kind):
        """0: the reference's auxiliary mixture (default); 1: Polya-Gamma"""
        self._check(self.lib.ba_logit_set_imputer(self._h, int(kind)))

    def logit_sweep(self, nsweeps=1, sync=True):
        self._check(self.lib.ba_logit_sweep(self._h, nsweeps))
        if sync:
            self.sync()

    def ss_set_structural(self, trend, nseasons, var_df, var_sigma_guess,
                          var_sigma_upper_limit, var_initial_sigma, initial_state_mean,
                          initial_state_variance):
        """trend (1 local level, 2 local linear trend) + optional seasonal state"""
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in
                (var_df, var_sigma_guess, var_sigma_upper_limit, var_initial_sigma,
                 initial_state_mean, initial_state_variance)]
        self._ssm_dim = int(trend) + (int(nseasons) - 1 if nseasons > 0 else 0)
        self._ar_lags = 0
        self._check(self.lib.ba_ss_set_structural(self._h, int(trend), int(nseasons),
                                                  *[_p(a) for a in arrs]))

    def ss_add_ar(self, lags, df, sigma_guess, sigma_upper_limit, initial_sigma, initial_phi,
                  initial_state_mean, initial_state_variance):
        """appends an ArStateModel(lags) block (+ ArPosteriorSampler) to the structural state"""
        ph = (None if initial_phi is None
              else np.ascontiguousarray(initial_phi, dtype=np.float64))
        a0 = np.ascontiguousarray(initial_state_mean, dtype=np.float64)
        p0 = np.ascontiguousarray(initial_state_variance, dtype=np.float64)
        if a0.shape != (lags,) or p0.shape != (lags,) or (ph is not None and ph.shape != (lags,)):
            raise ValueError("the block's initial moments and coefficients have `lags` entries")
        self._check(self.lib.ba_ss_add_ar(self._h, int(lags), float(df), float(sigma_guess),
                                          float(sigma_upper_limit), float(initial_sigma),
                                          _p(ph) if ph is not None else None, _p(a0), _p(p0)))
        self._ssm_dim += int(lags)
        self._ar_lags = int(lags)

    def ss_get_ar(self, chain):
        L = self._ar_lags
        phi, xtx, xty = np.zeros(L), np.zeros((L, L)), np.zeros(L)
        sig, yty, n = C.c_double(), C.c_double(), C.c_double()
        self._check(self.lib.ba_ss_get_ar(self._h, chain, _p(phi), C.byref(sig), _p(xtx), _p(xty),
                                          C.byref(yty), C.byref(n)))
        return dict(phi=phi, sigsq=sig.value, xtx=xtx, xty=xty, yty=yty.value, n=n.value)

    def ss_set_state_models(self, blocks):
        """a general list of state models, in the order they are added: dicts with kind
        (1 local level, 2 local linear trend, 3 seasonal, 4 autoregression, 5 static intercept,
        6 trig, 7 semilocal linear trend, 8 Student local linear trend: nu_priors = ((kind, a, b) of
        level and slope), initial_nu = (level, slope), 9 spike-and-slab autoregression: lags, initial_phi,
        slab_mean, slab_precision, inclusion_probabilities, truncate, max_flips, allow_model_selection,
        10 random-walk holiday: width and, optionally, calendar -- ss_set_holiday_calendar's positions,
        11 or "calendar_seasonal": nseasons and, optionally, calendar -- ss_set_season_calendar's flags;
        "monthly": the calendar seasonal of 12 seasons that start on the first day of a month, with
        first_date = (year, month, day) of the first observation and, optionally, calendar_length (the
        series' length and any forecast horizon; default: the series' length + 366);
        "dynamic_regression": predictors (rows x d, row t = x_t; rows past the series serve forecasts) and
        d entries each of df, sigma_guess, sigma_upper_limit, initial_sigma, a0, P0 -- it goes through
        ba_ss_add_dynamic_regression, a numeric kind 12 to ba_ss_add_state_model, which refuses it;
        "dynamic_regression_ar": predictors (rows x d) and lags -- every coefficient an autoregression of that
        many lags --, d entries each of df, sigma_guess, sigma_upper_limit, initial_sigma, and d x lags each of
        a0, P0 (default 0 and 1, bsts's) and initial_phi (default zeros): d state models of the list, one per
        coefficient, through ba_ss_add_dynamic_regression_ar;
        "regression_holiday": widths (one per holiday), prior = (mean, sd) and, optionally, calendar --
        ss_set_regression_holiday_calendar's flat indices -- and coefficients (the initial ones): no block of
        the list, ss_add_regression_holiday numbers such models on their own;
        "hierarchical_regression_holiday": nholidays, width, mean_prior = (mean, variance), variance_prior =
        (variance_guess, variance_guess_weight) and, optionally, calendar and coefficients as the plain model's --
        one of the list's regression holiday models, through ss_add_hierarchical_regression_holiday), nseasons, duration, t0, lags, df, sigma_guess, sigma_upper_limit, initial_sigma
        (one entry per variance parameter; none for kind 5), initial_phi, rotations (kind 6: the
        (cos, sin) pairs of the transition matrix), a0, P0 (tests/cases.py: general_spec)"""
        self._check(self.lib.ba_ss_clear_state_models(self._h))
        self._blocks = []
        self._rh_ncoef = []
        self._rhh_width = {}
        for b in blocks:
            if b["kind"] == "regression_holiday":
                model = self.ss_add_regression_holiday(b["widths"], b["prior"][0], b["prior"][1], b.get("coefficients"))
                if b.get("calendar") is not None:
                    self.ss_set_regression_holiday_calendar(model, b["calendar"])
                continue
            if b["kind"] == "hierarchical_regression_holiday":
                model = self.ss_add_hierarchical_regression_holiday(b["nholidays"], b["width"], b["mean_prior"][0], b["mean_prior"][1],
                                                                    b["variance_prior"][0], b["variance_prior"][1], b.get("coefficients"))
                if b.get("calendar") is not None:
                    self.ss_set_regression_holiday_calendar(model, b["calendar"])
                continue
            if b["kind"] == "monthly":
                n = int(b.get("calendar_length", self.T + 366))
                b = dict(b, kind=11, nseasons=12, calendar=monthly_cycle_calendar(*b["first_date"], n))
            elif b["kind"] == "calendar_seasonal":
                b = dict(b, kind=11)
            elif b["kind"] == "dynamic_regression":
                x = np.ascontiguousarray(b["predictors"], dtype=np.float64)
                if x.ndim != 2:
                    raise ValueError("predictors: a rows x d array")
                arrs = [np.ascontiguousarray(b[k], dtype=np.float64) for k in
                        ("df", "sigma_guess", "sigma_upper_limit", "initial_sigma", "a0", "P0")]
                if any(a.size != x.shape[1] for a in arrs):
                    raise ValueError("a dynamic regression takes one entry per predictor of df, sigma_guess, "
                                     "sigma_upper_limit, initial_sigma, a0 and P0")
                self._check(self.lib.ba_ss_add_dynamic_regression(self._h, x.shape[1], _p(x), x.shape[0],
                                                                  *[_p(a) for a in arrs]))
                self._blocks.append(dict(kind="dynamic_regression", nvar=x.shape[1], lags=0))
                continue
            elif b["kind"] == "dynamic_regression_ar":
                x = np.ascontiguousarray(b["predictors"], dtype=np.float64)
                if x.ndim != 2:
                    raise ValueError("predictors: a rows x d array")
                d, L = x.shape[1], int(b["lags"])
                arrs = [np.ascontiguousarray(b[k], dtype=np.float64) for k in
                        ("df", "sigma_guess", "sigma_upper_limit", "initial_sigma")]
                if any(a.size != d for a in arrs):
                    raise ValueError("an AR dynamic regression takes one entry per predictor of df, sigma_guess, "
                                     "sigma_upper_limit and initial_sigma")
                n = d * max(L, 0)
                a0 = np.ascontiguousarray(b.get("a0", np.zeros(n)), dtype=np.float64).ravel()
                p0 = np.ascontiguousarray(b.get("P0", np.ones(n)), dtype=np.float64).ravel()
                ph = None if b.get("initial_phi") is None else np.ascontiguousarray(b["initial_phi"], dtype=np.float64).ravel()
                if a0.size != n or p0.size != n or (ph is not None and ph.size != n):
                    raise ValueError("an AR dynamic regression takes d x lags entries of a0, P0 and initial_phi")
                first = C.c_int32()
                self._check(self.lib.ba_ss_add_dynamic_regression_ar(self._h, d, L, _p(x), x.shape[0], *[_p(a) for a in arrs],
                                                                     None if ph is None else _p(ph), _p(a0), _p(p0), C.byref(first)))
                assert first.value == len(self._blocks)
                self._blocks += [dict(kind="dynamic_regression_ar", nvar=1, lags=L, xcols=d) for _ in range(d)]
                continue
            kind = int(b["kind"])
            ip = np.zeros(4, np.int32)
            if kind == 11:
                ip[0] = b["nseasons"]
            elif kind == 3:
                ip[:3] = (b["nseasons"], b["duration"], b.get("t0", 0))
            elif kind == 4:
                ip[0] = b["lags"]
            elif kind == 9:
                ip[:] = (b["lags"], int(b.get("truncate", 1)), int(b.get("max_flips", -1)),
                         int(b.get("allow_model_selection", 1)))
                L = int(b["lags"])
                b = dict(b, initial_phi=np.concatenate([
                    np.asarray(b.get("initial_phi", np.zeros(L)), dtype=np.float64).ravel(),
                    np.asarray(b["slab_mean"], dtype=np.float64).ravel(),
                    np.asarray(b["inclusion_probabilities"], dtype=np.float64).ravel(),
                    np.asarray(b["slab_precision"], dtype=np.float64).ravel(order="F")]))
            elif kind == 6:
                ip[0] = len(b["rotations"]) // 2
            elif kind == 10:
                ip[0] = b["width"]
            elif kind == 7:
                ip[0], ip[1] = int(b.get("force_stationary", 1)), int(b.get("force_positive", 0))
            arrs = [np.ascontiguousarray(b[k], dtype=np.float64) for k in
                    ("df", "sigma_guess", "sigma_upper_limit", "initial_sigma")]
            if kind == 8 and "nu_priors" in b and "initial_nu" in b:   # (without them: the engine's "null argument")
                b = dict(b, initial_phi=np.concatenate([np.ravel(np.asarray(b["nu_priors"], dtype=np.float64)),
                                                        np.asarray(b["initial_nu"], dtype=np.float64)]))
            ph = np.ascontiguousarray(b["rotations"] if kind == 6 else
                                      (b["slope_priors"] if kind == 7 else b.get("initial_phi", np.zeros(0))),
                                      dtype=np.float64)
            a0 = np.ascontiguousarray(b["a0"], dtype=np.float64)
            p0 = np.ascontiguousarray(b["P0"], dtype=np.float64)
            self._check(self.lib.ba_ss_add_state_model(
                self._h, kind, ip.ctypes.data_as(C.POINTER(C.c_int32)),
                *[(_p(a) if a.size else None) for a in arrs],
                _p(ph) if (kind in (4, 6, 7, 8, 9) and ph.size) else None, _p(a0), _p(p0)))
            self._blocks.append(dict(kind=kind, nvar=2 if kind in (2, 7, 8) else (0 if kind == 5 else 1),
                                     lags=int(ip[0]) if kind in (4, 9) else 0))
            if kind == 10 and b.get("calendar") is not None:
                self.ss_set_holiday_calendar(len(self._blocks) - 1, b["calendar"])
            if kind == 11 and b.get("calendar") is not None:
                self.ss_set_season_calendar(len(self._blocks) - 1, b["calendar"])
        m, nb = C.c_int32(), C.c_int32()
        self._check(self.lib.ba_ss_state_dimension(self._h, C.byref(m), C.byref(nb)))
        self._ssm_dim = m.value
        self._ar_lags = 0

    def set_slot_limit(self, uniforms):
        """tests: a substream slot hands out `uniforms` numbers, then its spill stream (0: default)"""
        self._check(self.lib.ba_set_slot_limit(self._h, int(uniforms)))

    def ss_set_tuning(self, use_template_kernel=True, kernel=None):
        """kernel: 0 general, 1 the default choice,
        3 compiled for the shape (where it applies); 4 / 5: the local-level rounds as separate
        launches / as the persistent round kernel (the default)"""
        if kernel is None:
            kernel = 1 if use_template_kernel else 0
        self._check(self.lib.ba_ss_set_tuning(self._h, int(kernel)))

    def ss_get_state_model(self, chain, block, suf=True):
        """suf=False: the variance parameters / coefficients only"""
        b = self._blocks[block]
        nv, L = b["nvar"], b["lags"]
        var, n, ss = np.zeros(nv), np.zeros(nv), np.zeros(nv)
        out = dict(variances=var, suf_n=n, suf_ss=ss)
        if b["kind"] == 7:
            # a semilocal linear trend: (phi, mu) of the slope model; its Ar1Suf (sumsq, sum, cross,
            # n, first, last) with suf=True
            phi, a1 = np.zeros(2), np.zeros(6)
            self._check(self.lib.ba_ss_get_state_model(self._h, chain, block, _p(var), _p(n) if suf else None,
                                                       _p(ss) if suf else None, _p(phi), _p(a1) if suf else None,
                                                       None, None, None))
            out["phi"] = phi
            if suf:
                out["ar1_suf"] = a1
            return out
        if b["kind"] == 8:
            # a Student local linear trend: phi = (nu_level, nu_slope)
            nu = np.zeros(2)
            self._check(self.lib.ba_ss_get_state_model(self._h, chain, block, _p(var), _p(n) if suf else None,
                                                       _p(ss) if suf else None, _p(nu), None, None, None, None))
            out["nu"] = nu
            return out
        if not suf:
            phi = np.zeros(L) if L else None
            self._check(self.lib.ba_ss_get_state_model(self._h, chain, block, _p(var), None, None,
                                                       _p(phi), None, None, None, None))
            if L:
                out["phi"] = phi
            return out
        if L:
            phi, xtx, xty = np.zeros(L), np.zeros((L, L)), np.zeros(L)
            yty, an = C.c_double(), C.c_double()
            self._check(self.lib.ba_ss_get_state_model(
                self._h, chain, block, _p(var), _p(n), _p(ss), _p(phi), _p(xtx), _p(xty),
                C.cast(C.byref(yty), _dp), C.cast(C.byref(an), _dp)))
            out.update(phi=phi, xtx=xtx, xty=xty, yty=yty.value, n=an.value)
        else:
            self._check(self.lib.ba_ss_get_state_model(self._h, chain, block, _p(var), _p(n), _p(ss),
                                                       None, None, None, None, None))
        return out

    def ss_get_state_draw(self, chain):
        st = np.zeros((self.T, self._ssm_dim))
        self._check(self.lib.ba_ss_get_state_draw(self._h, chain, _p(st)))
        return st

    def ss_get_structural(self, chain):
        st = np.zeros((self.T, self._ssm_dim))
        var, n, ss = np.zeros(3), np.zeros(3), np.zeros(3)
        self._check(self.lib.ba_ss_get_structural(self._h, chain, _p(st), _p(var), _p(n), _p(ss)))
        return dict(state=st, variances=var, suf_n=n, suf_ss=ss)

    def ss_sweep(self, nsweeps=1, sync=True):
        self._check(self.lib.ba_ss_sweep(self._h, nsweeps))
        if sync:
            self.sync()

    def ss_set_lookahead(self, lookahead, chains=None):
        """ba_ss_draw_next enqueues `lookahead` rounds at a time; chains: whose state path
        is recorded (default: chain 0)"""
        if chains is not None:
            arr = np.ascontiguousarray(chains, dtype=np.int64)
            self._check(self.lib.ba_ss_lookahead_chains(self._h, len(arr),
                                                        arr.ctypes.data_as(C.POINTER(C.c_int64))))
        self._check(self.lib.ba_ss_set_lookahead(self._h, int(lookahead)))

    def ss_draw_next(self):
        self._check(self.lib.ba_ss_draw_next(self._h))

    def ss_impute_state(self):
        self._check(self.lib.ba_ss_impute_state(self._h))
        self.sync()

    def ss_trend_get_weights(self, chain):
        """the Student local linear trend's weights of one chain: (level, slope), T each"""
        lw, sw = np.zeros(self.T), np.zeros(self.T)
        self._check(self.lib.ba_ss_trend_get_weights(self._h, chain, _p(lw), _p(sw)))
        return lw, sw

    def ss_trend_set_weights(self, level_w, slope_w, chain=-1):
        lw = np.ascontiguousarray(level_w, dtype=np.float64)
        sw = np.ascontiguousarray(slope_w, dtype=np.float64)
        if lw.shape != (self.T,) or sw.shape != (self.T,):
            raise ValueError("the weights have T entries each")
        self._check(self.lib.ba_ss_trend_set_weights(self._h, chain, _p(lw), _p(sw)))

    def ss_trend_get_weight_suf(self, chain):
        """(n, sum w, sum log w) of the level weights, then of the slope weights"""
        out = np.zeros(6)
        self._check(self.lib.ba_ss_trend_get_weight_suf(self._h, chain, _p(out)))
        return out

    def ss_trend_draw_parameters(self):
        """the Student local linear trend's sample_posterior() alone, every chain"""
        self._check(self.lib.ba_ss_trend_draw_parameters(self._h))
        self.sync()

    def ss_autoar_draw_parameters(self):
        """the ArSpikeSlabSampler::draw() of every spike-and-slab autoregression alone, every chain"""
        self._check(self.lib.ba_ss_autoar_draw_parameters(self._h))
        self.sync()

    def ss_get_ar_inclusion(self, chain, block):
        """the inclusion indicators of a spike-and-slab autoregression (state model `block`) in one chain"""
        g = np.zeros(max(self._blocks[block]["lags"], 1), np.uint8)
        self._check(self.lib.ba_ss_get_ar_inclusion(self._h, chain, block, g.ctypes.data_as(C.POINTER(C.c_uint8))))
        return g[:self._blocks[block]["lags"]]

    def ss_set_holiday_calendar(self, block, positions):
        """a random-walk holiday's calendar (state model `block`): entry t is -1 (inactive) or the
        position of time t in the holiday's window, in [0, width); at least T entries, those past T
        serve forecasts"""
        pos = np.ascontiguousarray(positions, dtype=np.int32)
        self._check(self.lib.ba_ss_set_holiday_calendar(self._h, block, pos.ctypes.data_as(C.POINTER(C.c_int32)),
                                                        pos.size))

    def ss_add_regression_holiday(self, widths, prior_mean, prior_sd, coefficients=None):
        """a regression holiday model on the list of state models (at least one state model first): one
        coefficient per day of each holiday's window, all N(prior_mean, prior_sd^2); returns its index
        among the list's regression holiday models"""
        w = np.ascontiguousarray(widths, dtype=np.int32)
        c = None if coefficients is None else np.ascontiguousarray(coefficients, dtype=np.float64)
        if c is not None and c.size != int(w.sum()):
            raise ValueError("coefficients: one per day of every holiday's window")
        model = C.c_int32()
        self._check(self.lib.ba_ss_add_regression_holiday(self._h, w.size, w.ctypes.data_as(C.POINTER(C.c_int32)),
                                                          float(prior_mean), float(prior_sd),
                                                          None if c is None else _p(c), C.byref(model)))
        if not hasattr(self, "_rh_ncoef"):
            self._rh_ncoef = []
        del self._rh_ncoef[model.value:]
        self._rh_ncoef.append(int(w.sum()))
        return model.value

    def ss_add_hierarchical_regression_holiday(self, nholidays, width, mean_prior_mean, mean_prior_variance, variance_guess,
                                               variance_guess_weight, coefficients=None):
        """a hierarchical regression holiday model on the list of state models: nholidays holidays of one width d,
        their coefficient vectors N(mu, Omega^-1) with mu ~ N(mean_prior_mean, mean_prior_variance) and
        Omega ~ Wishart(variance_guess_weight, variance_guess_weight x variance_guess); returns its index among the
        list's regression holiday models (the calendar and the coefficients go through the plain model's calls)"""
        d = int(width)
        m0 = np.ascontiguousarray(mean_prior_mean, dtype=np.float64).reshape(-1)
        v0 = np.ascontiguousarray(mean_prior_variance, dtype=np.float64).reshape(-1)
        g = np.ascontiguousarray(variance_guess, dtype=np.float64).reshape(-1)
        if d >= 1 and (m0.size != d or v0.size != d * d or g.size != d * d):
            raise ValueError("mean_prior_mean: width entries; mean_prior_variance, variance_guess: width x width")
        c = None if coefficients is None else np.ascontiguousarray(coefficients, dtype=np.float64).reshape(-1)
        if c is not None and c.size != int(nholidays) * d:
            raise ValueError("coefficients: one per day of every holiday's window")
        model = C.c_int32()
        self._check(self.lib.ba_ss_add_hierarchical_regression_holiday(self._h, int(nholidays), d, _p(m0), _p(v0), _p(g),
                                                                       float(variance_guess_weight),
                                                                       None if c is None else _p(c), C.byref(model)))
        if not hasattr(self, "_rh_ncoef"):
            self._rh_ncoef = []
        del self._rh_ncoef[model.value:]
        self._rh_ncoef.append(int(nholidays) * d)
        if not hasattr(self, "_rhh_width"):
            self._rhh_width = {}
        self._rhh_width[model.value] = d
        return model.value

    def ss_get_hierarchical_regression_holiday(self, chain, model):
        """one chain's hyper-mean and hyper-precision of a hierarchical regression holiday model"""
        d = getattr(self, "_rhh_width", {}).get(model, 1)
        mean, prec = np.zeros(d), np.zeros((d, d))
        self._check(self.lib.ba_ss_get_hierarchical_regression_holiday(self._h, chain, model, _p(mean), _p(prec)))
        return dict(mean=mean, precision=prec)

    def ss_set_hierarchical_regression_holiday(self, chain, model, mean, precision):
        """the hyper-mean and hyper-precision of one chain, or of every chain (chain = -1)"""
        d = getattr(self, "_rhh_width", {}).get(model, 1)
        m = np.ascontiguousarray(mean, dtype=np.float64).reshape(-1)
        q = np.ascontiguousarray(precision, dtype=np.float64).reshape(-1)
        if m.size != d or q.size != d * d:
            raise ValueError("mean: width entries; precision: width x width")
        self._check(self.lib.ba_ss_set_hierarchical_regression_holiday(self._h, chain, model, _p(m), _p(q)))

    def ss_set_regression_holiday_calendar(self, model, index):
        """a regression holiday model's calendar: entry t is -1 (inactive) or the flat index offset_h + day
        of the coefficient active at time t; at least T entries, those past T serve forecasts"""
        idx = np.ascontiguousarray(index, dtype=np.int32)
        self._check(self.lib.ba_ss_set_regression_holiday_calendar(self._h, model, idx.ctypes.data_as(C.POINTER(C.c_int32)),
                                                                   idx.size))

    def ss_get_regression_holiday_calendar(self, model):
        n = C.c_int64()
        self._check(self.lib.ba_ss_get_regression_holiday_calendar(self._h, model, None, C.byref(n)))
        idx = np.zeros(max(n.value, 1), np.int32)
        self._check(self.lib.ba_ss_get_regression_holiday_calendar(self._h, model, idx.ctypes.data_as(C.POINTER(C.c_int32)),
                                                                   C.byref(n)))
        return idx[:n.value]

    def ss_get_regression_holiday(self, chain, model):
        """one chain's coefficients of a regression holiday model, the totals of its last observe_state and
        the counts (the same for every chain)"""
        n = self._rh_ncoef[model] if 0 <= model < len(getattr(self, "_rh_ncoef", [])) else 1
        coef, tot, cnt = np.zeros(n), np.zeros(n), np.zeros(n)
        self._check(self.lib.ba_ss_get_regression_holiday(self._h, chain, model, _p(coef), _p(tot), _p(cnt)))
        return dict(coefficients=coef, totals=tot, counts=cnt)

    def ss_set_regression_holiday(self, chain, model, coefficients):
        """the coefficients of one chain, or of every chain (chain = -1)"""
        c = np.ascontiguousarray(coefficients, dtype=np.float64)
        if not (0 <= model < len(getattr(self, "_rh_ncoef", []))) or c.size != self._rh_ncoef[model]:
            raise ValueError("coefficients: one per day of every holiday's window of the model")
        self._check(self.lib.ba_ss_set_regression_holiday(self._h, chain, model, _p(c)))

    def ss_set_dynamic_predictors(self, block, predictors):
        """a dynamic regression's predictors (state model `block`), rows x d: replaced, or extended with the
        rows a forecast needs (at least T rows; T + horizon for ss_forecast).  An AR dynamic regression: all
        its d columns, on the model's first block"""
        x = np.ascontiguousarray(predictors, dtype=np.float64)
        if x.ndim != 2 or x.shape[1] != self._blocks[block].get("xcols", self._blocks[block]["nvar"]):
            raise ValueError("predictors: a rows x d array")
        self._check(self.lib.ba_ss_set_dynamic_predictors(self._h, block, _p(x), x.shape[0]))

    def ss_get_dynamic_predictors(self, block):
        n = C.c_int64()
        self._check(self.lib.ba_ss_get_dynamic_predictors(self._h, block, None, C.byref(n)))
        d = self._blocks[block].get("xcols", self._blocks[block]["nvar"])
        x = np.zeros((max(n.value, 1), d))
        self._check(self.lib.ba_ss_get_dynamic_predictors(self._h, block, _p(x), C.byref(n)))
        return x[:n.value]

    def ss_get_holiday_calendar(self, block):
        n = C.c_int64()
        self._check(self.lib.ba_ss_get_holiday_calendar(self._h, block, None, C.byref(n)))
        pos = np.zeros(max(n.value, 1), np.int32)
        self._check(self.lib.ba_ss_get_holiday_calendar(self._h, block, pos.ctypes.data_as(C.POINTER(C.c_int32)),
                                                        C.byref(n)))
        return pos[:n.value]

    def ss_set_season_calendar(self, block, new_season):
        """a calendar seasonal's calendar (state model `block`): entry t is 1 where time t starts a new
        season, else 0; at least T entries, those past T serve forecasts"""
        raw = np.asarray(new_season)
        if raw.size and (raw.min() < 0 or raw.max() > 255):
            raise ValueError("a season calendar's entries must be 0 or 1")
        flags = np.ascontiguousarray(raw, dtype=np.uint8)
        self._check(self.lib.ba_ss_set_season_calendar(self._h, block, flags.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                       flags.size))

    def ss_get_season_calendar(self, block):
        n = C.c_int64()
        self._check(self.lib.ba_ss_get_season_calendar(self._h, block, None, C.byref(n)))
        flags = np.zeros(max(n.value, 1), np.uint8)
        self._check(self.lib.ba_ss_get_season_calendar(self._h, block, flags.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                       C.byref(n)))
        return flags[:n.value]

    def ss_forecast(self, newX):
        """one predictive draw of the next len(newX) observations per chain"""
        h = newX.shape[0]
        out = np.zeros((self.chains, h))
        self._check(self.lib.ba_ss_forecast(self._h, h, _p(_fcol(newX)), _p(out)))
        return out

    def ss_prediction_errors(self, standardize=False, chains=None, variances=False, log_likelihood=False):
        """bsts's one.step.prediction.errors of every chain's current draw (chains: a (first, count)
        pair or a range; None: all): chains x T, row c = chain first + c.  With variances or
        log_likelihood: a dict of errors, variances (F_t, the same shape) and log_likelihood (one per
        chain), the ones asked for"""
        if chains is None:
            first, count = 0, self.chains
        elif isinstance(chains, range):
            if chains.step != 1:
                raise ValueError("chains: a contiguous range")
            first, count = chains.start, len(chains)
        else:
            first, count = (int(v) for v in chains)
        rows = max(count, 0)
        err = np.zeros((rows, self.T))
        var = np.zeros((rows, self.T)) if variances else None
        ll = np.zeros(rows) if log_likelihood else None
        self._check(self.lib.ba_ss_prediction_errors(self._h, first, count, 1 if standardize else 0,
                                                     _p(err), _p(var), _p(ll)))
        if not variances and not log_likelihood:
            return err
        out = dict(errors=err)
        if variances:
            out["variances"] = var
        if log_likelihood:
            out["log_likelihood"] = ll
        return out

    def ss_holdout_prediction_errors(self, newX, newY, standardize=False, chains=None, variances=False):
        """bsts.prediction.errors' holdout part for every chain's current draw: the one-step prediction
        errors of the len(newY) rows (newX: len(newY) x p; None where p = 0) that follow the series, from the
        chain's drawn final state.  chains as in ss_prediction_errors; chains x horizon, or with variances a
        dict of errors and variances (F_i, the same shape)"""
        if chains is None:
            first, count = 0, self.chains
        elif isinstance(chains, range):
            if chains.step != 1:
                raise ValueError("chains: a contiguous range")
            first, count = chains.start, len(chains)
        else:
            first, count = (int(v) for v in chains)
        newY = _f64(newY).ravel()
        h = newY.shape[0]
        nx = None
        if newX is not None and np.size(newX) > 0:
            nx = _fcol(np.asarray(newX, dtype=np.float64).reshape(h, -1))
        rows = max(count, 0)
        err = np.zeros((rows, h))
        var = np.zeros((rows, h)) if variances else None
        self._check(self.lib.ba_ss_holdout_prediction_errors(self._h, first, count, 1 if standardize else 0, h,
                                                             _p(nx), _p(newY), _p(err), _p(var)))
        return dict(errors=err, variances=var) if variances else err

    def ss_get_state(self, chain, state=True, suf=True):
        """state=False / suf=False: do not ask for the state path / the level model's
        sufficient statistics (NULL pointers)"""
        st = np.zeros(self.T) if state else None
        ls, n, ss = C.c_double(), C.c_double(), C.c_double()
        self._check(self.lib.ba_ss_get_state(self._h, chain, _p(st), C.byref(ls),
                                             C.byref(n) if suf else None, C.byref(ss) if suf else None))
        return dict(state=st, level_sigsq=ls.value, level_n=n.value, level_sumsq=ss.value)

    def ss_set_level_sigsq(self, sigsq, chain=-1):
        self._check(self.lib.ba_ss_set_level_sigsq(self._h, chain, sigsq))

    def ss_get_chain_suf(self, chain):
        xty = np.zeros(self.p)
        yty, n = C.c_double(), C.c_double()
        self._check(self.lib.ba_ss_get_chain_suf(self._h, chain, _p(xty), C.byref(yty),
                                                 C.byref(n)))
        return dict(xty=xty, yty=yty.value, n=n.value)


class Group:
    """Several engines behind one handle (ba_group_*): one per entry of `devices`, chains
    sharded by global id; the data build and the summaries are the two collectives."""

    def __init__(self, devices, chains_per_device, seed=8675309):
        self.lib = load_library()
        dv = (C.c_int32 * len(devices))(*devices)
        h = C.c_void_p()
        self._h = None
        rc = self.lib.ba_group_create(dv, len(devices), chains_per_device, seed, C.byref(h))
        if rc != 0:
            raise BoomAmdError(rc, self.lib.ba_group_last_error().decode())
        self._h = h
        self.size = len(devices)
        self.chains_per_device = chains_per_device
        self.p = 0
        self.engines = [Engine(chains_per_device, _borrowed=self.lib.ba_group_engine(h, i))
                        for i in range(self.size)]

    def _check(self, rc):
        if rc != 0:
            raise BoomAmdError(rc, self.lib.ba_group_last_error().decode())

    def close(self):
        if self._h is not None:
            for e in self.engines:
                e.close()
            self.lib.ba_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def call(self, fn):
        """fn(engine) on every engine of the group through ba_group_call (the C-ABI's own
        loop: stops at the first error)"""
        by_handle = {e._h.value: e for e in self.engines}
        err = []

        @C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p)
        def tramp(h, _):
            try:
                fn(by_handle[h])
                return 0
            except BoomAmdError as ex:
                err.append(ex)
                return ex.args[0] if ex.args and isinstance(ex.args[0], int) and ex.args[0] else -1
        rc = self.lib.ba_group_call(self._h, C.cast(tramp, C.c_void_p), None)
        if err:
            raise err[0]
        self._check(rc)

    def ss_sweep(self, nsweeps=1, sync=True):
        self._check(self.lib.ba_group_ss_sweep(self._h, nsweeps))
        if sync:
            self.sync()

    def ss_draw_next(self):
        self._check(self.lib.ba_group_ss_draw_next(self._h))

    def logit_sweep(self, nsweeps=1, sync=True):
        self._check(self.lib.ba_group_logit_sweep(self._h, nsweeps))
        if sync:
            self.sync()

    def locate(self, global_chain):
        e, c = C.c_int32(), C.c_int64()
        self._check(self.lib.ba_group_locate(self._h, global_chain, C.byref(e), C.byref(c)))
        return e.value, c.value

    def build_suf_from_xy(self, X, y):
        n, p = X.shape
        self._check(self.lib.ba_group_build_suf_from_xy(self._h, n, p, _p(_fcol(X)), _p(_f64(y))))
        self.p = p
        for e in self.engines:
            e.p = p

    def set_priors(self, b, ominv, pi, prior_df, sigma_guess, max_model_size=-1,
                   sigma_upper_limit=float("inf")):
        self._check(self.lib.ba_group_set_priors(self._h, _p(_f64(b)), _p(_fcol(ominv)), _p(_f64(pi)),
                                                 int(max_model_size), prior_df, sigma_guess,
                                                 sigma_upper_limit))

    def set_state(self, gamma, beta=None, sigsq=1.0):
        g = np.ascontiguousarray(gamma, dtype=np.uint8)
        bb = None if beta is None else _f64(beta)
        self._check(self.lib.ba_group_set_state(self._h, _b(g), _p(bb), sigsq))

    def sweep(self, nsweeps=1, sync=True):
        self._check(self.lib.ba_group_sweep(self._h, nsweeps))
        if sync:
            self.sync()

    def sync(self):
        self._check(self.lib.ba_group_sync(self._h))

    def reset_summaries(self):
        self._check(self.lib.ba_group_reset_summaries(self._h))

    def get_summaries(self):
        p = self.p
        inc, bs, bs2 = np.zeros(p), np.zeros(p), np.zeros(p)
        sc = np.zeros(SUMMARY_SCALARS)
        blocks = np.zeros((self.size, 3 * p + SUMMARY_SCALARS))
        self._check(self.lib.ba_group_get_summaries(self._h, _p(inc), _p(bs), _p(bs2), _p(sc), _p(blocks)))
        return dict(inclusion_count=inc, beta_sum=bs, beta_sumsq=bs2, sweeps=sc[0], sigsq_sum=sc[1],
                    k_sum=sc[3], accepts=sc[4], proposals=sc[5], min_margin=sc[6], blocks=blocks)
