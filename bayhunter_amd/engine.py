"""ctypes binding of the engine's C ABI (include/bh_engine.h -> bayhunter_amd/libbh_engine.so).

This is the only place Python touches the native library.  There is NO CPU fallback: if the
shared library is missing, or no MI355X/HIP device is usable, creating an `Engine` raises
`EngineError`.  (The CPU restatement under oracle/ is test infrastructure and is never
imported from here.)

Host API  : numpy arrays in, numpy arrays out (the library stages through its own device buffers).
Device API: raw device pointers (`tensor.data_ptr()`), asynchronous on a HIP stream -- what
            bench.py and the multi-GPU chain driver use with torch-owned HBM buffers.
"""
import contextlib
import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libbh_engine.so")

BH_OK, BH_EINVAL, BH_EHIP, BH_ENOMEM, BH_EUNSUPPORTED = 0, -1, -2, -3, -4
HOST, DEVICE = 0, 1
WAVE_LOVE, WAVE_RAYLEIGH = 1, 2
VEL_PHASE, VEL_GROUP = 0, 1
RF_P, RF_SV = 0, 1
LAW_NOCORR, LAW_NOCORR_SCALED, LAW_EXP, LAW_GAUSS = 0, 1, 2, 3
TARGET_SWD, TARGET_RF, TARGET_USER = 0, 1, 2
TARGET_ELLIP = 3                    # BH_TARGET_ELLIP (include/bh_engine_ellip_target.h): a USER target given the ellipticity forward model
SEARCH_REFERENCE, SEARCH_FAST, SEARCH_FAST_RAYLEIGH = 0, 1, 2  # bh_engine_set_swd_search
ARITH_EXACT, ARITH_FAST = 0, 1  # bh_engine_set_swd_arith
SCAN_STEPS, SCAN_COUNTED, SCAN_AUTO = 0, 1, 2  # bh_engine_set_swd_scan
MAX_PERIODS, MAX_LAYERS, MAX_TARGETS = 60, 100, 8

_d = C.POINTER(C.c_double)
_i32 = C.POINTER(C.c_int32)


class EngineError(RuntimeError):
    pass


class SwdLaunch(C.Structure):
    """Mirror of `bh_swd_launch` (include/bh_engine_debug.h)."""
    _fields_ = [("family", C.c_int), ("role", C.c_int), ("key", C.c_int * 6), ("two_classes", C.c_int), ("interleaved", C.c_int),
                ("pair_order", C.c_int), ("restart", C.c_int), ("grid_x", C.c_int), ("fair", C.c_int)]


class TargetDesc(C.Structure):
    """Mirror of `bh_target_desc` (include/bh_engine.h)."""
    _fields_ = [("kind", C.c_int32), ("law", C.c_int32), ("n", C.c_int32),
                ("iwave", C.c_int32), ("igr", C.c_int32), ("mode", C.c_int32), ("flsph", C.c_int32),
                ("waveno", C.c_int32), ("nsamp", C.c_int32),
                ("p_s_per_deg", C.c_double), ("gauss", C.c_double), ("fsamp", C.c_double),
                ("tshift", C.c_double), ("nsv", C.c_double),
                ("x", _d), ("yobs", _d), ("yerr", _d), ("rinv", _d), ("logdet_r", C.c_double)]


BH_MAX_TARGETS = 8
BH_CHAIN_MAXLAYERS = 32
BH_CHAIN_MAXDEPTH = 7


class ChainConfig(C.Structure):
    """bh_chain_config of include/bh_engine.h"""
    _fields_ = [("nt", C.c_int32), ("maxlayers", C.c_int32), ("layermin", C.c_int32), ("layermax", C.c_int32),
                ("iter_burnin", C.c_int32), ("iterations", C.c_int32),
                ("vsmin", C.c_double), ("vsmax", C.c_double), ("zmin", C.c_double), ("zmax", C.c_double),
                ("thickmin", C.c_double), ("lvz", C.c_double), ("hvz", C.c_double),
                ("vpvsmin", C.c_double), ("vpvsmax", C.c_double), ("mantle_vs", C.c_double), ("mantle_vpvs", C.c_double),
                ("acc_lo", C.c_double), ("acc_hi", C.c_double),
                ("noise_lo", C.c_double * (2 * BH_MAX_TARGETS)), ("noise_hi", C.c_double * (2 * BH_MAX_TARGETS)),
                ("seed", C.c_uint64), ("chain_offset", C.c_int64)]


class ChainPrior(C.Structure):
    """bh_chain_prior of include/bh_engine_sites_priors.h: the fields of bh_chain_config that belong to a station"""
    _fields_ = [("layermin", C.c_int32), ("layermax", C.c_int32),
                ("vsmin", C.c_double), ("vsmax", C.c_double), ("zmin", C.c_double), ("zmax", C.c_double),
                ("thickmin", C.c_double), ("lvz", C.c_double), ("hvz", C.c_double),
                ("vpvsmin", C.c_double), ("vpvsmax", C.c_double), ("mantle_vs", C.c_double), ("mantle_vpvs", C.c_double),
                ("acc_lo", C.c_double), ("acc_hi", C.c_double),
                ("noise_lo", C.c_double * (2 * BH_MAX_TARGETS)), ("noise_hi", C.c_double * (2 * BH_MAX_TARGETS))]


CHAIN_STATE_FIELDS = ("n", "vs", "z", "vpvs", "noise", "like", "misfits", "propdist", "proposed", "accepted", "naccepted",
                      "beta", "pn", "move", "valid", "pvs", "pz", "pvpvs", "pnoise", "dvs2", "lay_n", "lay_h", "lay_vp", "lay_vs",
                      "inject", "lay_rho")


class ChainState(C.Structure):
    """bh_chain_state of include/bh_engine.h (all members are device pointers)"""
    _fields_ = [(k, C.c_void_p) for k in CHAIN_STATE_FIELDS]


class ChainRecord(C.Structure):
    """bh_chain_record of include/bh_engine_chain_record.h: the device store of thinned samples (the arrays are device pointers)"""
    _fields_ = [("models", C.c_void_p), ("likes", C.c_void_p), ("vpvs", C.c_void_p), ("misfits", C.c_void_p), ("noise", C.c_void_p),
                ("beta", C.c_void_p), ("rows", C.c_int64), ("thinning", C.c_int64), ("row0", C.c_int64)]


_lib = None


def load_library():
    """dlopen libbh_engine.so once.  torch (when the process uses it) must be imported BEFORE
    the library so that both share one HIP runtime (torch ships its own libamdhip64.so with the
    same SONAME); importing it here first makes the order irrelevant for callers."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EngineError("native engine %s is not built; run `python -c 'import __graft_entry__ as g; "
                          "g.build()'` (or `make -C bayhunter_amd/csrc`)" % LIB_PATH)
    if "torch" not in sys.modules and os.environ.get("BH_NO_TORCH", "0") != "1":
        try:
            import torch  # noqa: F401
        except Exception:  # torch is optional for the plugin path
            pass
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    vp = C.c_void_p
    L.bh_abi_version.restype = C.c_int
    L.bh_engine_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.bh_engine_destroy.argtypes = [vp]
    L.bh_engine_destroy.restype = None
    L.bh_engine_last_error.argtypes = [vp]
    L.bh_engine_last_error.restype = C.c_char_p
    L.bh_engine_stream.argtypes = [vp]
    L.bh_engine_stream.restype = vp
    L.bh_engine_synchronize.argtypes = [vp]
    L.bh_engine_set_instrumentation.argtypes = [vp, C.c_int, C.c_int]
    L.bh_engine_set_swd_group.argtypes = [vp, C.c_int]
    L.bh_engine_set_swd_lookahead.argtypes = [vp, C.c_int]
    L.bh_engine_set_swd_search.argtypes = [vp, C.c_int]
    L.bh_engine_get_swd_search.argtypes = [vp]
    L.bh_engine_set_swd_arith.argtypes = [vp, C.c_int]
    L.bh_engine_last_swd_kernel.argtypes = [vp]
    L.bh_engine_last_swd_launches.argtypes = [vp, C.POINTER(SwdLaunch), C.c_int, C.POINTER(C.c_int)]
    L.bh_engine_last_swd_order.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.bh_engine_last_swd_perm.argtypes = [vp, C.c_int, C.POINTER(C.c_int32), C.c_int]
    L.bh_engine_set_swd_trials.argtypes = [vp, C.c_int]
    L.bh_engine_get_swd_trials.argtypes = [vp]
    L.bh_engine_get_swd_arith.argtypes = [vp]
    L.bh_engine_set_swd_scan.argtypes = [vp, C.c_int]
    L.bh_engine_get_swd_scan.argtypes = [vp]
    L.bh_engine_set_tuning.argtypes = [vp, C.c_char_p, C.c_int]
    L.bh_engine_get_tuning.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int)]
    L.bh_engine_guard_stats.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.bh_engine_set_typical_layers.argtypes = [vp, C.c_int]
    L.bh_engine_set_model_order.argtypes = [vp, C.c_int]
    L.bh_timing_reset.argtypes = [vp]
    L.bh_timing_collect.argtypes = [vp, C.POINTER(C.c_int), _d, _d]
    L.bh_timing_steps.argtypes = [vp, C.c_int, _d, C.POINTER(C.c_int)]
    L.bh_last_neval.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.bh_debug_counters.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.bh_debug_guard_list.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int)]
    L.bh_debug_trace.argtypes = [vp, C.POINTER(C.c_uint64), C.c_int]
    L.bh_swd_batch.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_ssize_t,
                               C.c_ssize_t, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]
    L.bh_rf_batch.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp,
                              C.c_ssize_t, C.c_ssize_t, C.c_double, C.c_double, C.c_int, C.c_double,
                              C.c_double, C.c_double, C.c_int, C.c_int, vp]
    L.bh_targets_set.argtypes = [vp, C.c_int, C.POINTER(TargetDesc)]
    L.bh_evaluate_batch.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp,
                                    C.c_ssize_t, C.c_ssize_t, vp, vp, vp, vp, vp]
    L.bh_loglike_batch.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    L.bh_probe_math.argtypes = [vp, C.c_int, C.c_int, _d, _d]
    L.bh_probe_swd_secular.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, _d, _d, _d]
    L.bh_sites_set.argtypes = [vp, C.c_int, vp, vp]
    L.bh_sites_set_rf.argtypes = [vp, C.c_int, vp, vp]
    L.bh_sites_set_x.argtypes = [vp, C.c_int, vp, vp, vp, vp]
    L.bh_sites_set_x_all.argtypes = [vp, C.c_int, vp, vp, vp, vp]
    L.bh_sites_set_missing.argtypes = [vp, C.c_int, vp, vp, vp, vp]
    L.bh_sites_set_missing_gauss.argtypes = [vp, C.c_int, vp, vp, vp, vp]
    L.bh_sites_set_gauss.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    L.bh_sites_set_axes.argtypes = [vp, C.c_int, vp, vp, vp, vp]
    L.bh_sites_set_rf_axis.argtypes = [vp, C.c_int, vp, vp, vp, vp]
    L.bh_sites_set_laws.argtypes = [vp, C.c_int, vp, vp]
    L.bh_chain_propose_sites.argtypes = [vp, C.POINTER(ChainConfig), C.POINTER(ChainState), C.c_int, C.c_int, vp]
    L.bh_chain_propose_window_sites.argtypes = [vp, C.POINTER(ChainConfig), C.POINTER(ChainState), C.c_int, C.c_int, C.c_int, C.c_ssize_t, vp]
    _cc, _cs, _cp = C.POINTER(ChainConfig), C.POINTER(ChainState), C.c_void_p   # (the table of records is a device pointer)
    L.bh_chain_propose_priors.argtypes = [vp, _cc, _cs, C.c_int, C.c_int, _cp, C.c_int, vp, vp]
    L.bh_chain_propose_window_priors.argtypes = [vp, _cc, _cs, C.c_int, C.c_int, C.c_int, C.c_ssize_t, _cp, C.c_int, vp, vp]
    L.bh_chain_accept_priors.argtypes = [vp, _cc, _cs, C.c_int, C.c_int, vp, vp, _cp, C.c_int, vp]
    L.bh_chain_accept_window_priors.argtypes = [vp, _cc, _cs, C.c_int, C.c_int, C.c_int, C.c_ssize_t, vp, vp, _cp, C.c_int, vp]
    _cr = C.POINTER(ChainRecord)
    L.bh_chain_accept_window_record.argtypes = [vp, _cc, _cs, C.c_int, C.c_int, C.c_int, C.c_ssize_t, vp, vp, _cr]
    L.bh_chain_accept_window_priors_record.argtypes = [vp, _cc, _cs, C.c_int, C.c_int, C.c_int, C.c_ssize_t, vp, vp, _cp, C.c_int, vp, _cr]
    L.bh_evaluate_sites.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp,
                                    C.c_ssize_t, C.c_ssize_t, vp, vp, vp, vp, vp, vp]
    L.bh_chain_propose.argtypes = [vp, C.POINTER(ChainConfig), C.POINTER(ChainState), C.c_int, C.c_int]
    L.bh_chain_accept.argtypes = [vp, C.POINTER(ChainConfig), C.POINTER(ChainState), C.c_int, C.c_int, vp, vp]
    L.bh_chain_propose_window.argtypes = [vp, C.POINTER(ChainConfig), C.POINTER(ChainState), C.c_int, C.c_int, C.c_int, C.c_ssize_t]
    L.bh_chain_accept_window.argtypes = [vp, C.POINTER(ChainConfig), C.POINTER(ChainState), C.c_int, C.c_int, C.c_int, C.c_ssize_t, vp, vp]
    L.bh_posterior_create.argtypes = [vp, C.POINTER(vp)]
    L.bh_posterior_destroy.argtypes = [vp]
    L.bh_posterior_destroy.restype = None
    L.bh_posterior_load.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int64, C.c_int, C.c_int64, vp, vp, C.c_int, vp, vp, vp]
    L.bh_posterior_columns.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.bh_posterior_hist.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp]
    L.bh_posterior_interfaces.argtypes = [vp, C.c_int, vp, vp]
    for name in ("bh_posterior_create", "bh_posterior_load", "bh_posterior_columns", "bh_posterior_hist", "bh_posterior_interfaces"):
        getattr(L, name).restype = C.c_int
    L.bh_posterior_keep_rows.argtypes = [vp, C.c_int]
    L.bh_posterior_moho.argtypes = [vp, vp, vp, vp, vp]
    L.bh_posterior_attach.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int64, vp, C.c_int]
    L.bh_posterior_scalar_cols.argtypes = [vp, C.c_int, vp]
    L.bh_posterior_scalar_stats.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.bh_posterior_scalar_hist.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp]
    L.bh_posterior_scalar_hist2d.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
    for name in POSTERIOR_SCALARS_SYMBOLS:
        getattr(L, name).restype = C.c_int
    L.bh_posterior_layers.argtypes = [vp, C.c_int64, C.c_int64, C.c_int, vp, C.c_int, C.c_int64, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int64, vp]
    L.bh_posterior_best.argtypes = [vp, C.c_int, C.c_int, vp, vp, C.c_int64, C.c_int, vp, C.c_int64, vp, vp]
    L.bh_posterior_data_fill.argtypes = [vp, vp, C.c_int64, C.c_int64, C.c_int, vp, vp, C.c_int, vp, vp]
    L.bh_posterior_scalar_quantiles.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp]
    L.bh_posterior_scalar_gather.argtypes = [vp, C.c_int, C.c_int64, vp, vp]
    for name in POSTERIOR_DATAFIT_SYMBOLS:
        getattr(L, name).restype = C.c_int
    L.bh_posterior_column_quantiles.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp, vp, vp]
    for name in POSTERIOR_QUANTILES_SYMBOLS:
        getattr(L, name).restype = C.c_int
    L.bh_posterior_cov.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.bh_posterior_cov_finish.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    for name in POSTERIOR_COV_SYMBOLS:
        getattr(L, name).restype = C.c_int
    L.bh_posterior_features.argtypes = [vp, C.c_int, vp, vp, vp]
    for name in POSTERIOR_FEATURES_SYMBOLS:
        getattr(L, name).restype = C.c_int
    L.bh_posterior_classes.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp]
    L.bh_posterior_scalar_export.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int64, vp]
    for name in POSTERIOR_CLASSES_SYMBOLS:
        getattr(L, name).restype = C.c_int
    L.bh_posterior_resid_fill.argtypes = [vp, vp, C.c_int64, C.c_int64, C.c_int, vp, vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, C.c_int,
                                          C.c_int64, vp, vp]
    for name in POSTERIOR_RESID_SYMBOLS:
        getattr(L, name).restype = C.c_int
    L.bh_chain_diag_series.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_int64, vp, C.c_int,
                                       vp, vp, vp, vp, vp, vp, vp]
    L.bh_chain_diag_models.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_int64, vp, C.c_int, vp,
                                       C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.bh_chain_diag_medians.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int64, C.c_int, C.c_int64, C.c_int64, vp, vp, vp]
    for name in CHAIN_DIAG_SYMBOLS:
        getattr(L, name).restype = C.c_int
    L.bh_chain_ladder_index.argtypes = [vp, C.c_int, vp, C.c_int64, C.c_int, C.c_int64, vp, vp, C.c_int, C.c_int, vp, C.c_int64, vp,
                                        C.c_int64, vp, vp, vp]
    L.bh_chain_diag_series_sel.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_int64, vp,
                                           C.c_int, vp, C.c_int64, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.bh_chain_diag_models_sel.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_int64, vp,
                                           C.c_int, vp, C.c_int64, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.bh_chain_diag_medians_sel.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int64, C.c_int, C.c_int64, C.c_int64, vp, C.c_int, vp,
                                            C.c_int64, vp, vp]
    for name in CHAIN_LADDER_SYMBOLS:
        getattr(L, name).restype = C.c_int
    L.bh_chain_ladder_holders.argtypes = [vp, C.c_int, vp, C.c_int64, C.c_int, C.c_int64, vp, vp, C.c_int, C.c_int, vp, C.c_int64, vp]
    L.bh_chain_ladder_evidence.argtypes = [vp, C.c_int, vp, C.c_int64, C.c_int, C.c_int64, vp, C.c_int, C.c_int64, C.c_int64, vp, vp,
                                           C.c_int, C.c_int, vp, C.c_int64, vp, vp, vp, vp, vp, vp, vp]
    for name in CHAIN_LADDER_EVIDENCE_SYMBOLS:
        getattr(L, name).restype = C.c_int
    L.bh_ladder_sweep_create.argtypes = [vp, C.c_int, vp, C.c_int, C.POINTER(vp)]
    L.bh_ladder_sweep_run.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_double]
    L.bh_ladder_sweep_read.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.bh_ladder_sweep_destroy.argtypes = [vp, vp]
    for name in LADDER_SWEEP_SYMBOLS:
        getattr(L, name).restype = C.c_int
    L.bh_chain_rank_series.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_int64, vp, C.c_int, vp,
                                       vp, vp, vp, vp, vp, C.c_int64, C.c_int64]
    L.bh_chain_rank_models.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_int64, vp, C.c_int, vp,
                                       C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int64, C.c_int64]
    for name in CHAIN_RANK_SYMBOLS:
        getattr(L, name).restype = C.c_int
    L.bh_chain_diag_features.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_int64, vp, C.c_int, vp,
                                         C.c_int64, C.c_int, vp, C.c_int, vp, vp, vp, vp, C.c_int64, C.c_int64, vp]
    for name in CHAIN_DIAG_FEATURES_SYMBOLS:
        getattr(L, name).restype = C.c_int
    L.bh_swd_ellip.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_ssize_t, C.c_ssize_t, C.c_int, vp,
                               C.c_int, vp, vp, C.c_int, vp, vp, vp, vp]
    for name in SWD_ELLIP_SYMBOLS:
        getattr(L, name).restype = C.c_int
    L.bh_targets_set_ellip.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int]
    L.bh_plan_ellip.argtypes = [C.c_int, vp, C.c_int, vp]
    for name in ELLIP_TARGET_SYMBOLS:
        getattr(L, name).restype = C.c_int
    L.bh_targets_set_ellip_sites.argtypes = [vp, C.c_int, C.c_int]
    L.bh_plan_ellip_sites.argtypes = [C.c_int, vp, vp, C.c_int, vp, vp, C.c_int, vp, vp]
    for name in SITE_ELLIP_SYMBOLS:
        getattr(L, name).restype = C.c_int
    for name in ("bh_engine_create", "bh_engine_synchronize", "bh_engine_set_instrumentation", "bh_engine_set_swd_group", "bh_engine_set_swd_lookahead", "bh_engine_set_swd_search", "bh_engine_get_swd_search", "bh_engine_set_swd_arith", "bh_engine_get_swd_arith", "bh_engine_last_swd_kernel", "bh_engine_set_swd_trials", "bh_engine_get_swd_trials", "bh_engine_set_swd_scan", "bh_engine_get_swd_scan", "bh_engine_set_tuning", "bh_engine_get_tuning", "bh_engine_guard_stats", "bh_engine_set_typical_layers", "bh_engine_set_model_order",
                 "bh_timing_reset", "bh_timing_collect", "bh_timing_steps", "bh_last_neval", "bh_debug_counters", "bh_debug_trace", "bh_debug_guard_list", "bh_swd_batch", "bh_rf_batch", "bh_targets_set",
                 "bh_evaluate_batch", "bh_loglike_batch", "bh_probe_math", "bh_probe_swd_secular", "bh_chain_propose", "bh_chain_accept",
                 "bh_chain_propose_window", "bh_chain_accept_window", "bh_sites_set", "bh_evaluate_sites", "bh_sites_set_rf", "bh_sites_set_x", "bh_sites_set_x_all",
                 "bh_sites_set_missing", "bh_chain_propose_sites", "bh_chain_propose_window_sites") + SITE_GAUSS_SYMBOLS + SITE_PRIORS_SYMBOLS + SITE_RF_AXIS_SYMBOLS + SITE_LAWS_SYMBOLS + CHAIN_RECORD_SYMBOLS:
        getattr(L, name).restype = C.c_int
    if L.bh_abi_version() != 10:
        raise EngineError("ABI version mismatch")
    _lib = L
    return L


# include/bh_engine.h: the drop-in contract
EXPORTED_SYMBOLS = ("bh_abi_version", "bh_engine_create", "bh_engine_destroy", "bh_engine_last_error",
                    "bh_engine_stream", "bh_engine_synchronize", "bh_engine_set_swd_search", "bh_engine_get_swd_search",
                    "bh_engine_set_swd_arith", "bh_engine_get_swd_arith", "bh_engine_set_swd_trials", "bh_engine_get_swd_trials",
                    "bh_engine_guard_stats", "bh_engine_set_typical_layers", "bh_engine_set_model_order",
                    "bh_swd_batch", "bh_rf_batch", "bh_targets_set", "bh_evaluate_batch", "bh_loglike_batch",
                    "bh_chain_propose", "bh_chain_accept", "bh_chain_propose_window", "bh_chain_accept_window")
# include/bh_engine_debug.h: measurement, diagnostics, experiment switches (bench.py, tools/, tests)
DEBUG_SYMBOLS = ("bh_engine_set_swd_group", "bh_engine_set_swd_lookahead", "bh_engine_last_swd_kernel", "bh_engine_last_swd_launches",
                 "bh_engine_last_swd_order", "bh_engine_last_swd_perm",
                 "bh_engine_set_swd_scan",
                 "bh_engine_get_swd_scan", "bh_engine_set_tuning",
                 "bh_engine_get_tuning", "bh_probe_math", "bh_probe_swd_secular", "bh_engine_set_instrumentation", "bh_timing_reset",
                 "bh_timing_collect", "bh_timing_steps", "bh_last_neval", "bh_debug_counters", "bh_debug_trace", "bh_debug_guard_list")
# include/bh_engine_sites.h: many stations at once (site-indexed observed data)
SITE_SYMBOLS = ("bh_sites_set", "bh_evaluate_sites")
# include/bh_engine_sites_rf.h: receiver-function ray parameter and near-surface velocity per site
SITE_RF_SYMBOLS = ("bh_sites_set_rf",)
# include/bh_engine_sites_x.h: dispersion periods per site
SITE_X_SYMBOLS = ("bh_sites_set_x",)
# include/bh_engine_sites_x_all.h: ... on every dispersion target (group velocities, higher modes)
SITE_X_ALL_SYMBOLS = ("bh_sites_set_x_all",)
# include/bh_engine_sites_missing.h: sites that lack some of the targets
SITE_MISSING_SYMBOLS = ("bh_sites_set_missing", "bh_chain_propose_sites", "bh_chain_propose_window_sites")
# include/bh_engine_sites_gauss.h: a Gauss-law noise correlation per site
SITE_GAUSS_SYMBOLS = ("bh_sites_set_gauss", "bh_sites_set_missing_gauss")
# include/bh_engine_sites_rf_axis.h: a receiver-function time axis and Gauss filter per site
SITE_RF_AXIS_SYMBOLS = ("bh_sites_set_axes", "bh_sites_set_rf_axis")
# include/bh_engine_sites_laws.h: a noise law per (site, target)
SITE_LAWS_SYMBOLS = ("bh_sites_set_laws",)
# include/bh_engine_sites_priors.h: chains under their own site's priors and sampler settings
SITE_PRIORS_SYMBOLS = ("bh_chain_propose_priors", "bh_chain_propose_window_priors", "bh_chain_accept_priors",
                       "bh_chain_accept_window_priors")
# include/bh_engine_chain_record.h: the window accept calls that write the chains' thinned samples on the device
CHAIN_RECORD_SYMBOLS = ("bh_chain_accept_window_record", "bh_chain_accept_window_priors_record")
# include/bh_engine_posterior.h: posterior velocity-depth summaries of many sites (bayhunter_amd/posterior.py)
POSTERIOR_SYMBOLS = ("bh_posterior_create", "bh_posterior_destroy", "bh_posterior_load", "bh_posterior_columns",
                     "bh_posterior_hist", "bh_posterior_interfaces")
# include/bh_engine_posterior_scalars.h: per-site posteriors of Moho depth, crustal vs and scalar columns (bayhunter_amd/posterior.py)
POSTERIOR_SCALARS_SYMBOLS = ("bh_posterior_keep_rows", "bh_posterior_moho", "bh_posterior_attach", "bh_posterior_scalar_cols", "bh_posterior_scalar_stats",
                             "bh_posterior_scalar_hist", "bh_posterior_scalar_hist2d")
SCALARS_MOHO, SCALARS_USER = 0, 1   # BH_SCALARS_MOHO, BH_SCALARS_USER
# include/bh_engine_posterior_datafit.h: best fits per chain and posterior predictive bands per site (bayhunter_amd/datafits.py)
POSTERIOR_DATAFIT_SYMBOLS = ("bh_posterior_layers", "bh_posterior_best", "bh_posterior_data_fill", "bh_posterior_scalar_quantiles",
                             "bh_posterior_scalar_gather")
SCALARS_DATA = 3                    # BH_SCALARS_DATA
DATAFIT_MAXCOLS = 4096              # BH_DATAFIT_MAXCOLS
QUANTILES_MAXRANKS = 8              # BH_QUANTILES_MAXRANKS
# include/bh_engine_posterior_quantiles.h: several order statistics of every (site, depth) column of the interpolated vs
# (bayhunter_amd/posterior.py: posterior_models(quantiles=...))
POSTERIOR_QUANTILES_SYMBOLS = ("bh_posterior_column_quantiles",)
# include/bh_engine_posterior_cov.h: per-site covariance and correlation of vs at depth and scalar columns
# (bayhunter_amd/posterior.py: posterior_covariance)
POSTERIOR_COV_SYMBOLS = ("bh_posterior_cov", "bh_posterior_cov_finish")
COV_MAXCOLS = 256                   # BH_COV_MAXCOLS
COV_LIMB_BITS = 14                  # BH_COV_LIMB_BITS
# include/bh_engine_posterior_features.h: structural features of the layered models as a scalar set
# (bayhunter_amd/posterior.py: posterior_features)
POSTERIOR_FEATURES_SYMBOLS = ("bh_posterior_features",)
SCALARS_FEATURES = 4                # BH_SCALARS_FEATURES
SCALARS_MAXCOLS = 64                # BH_SCALARS_MAXCOLS
FEATURES_MAXKINDS = 64              # BH_FEATURES_MAXKINDS
(FEATURE_VSMEAN, FEATURE_VSTIME, FEATURE_TTS, FEATURE_VSMIN, FEATURE_VSMAX, FEATURE_DROP, FEATURE_JUMP, FEATURE_ABOVE,
 FEATURE_NIFACES) = range(9)        # BH_FEATURE_*
# include/bh_engine_posterior_classes.h: every row's class by a rule over the scalar sets' columns, and a set's columns by input row
# (bayhunter_amd/posterior.py: posterior_classes and classes=)
POSTERIOR_CLASSES_SYMBOLS = ("bh_posterior_classes", "bh_posterior_scalar_export")
CLASSES_MAX = 16                    # BH_CLASSES_MAX
CLASS_MAXTERMS = 64                 # BH_CLASS_MAXTERMS
CLASS_IN, CLASS_HAS, CLASS_LACKS = 0, 1, 2   # BH_CLASS_*
# include/bh_engine_posterior_resid.h: every row's residuals against the noise it assumed, as a scalar set
# (bayhunter_amd/datafits.py: posterior_residuals)
POSTERIOR_RESID_SYMBOLS = ("bh_posterior_resid_fill",)
SCALARS_RESID = 5                   # BH_SCALARS_RESID
RESID_MAXLAG = 32                   # BH_RESID_MAXLAG
RESID_FIXED = 5                     # BH_RESID_FIXED
# include/bh_engine_chain_diag.h: the sums behind split R-hat and ESS of the chains' recorded series, and the medians of the
# outlier rule (bayhunter_amd/diagnostics.py)
CHAIN_DIAG_SYMBOLS = ("bh_chain_diag_series", "bh_chain_diag_models", "bh_chain_diag_medians")
DIAG_MAXLAG = 2048                  # BH_DIAG_MAXLAG
DIAG_MAXCOLS = 64                   # BH_DIAG_MAXCOLS
DIAG_MAXDEPTHS = 63                 # BH_DIAG_MAXDEPTHS
DIAG_TILE = 256                     # BH_DIAG_TILE
DIAG_LAGBLOCK = 1024                # BH_DIAG_LAGBLOCK
# include/bh_engine_chain_diag_ladders.h: the cold series of tempered runs -- the chain that holds every ladder's largest beta at every
# row, the ladders' mixing numbers, and the sums and medians of series that read that chain (bayhunter_amd/diagnostics.py)
CHAIN_LADDER_SYMBOLS = ("bh_chain_ladder_index", "bh_chain_diag_series_sel", "bh_chain_diag_models_sel", "bh_chain_diag_medians_sel")
LADDER_MAXRUNGS = 64                # BH_LADDER_MAXRUNGS
# include/bh_engine_chain_ladder_evidence.h: the chain that holds every rung of every ladder at every row, and the sums of the
# evidence estimates over the rung series (bayhunter_amd/diagnostics.py: ladder_holders, ladder_evidence)
CHAIN_LADDER_EVIDENCE_SYMBOLS = ("bh_chain_ladder_holders", "bh_chain_ladder_evidence")
EVIDENCE_DROP = 512                 # BH_EVIDENCE_DROP
# include/bh_engine_chain_ladder_sweep.h: the swap sweep of tempered chains as one kernel, with the counts per neighbouring pair of
# rungs and the adaptation of the interior temperatures (LadderSweep below; bayhunter_amd/parallel.py: KernelExchange)
LADDER_SWEEP_SYMBOLS = ("bh_ladder_sweep_create", "bh_ladder_sweep_run", "bh_ladder_sweep_read", "bh_ladder_sweep_destroy")
# include/bh_engine_chain_rank.h: the rank transform of the chains' series pooled per site -- normal scores of the average ranks, of
# the folded ranks, and the tail indicators (bayhunter_amd/diagnostics.py: rank_series, rank_models, rank_convergence)
CHAIN_RANK_SYMBOLS = ("bh_chain_rank_series", "bh_chain_rank_models")
RANK_TILE = 4096                    # BH_RANK_TILE
RANK_RADIXBITS = 8                  # BH_RANK_RADIXBITS
# include/bh_engine_chain_diag_features.h: the structural features of the store's model rows as time-ordered series, value and
# presence (bayhunter_amd/diagnostics.py: chain_feature_series, feature_convergence)
CHAIN_DIAG_FEATURES_SYMBOLS = ("bh_chain_diag_features",)
# include/bh_engine_swd_ellip.h: the Rayleigh ellipticity (H/V) of the fundamental mode from the compound vector at the root
# (Engine.swd_ellip; bayhunter_amd/surf96_ellip.py)
SWD_ELLIP_SYMBOLS = ("bh_swd_ellip",)
ELLIP_MAXSTEPS = 3                  # nsteps of bh_swd_ellip: 0..3
ELLIP_MISMATCH_MAX = 1.0e-2         # BH_ELLIP_MISMATCH_MAX: an entry whose mismatch is above it raises the flag
# include/bh_engine_ellip_target.h: the ellipticity as a registered target with a forward model -- the fused calls and the device
# chains run it (Engine.set_targets; Targets.RayleighEllipticity(fused=True)) -- and the pure plan of where its velocities come from
ELLIP_TARGET_SYMBOLS = ("bh_targets_set_ellip", "bh_plan_ellip")
# include/bh_engine_sites_ellip.h: an ellipticity target with its own periods at every site, or absent at a site
# (Engine.set_target_ellip_sites; SiteTargets(per_site_ellip=True)), and the pure plan of its search under a count table
SITE_ELLIP_SYMBOLS = ("bh_targets_set_ellip_sites", "bh_plan_ellip_sites")


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def pack_models(models, Lmax=None):
    """List of (h, vp, vs, rho) 1-D arrays -> layer-major float64 [Lmax, B] arrays + nlay[B]."""
    B = len(models)
    nlay = np.array([len(m[0]) for m in models], dtype=np.int32)
    if Lmax is None:
        Lmax = int(nlay.max()) if B else 1
    out = [np.zeros((Lmax, B)) for _ in range(4)]
    for b, m in enumerate(models):
        for a, v in zip(out, m):
            a[:nlay[b], b] = v
    return nlay, out[0], out[1], out[2], out[3]


class LadderSweep(object):
    """A plan of include/bh_engine_chain_ladder_sweep.h: the ladders of C chains, with the counters of their sweeps on the device.
    `ladder[c]` in 0..K-1, every id used.  The sorted layout of `logu`, of the counters and of the rung betas: ladder after ladder
    in ascending id, rung 0 the coldest; `start[k] + r` is rung r of ladder k and the pair (r, r+1)."""

    def __init__(self, engine, ladder, K=None):
        lad = np.ascontiguousarray(ladder, dtype=np.int32)
        if lad.ndim != 1 or lad.size < 1:
            raise ValueError("ladder must be a sequence of one id per chain")
        self.engine, self.C = engine, int(lad.size)
        self.K = int(lad.max()) + 1 if K is None else int(K)
        self._h = None
        h = C.c_void_p()
        engine._check(engine._L.bh_ladder_sweep_create(engine._h, self.C, _ptr(lad), self.K, C.byref(h)))
        self._h = h
        self.ladder = lad.astype(np.int64)
        counts = np.bincount(self.ladder, minlength=self.K)
        self.start = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
        self.members = [np.flatnonzero(self.ladder == k) for k in range(self.K)]

    def _f64_dev(self, t, name):
        import torch
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device.index == self.engine.device and t.dtype == torch.float64
                and t.is_contiguous() and t.numel() == self.C):
            raise ValueError("%s must be a contiguous float64 tensor of %d elements on GPU %d" % (name, self.C, self.engine.device))
        return t.data_ptr()

    def run(self, like, beta, logu, parity, phase, adapt=0, kappa=0.0, stream=None):
        """Enqueue one sweep (stream None: the engine's): `beta` is updated in place, nothing waits.  `like`, `beta`, `logu`:
        float64 device tensors [C], logu in the sorted layout.  adapt with phase 1 is refused (BH_EINVAL)."""
        e = self.engine
        e._check(e._L.bh_ladder_sweep_run(e._h, self._h, stream, self._f64_dev(like, "like"), self._f64_dev(beta, "beta"),
                                          self._f64_dev(logu, "logu"), int(parity), int(phase), int(adapt), float(kappa)))

    def read(self):
        """Wait for the last sweep; dict of proposed, accepted (int64 [2][C]: phase, position), rung_beta (float64 [C], zeros before
        the first sweep), adaptations, skipped (int64 [K])."""
        e = self.engine
        out = dict(proposed=np.zeros((2, self.C), dtype=np.int64), accepted=np.zeros((2, self.C), dtype=np.int64),
                   rung_beta=np.zeros(self.C), adaptations=np.zeros(self.K, dtype=np.int64), skipped=np.zeros(self.K, dtype=np.int64))
        e._check(e._L.bh_ladder_sweep_read(e._h, self._h, _ptr(out["proposed"]), _ptr(out["accepted"]), _ptr(out["rung_beta"]),
                                           _ptr(out["adaptations"]), _ptr(out["skipped"])))
        return out

    def close(self):
        if getattr(self, "_h", None) and getattr(self.engine, "_h", None):
            self.engine._L.bh_ladder_sweep_destroy(self.engine._h, self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine(object):
    """One engine = one GPU (HIP device ordinal `device`) = one stream."""

    def __init__(self, device=0):
        self._L = load_library()
        h = C.c_void_p()
        rc = self._L.bh_engine_create(int(device), C.byref(h))
        if rc != BH_OK:
            raise EngineError("bh_engine_create(device=%d) failed with %d: no usable HIP device "
                              "(this package has no CPU fallback)" % (device, rc))
        self._h = h
        self.device = int(device)
        self._owner = None  # the JointTarget whose targets are currently registered
        self.ntargets = 0
        self.ldy = 0
        self.nsites = 0

    def close(self):
        if getattr(self, "_h", None):
            self._L.bh_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != BH_OK:
            msg = self._L.bh_engine_last_error(self._h)
            raise EngineError("engine call failed (%d): %s" % (rc, msg.decode() if msg else "?"))

    # -- plumbing ---------------------------------------------------------------------------
    @property
    def stream(self):
        return self._L.bh_engine_stream(self._h)

    def synchronize(self):
        self._check(self._L.bh_engine_synchronize(self._h))

    def set_instrumentation(self, timing=False, counting=False):
        self._check(self._L.bh_engine_set_instrumentation(self._h, int(timing), int(counting)))

    def set_swd_group(self, lanes_per_model):
        """0 = automatic; 1..32 lanes of a wavefront per model in the dispersion kernel."""
        self._check(self._L.bh_engine_set_swd_group(self._h, int(lanes_per_model)))

    def set_typical_layers(self, nlay):
        """Hint for device-resident batches: typical layer count (0 = unknown)."""
        self._check(self._L.bh_engine_set_typical_layers(self._h, int(nlay)))

    def set_model_order(self, sort_by_depth=True):
        """False: batches are of uniform depth (or sorted already): skip the on-device sort by layer count."""
        self._check(self._L.bh_engine_set_model_order(self._h, int(bool(sort_by_depth))))

    def set_swd_lookahead(self, trials_per_round):
        """0 = automatic; 1..12 trial phase velocities per round of the dispersion root search."""
        self._check(self._L.bh_engine_set_swd_lookahead(self._h, int(trials_per_round)))

    def set_swd_search(self, search):
        """"fast" (the engine's default): the reference's brackets, ~3 evaluations inside each instead of nevill's 10-12;
        fundamental-mode phase-velocity targets only; within 1.2e-6 relative of the reference (north_star: 1e-5), failure
        flags the reference's (a guard re-runs the models whose outcome hinges on the last bits of a root with the
        reference's sequence).  "reference": the reference's sequence of secular-function evaluations, velocities
        bit-identical to surfdisp96 (replays of recorded reference chains: ChainBatch).  "fast_rayleigh": "fast" for the
        Rayleigh targets only -- for samplers, whose Love proposals trip the guard too often (include/bh_engine.h)."""
        codes = {"reference": SEARCH_REFERENCE, "fast": SEARCH_FAST, "fast_rayleigh": SEARCH_FAST_RAYLEIGH}
        codes.update({v: v for v in list(codes.values())})
        code = codes.get(search)
        if code is None:
            raise ValueError("search must be 'reference', 'fast' or 'fast_rayleigh'")
        self._check(self._L.bh_engine_set_swd_search(self._h, code))

    def swd_search(self):
        return {SEARCH_FAST: "fast", SEARCH_FAST_RAYLEIGH: "fast_rayleigh"}.get(self._L.bh_engine_get_swd_search(self._h), "reference")

    @contextlib.contextmanager
    def settings(self, search=None, arith=None, trials=None, typical_layers=None):
        """The calls inside run with these settings (set_swd_search / set_swd_arith / set_swd_trials / set_typical_layers); an argument
        of None leaves the engine's own.  A value is set only where it differs from the engine's, and what was set is restored
        afterwards, in reverse order, also when the body raises.  typical_layers cannot be read back: it is set on entry and reset
        to 0 (unknown) on exit."""
        undo = []
        try:
            for value, get, put in ((search, self.swd_search, self.set_swd_search), (arith, self.swd_arith, self.set_swd_arith),
                                    (trials, self.swd_trials, self.set_swd_trials)):
                prev = None if value is None else get()
                if prev != value:
                    put(value)
                    undo.append((put, prev))
            if typical_layers is not None:
                self.set_typical_layers(typical_layers)
                undo.append((self.set_typical_layers, 0))
            yield self
        finally:
            for put, prev in reversed(undo):
                put(prev)

    def searching(self, search):
        """The calls inside run with this root refinement; the engine's setting is restored afterwards."""
        return self.settings(search=search)

    def set_swd_arith(self, arith):
        """Arithmetic of the launches in which every target takes the short refinement (include/bh_engine.h:
        bh_engine_set_swd_arith): "fast" (default) = fused multiply-adds, Newton-refined hardware reciprocals, polynomial
        sin / cos / exp -- same guarantees as the "fast" search; "exact" = the reference's operations and rounding points."""
        codes = {"exact": ARITH_EXACT, "fast": ARITH_FAST, ARITH_EXACT: ARITH_EXACT, ARITH_FAST: ARITH_FAST}
        code = codes.get(arith)
        if code is None:
            raise ValueError("arith must be 'exact' or 'fast'")
        self._check(self._L.bh_engine_set_swd_arith(self._h, code))

    def set_swd_trials(self, trials):
        """Trials per model and round of the trial-per-lane kernel: 0 = by the call's shape (64 up to 1024 (model, target)
        pairs, 32 up to 5120, 16 up to 10240, 8 up to 28672, 4 beyond), or 4 / 8 / 16 / 32 / 64 in every call (bh_engine_set_swd_trials)."""
        self._check(self._L.bh_engine_set_swd_trials(self._h, int(trials)))

    def swd_trials(self):
        return int(self._L.bh_engine_get_swd_trials(self._h))

    def trying(self, trials):
        """The calls inside run the trial-per-lane kernel with this many trials per round (None: the engine's setting stays);
        the engine's setting is restored afterwards."""
        return self.settings(trials=trials)

    def last_swd_kernel(self):
        """Which dispersion kernel the most recent call launched: "group", "lane", "lean" (bh_engine_last_swd_kernel) or None."""
        return {0: "group", 1: "lane", 2: "lean"}.get(self._L.bh_engine_last_swd_kernel(self._h))

    def last_swd_launches(self):
        """Every dispersion kernel launch of the most recent call with dispersion targets (bh_engine_last_swd_launches), in launch
        order: dicts of family ("group" / "lane" / "lean"), role ("main" / "rerun" / "second"), key (the instantiation's template
        arguments, a tuple of 6 ints) and the launch's features."""
        out = (SwdLaunch * 32)()
        n = C.c_int(0)
        self._check(self._L.bh_engine_last_swd_launches(self._h, out, 32, C.byref(n)))
        return [dict(family={0: "group", 1: "lane", 2: "lean"}[r.family], role={0: "main", 1: "rerun", 2: "second"}[r.role],
                     key=tuple(r.key), two_classes=bool(r.two_classes), interleaved=bool(r.interleaved),
                     pair_order=bool(r.pair_order), restart=bool(r.restart), grid_x=int(r.grid_x), fair=int(r.fair))
                for r in out[:n.value]]

    def last_swd_order(self):
        """How the most recent call with dispersion targets ordered its models (bh_engine_last_swd_order): (order, workgroups,
        fills) -- "none" / "depth" / "length" / "pair"; workgroups of the ordering launch (0: none, 1, or 8: one per XCD block);
        the set of what that launch zeroed for the call, of "guard", "flags", "counters"."""
        wg, fills = C.c_int(0), C.c_int(0)
        order = self._L.bh_engine_last_swd_order(self._h, C.byref(wg), C.byref(fills))
        return ({0: "none", 1: "depth", 2: "length", 3: "pair"}.get(order), int(wg.value),
                {n for b, n in ((1, "guard"), (2, "flags"), (4, "counters")) if fills.value & b})

    def last_swd_perm(self, target, B):
        """The processing order the most recent call with dispersion targets computed for target 0 / 1 of its launch
        (bh_engine_last_swd_perm): int32 [B], or None where it kept the caller's order."""
        out = np.zeros(int(B), dtype=np.int32)
        n = self._L.bh_engine_last_swd_perm(self._h, int(target), out.ctypes.data_as(C.POINTER(C.c_int32)), int(B))
        if n < 0:
            self._check(n)
        return out[:n] if n > 0 else None

    def swd_arith(self):
        return "fast" if self._L.bh_engine_get_swd_arith(self._h) == ARITH_FAST else "exact"

    def computing(self, arith):
        """The calls inside run with this arithmetic; the engine's setting is restored afterwards."""
        return self.settings(arith=arith)

    def set_swd_scan(self, scan):
        """Love bracket scans: "counted" = skip the steps a mode count proves to be without a sign change (same brackets, same
        bits, a third of the scan's evaluations) wherever a Love target is; "auto" (default) = only where that is measured
        to pay; "steps" = every step evaluated, as the reference does (include/bh_engine.h: bh_engine_set_swd_scan)."""
        codes = {"steps": SCAN_STEPS, "counted": SCAN_COUNTED, "auto": SCAN_AUTO}
        codes.update({v: v for v in list(codes.values())})
        code = codes.get(scan)
        if code is None:
            raise ValueError("scan must be 'steps', 'counted' or 'auto'")
        self._check(self._L.bh_engine_set_swd_scan(self._h, code))

    def swd_scan(self):
        return {SCAN_STEPS: "steps", SCAN_COUNTED: "counted"}.get(self._L.bh_engine_get_swd_scan(self._h), "auto")

    def guard_stats(self):
        """(models per target of the last dispersion call that the guard of the "fast" search ran again with the reference's
        sequence -- in the re-run launch or, one model per wavefront, in place --, re-run launches enqueued since the engine
        was created)"""
        counts = (C.c_int32 * 8)()
        n = C.c_uint64(0)
        self._check(self._L.bh_engine_guard_stats(self._h, counts, C.byref(n), None))
        return list(counts), int(n.value)

    def guard_total(self):
        """guarded (model, target) pairs since the engine was created"""
        return sum(self.guard_totals())

    def guard_totals(self):
        """the same per dispersion target of the calls (in the order the targets were registered)"""
        tot = (C.c_uint64 * 8)()
        self._check(self._L.bh_engine_guard_stats(self._h, None, None, tot))
        return [int(x) for x in tot]

    def timing_reset(self):
        self._check(self._L.bh_timing_reset(self._h))

    def timing_collect(self):
        """(ncalls, total_ms, {'swd': ms, 'rf': ms, 'like': ms}) summed over the timed calls
        since timing_reset(); waits for them to finish."""
        n = C.c_int(0)
        tot = C.c_double(0)
        fam = (C.c_double * 3)()
        self._check(self._L.bh_timing_collect(self._h, C.byref(n), C.byref(tot), fam))
        return n.value, tot.value, {"swd": fam[0], "rf": fam[1], "like": fam[2]}

    def timing_steps(self, maxn=4096):
        """Per-call times [ms] of the timed calls since timing_reset(): start of call i -> start of call i+1 (the last:
        its own span), from the engine's own events."""
        out = np.zeros(int(maxn))
        n = C.c_int(0)
        self._check(self._L.bh_timing_steps(self._h, int(maxn), out.ctypes.data_as(_d), C.byref(n)))
        return out[:n.value].copy()

    def last_timing(self):
        """(total_ms, families) of the calls since the last reset, then resets."""
        n, tot, fam = self.timing_collect()
        self.timing_reset()
        return tot, fam

    def debug_counters(self):
        out = (C.c_uint64 * 16)()
        self._check(self._L.bh_debug_counters(self._h, out))
        return [int(v) for v in out]

    def debug_trace(self):
        """Development aid: [nwaves, 4] uint64 records of the last counted dispersion launch
        (start, end in 100 MHz ticks, core cycles, rounds | wave type << 32 | HW_ID << 36)."""
        n = min(self.debug_counters()[7], 16384)
        out = (C.c_uint64 * (4 * max(n, 1)))()
        self._check(self._L.bh_debug_trace(self._h, out, n))
        return np.frombuffer(out, dtype=np.uint64).reshape(-1, 4)[:n].copy()

    def guard_list(self, target, B):
        """Development aid: the batch indices (int32, unordered) that the guard listed for the re-run launch of the most recent
        dispersion call, for its target-th dispersion target; B: that call's batch size (bh_debug_guard_list)."""
        out = np.zeros(max(int(B), 1), dtype=np.int32)
        n = C.c_int(0)
        self._check(self._L.bh_debug_guard_list(self._h, int(target), int(B), out.ctypes.data_as(C.POINTER(C.c_int32)), int(B), C.byref(n)))
        return out[:n.value].copy()

    def last_neval(self):
        v = C.c_uint64(0)
        self._check(self._L.bh_last_neval(self._h, C.byref(v)))
        return int(v.value)

    @staticmethod
    def _model_args(nlay, h, vp, vs, rho, layout):
        """Validate host model arrays; returns (B, Lmax, stride_l, stride_b, arrays...)."""
        h = _f64(h)
        if layout == "layer_major":   # [Lmax, B]
            Lmax, B = h.shape
            sl, sb = max(B, 1), 1
        elif layout == "model_major":  # [B, Lmax]
            B, Lmax = h.shape
            sl, sb = 1, Lmax
        else:
            raise ValueError("layout must be 'layer_major' or 'model_major'")
        arrs = [h] + [None if a is None else _f64(a) for a in (vp, vs, rho)]
        for a in arrs:
            if a is not None and a.shape != h.shape:
                raise ValueError("model arrays must have identical shapes")
        nlay = np.ascontiguousarray(nlay, dtype=np.int32)
        if nlay.shape != (B,):
            raise ValueError("nlay must have shape (B,)")
        if B and (nlay.min() < 1 or nlay.max() > Lmax):
            raise ValueError("nlay entries must be in 1..Lmax")
        return B, Lmax, sl, sb, nlay, arrs

    # -- host API ---------------------------------------------------------------------------
    def swd_batch(self, nlay, h, vp, vs, rho, periods, iwave, igr, mode=1, flsph=0,
                  layout="layer_major"):
        """Batched surfdisp96.  Returns (vel[B, K], err[B])."""
        B, Lmax, sl, sb, nlay, (h, vp, vs, rho) = self._model_args(nlay, h, vp, vs, rho, layout)
        periods = _f64(periods)
        K = periods.size
        vel = np.zeros((B, K))
        err = np.zeros(B, dtype=np.int32)
        self._check(self._L.bh_swd_batch(self._h, HOST, None, B, Lmax, _ptr(nlay), _ptr(h), _ptr(vp),
                                         _ptr(vs), _ptr(rho), sl, sb, K, _ptr(periods), int(iwave),
                                         int(igr), int(mode), int(flsph), _ptr(vel), _ptr(err)))
        return vel, err

    def swd_ellip(self, nlay, h, vp, vs, rho, periods, vel=None, err=None, nsteps=2, layout="layer_major"):
        """Rayleigh ellipticity of the fundamental mode (include/bh_engine_swd_ellip.h): hv = u_r / u_z at the surface, positive =
        retrograde.  vel [B, K] and err [B] given: the phase velocities to start from; else the engine's own Rayleigh phase
        search runs first (with the search and arithmetic it is set to).  nsteps: secant steps of the polish (0..3).
        Returns a dict: hv [B, K], mismatch [B, K] (the relative difference of the two expressions of hv: a bound of its
        error), c [B, K] (the velocity hv was evaluated at), vel [B, K], err [B], flag [B] (a step of the polish left the window of
        1e-5 c, a value is not a number, or a mismatch is above ELLIP_MISMATCH_MAX: the arithmetic does not determine hv).  A model without a root (err != 0) and an entry with vel <= 0 are zero rows."""
        B, Lmax, sl, sb, nlay, (h, vp, vs, rho) = self._model_args(nlay, h, vp, vs, rho, layout)
        periods = _f64(periods).reshape(-1)
        K = periods.size
        if (vel is None) != (err is None):
            raise ValueError("vel and err go together")
        have = vel is not None
        if have:
            vel = np.array(vel, dtype=np.float64, order="C")
            err = np.array(err, dtype=np.int32, order="C")
            if vel.shape != (B, K) or err.shape != (B,):
                raise ValueError("vel must have shape (B, K) and err (B,)")
        else:
            vel = np.zeros((B, K))
            err = np.zeros(B, dtype=np.int32)
        hv, mis, cpol = np.zeros((B, K)), np.zeros((B, K)), np.zeros((B, K))
        flag = np.zeros(B, dtype=np.int32)
        self._check(self._L.bh_swd_ellip(self._h, HOST, None, B, Lmax, _ptr(nlay), _ptr(h), _ptr(vp), _ptr(vs), _ptr(rho), sl, sb,
                                         K, _ptr(periods), int(have), _ptr(vel), _ptr(err), int(nsteps), _ptr(hv), _ptr(mis),
                                         _ptr(cpol), _ptr(flag)))
        return {"hv": hv, "mismatch": mis, "c": cpol, "vel": vel, "err": err, "flag": flag}

    def rf_batch(self, nlay, h, vp, vs, rho, p, gauss, nsamp, fsamp, tshift, waveno, nkeep,
                 nsv=0.0, qp=None, qs=None, layout="layer_major"):
        """Batched rfmini synrf.  Returns rf[B, nkeep]."""
        B, Lmax, sl, sb, nlay, (h, vp, vs, rho) = self._model_args(nlay, h, vp, vs, rho, layout)
        qp = None if qp is None else _f64(qp)
        qs = None if qs is None else _f64(qs)
        rf = np.zeros((B, int(nkeep)))
        self._check(self._L.bh_rf_batch(self._h, HOST, None, B, Lmax, _ptr(nlay), _ptr(h), _ptr(vp),
                                        _ptr(vs), _ptr(rho), _ptr(qp), _ptr(qs), sl, sb, float(p),
                                        float(gauss), int(nsamp), float(fsamp), float(tshift),
                                        float(nsv), int(waveno), int(nkeep), _ptr(rf)))
        return rf

    def set_targets(self, descs):
        """descs: list of dicts with the `bh_target_desc` fields (arrays as numpy)."""
        arr = (TargetDesc * max(1, len(descs)))()
        keep = []
        ldy = 0
        for i, d in enumerate(descs):
            t = arr[i]
            t.kind, t.law, t.n = int(d["kind"]), int(d["law"]), int(d["n"])
            t.iwave, t.igr = int(d.get("iwave", 2)), int(d.get("igr", 0))
            t.mode, t.flsph = int(d.get("mode", 1)), int(d.get("flsph", 0))
            t.waveno, t.nsamp = int(d.get("waveno", 0)), int(d.get("nsamp", 0))
            t.p_s_per_deg, t.gauss = float(d.get("p", 6.4)), float(d.get("gauss", 1.0))
            t.fsamp, t.tshift, t.nsv = float(d.get("fsamp", 1.0)), float(d.get("tshift", 0.0)), float(d.get("nsv", 0.0))
            for key in ("x", "yobs", "yerr", "rinv"):
                v = d.get(key)
                if v is not None:
                    v = _f64(v)
                    keep.append(v)
                    setattr(t, key, v.ctypes.data_as(_d))
            t.logdet_r = float(d.get("logdet_r", 0.0))
            ldy += t.n
        self._check(self._L.bh_targets_set(self._h, len(descs), arr))
        self.ntargets = len(descs)
        self.ldy = ldy
        self.nsites = 0
        for i, d in enumerate(descs):   # (a USER descriptor with nsteps: it takes the ellipticity forward model at its x)
            if int(d["kind"]) == TARGET_USER and "nsteps" in d:
                self.set_target_ellip(i, d["x"], nsteps=d["nsteps"], signed=d.get("signed", False), ratio=d.get("ratio", "hv"))
                if d.get("ellip_sites"):    # (its periods and counts are the count table's, site by site)
                    self.set_target_ellip_sites(i, True)

    TARGET_ELLIP = TARGET_ELLIP

    def set_target_ellip_sites(self, t, own=True):
        """Registered ellipticity target t takes its periods and their count from the count table, site by site
        (bh_targets_set_ellip_sites, include/bh_engine_sites_ellip.h): between set_target_ellip and any set_sites*.  Its n is then
        the capacity of its columns and its registered periods a placeholder; set_sites_x_all or a later table serves it, with
        set_sites_missing and beyond a site may lack it (count 0).  evaluate_batch refuses such a set; set_targets resets the flag."""
        self._check(self._L.bh_targets_set_ellip_sites(self._h, int(t), int(bool(own))))

    def set_target_ellip(self, t, periods, nsteps=2, signed=False, ratio="hv"):
        """Give registered USER target t the Rayleigh-ellipticity forward model at `periods` (bh_targets_set_ellip,
        include/bh_engine_ellip_target.h): its kind is TARGET_ELLIP from then on, and the fused calls compute it."""
        if ratio not in ("hv", "zh"):
            raise ValueError("ratio must be 'hv' or 'zh', not %r" % (ratio,))
        x = _f64(np.asarray(periods, dtype=float).reshape(-1))
        self._check(self._L.bh_targets_set_ellip(self._h, int(t), int(x.size), _ptr(x), int(nsteps), int(bool(signed)), int(ratio == "zh")))

    def evaluate_batch(self, nlay, h, vp, vs, noise, rho=None, layout="layer_major", want_ymod=False):
        """Batched JointTarget.evaluate.  noise[B, 2*nt].  Returns (logL[B], misfits[B, nt+1],
        err[B][, ymod[B, ldy]])."""
        B, Lmax, sl, sb, nlay, (h, vp, vs, rho) = self._model_args(nlay, h, vp, vs, rho, layout)
        nt = self.ntargets
        noise = _f64(noise)
        if noise.shape != (B, 2 * nt):
            raise ValueError("noise must have shape (B, 2*ntargets)")
        logL = np.zeros(B)
        misf = np.zeros((B, nt + 1))
        err = np.zeros(B, dtype=np.int32)
        ymod = np.zeros((B, self.ldy)) if want_ymod else None
        self._check(self._L.bh_evaluate_batch(self._h, HOST, None, B, Lmax, _ptr(nlay), _ptr(h),
                                              _ptr(vp), _ptr(vs), _ptr(rho), sl, sb, _ptr(noise),
                                              _ptr(logL), _ptr(misf), _ptr(err), _ptr(ymod)))
        return (logL, misf, err, ymod) if want_ymod else (logL, misf, err)

    def set_sites(self, yobs, yerr=None):
        """Observed data of S sites for the registered targets (bh_sites_set): yobs[S, ldy], target after target as in ymod;
        yerr[S, ldy] is read in the columns of nocorr_scalederr targets only (None if there is none).  set_targets drops it."""
        yobs = _f64(yobs)
        if yobs.ndim != 2 or yobs.shape[1] != self.ldy or yobs.shape[0] < 1:
            raise ValueError("yobs must have shape (nsites, %d)" % self.ldy)
        if yerr is not None:
            yerr = _f64(yerr)
            if yerr.shape != yobs.shape:
                raise ValueError("yerr must have the shape of yobs")
        self._check(self._L.bh_sites_set(self._h, yobs.shape[0], _ptr(yobs), _ptr(yerr)))
        self.nsites = yobs.shape[0]

    def set_sites_x(self, n, x, yobs, yerr=None):
        """The site table together with every site's own dispersion periods (bh_sites_set_x, instead of set_sites): n[S, nt]
        int32 samples of every (site, target); x, yobs and yerr[S, ldy] in ymod's column layout, the columns beyond a site's
        count unread.  The registered descriptors give every dispersion target's capacity (their n) and a placeholder x.
        evaluate_sites then computes a model's dispersion curves at its site's periods; set_targets and set_sites drop the table."""
        self._set_sites_x(self._L.bh_sites_set_x, n, x, yobs, yerr)

    def set_sites_x_all(self, n, x, yobs, yerr=None):
        """set_sites_x for every dispersion target the engine serves (bh_sites_set_x_all): group-velocity and higher-mode
        targets may differ from site to site in their periods and counts as well; same arrays, same lifetime."""
        self._set_sites_x(self._L.bh_sites_set_x_all, n, x, yobs, yerr)

    def set_sites_missing(self, n, x, yobs, yerr=None):
        """set_sites_x_all where a count may be 0: that site lacks that target (bh_sites_set_missing) -- nothing of it is
        computed, read or added for the site's models.  Same arrays, same lifetime; with a receiver-function target
        set_sites_rf must follow."""
        self._set_sites_x(self._L.bh_sites_set_missing, n, x, yobs, yerr)

    def set_sites_missing_gauss(self, n, x, yobs, yerr=None):
        """set_sites_missing that accepts a Gauss-law target which some site lacks (bh_sites_set_missing_gauss); such a target
        then needs its table of correlation classes (set_sites_gauss, the lacking sites in class -1) before evaluate_sites."""
        self._set_sites_x(self._L.bh_sites_set_missing_gauss, n, x, yobs, yerr)

    def set_sites_axes(self, n, x, yobs, yerr=None):
        """set_sites_missing_gauss where a receiver function's count may be 0 or 1 .. its descriptor's n, the capacity of its
        columns (bh_sites_set_axes).  A count that differs from the descriptor's then needs set_sites_rf and set_sites_rf_axis
        before evaluate_sites -- and, Gauss law, the padded class table of set_sites_gauss."""
        self._set_sites_x(self._L.bh_sites_set_axes, n, x, yobs, yerr)

    def set_sites_rf_axis(self, nsamp, fsamp, tshift, gauss):
        """The receiver-function transform length nsamp (int32), sampling rate fsamp (Hz), time shift tshift (s) and Gauss width
        gauss of every site (bh_sites_set_rf_axis): arrays [nsites, ntargets], read in the columns of receiver-function targets
        only.  evaluate_sites then synthesises a model's trace on its site's own axis.  Register it after set_sites_rf, which
        drops it as set_sites* and set_targets do, and before set_sites_gauss."""
        nsamp = np.ascontiguousarray(nsamp, dtype=np.int32)
        fsamp, tshift, gauss = _f64(fsamp), _f64(tshift), _f64(gauss)
        if nsamp.ndim != 2 or nsamp.shape[1] != self.ntargets or any(a.shape != nsamp.shape for a in (fsamp, tshift, gauss)):
            raise ValueError("nsamp, fsamp, tshift and gauss must have shape (nsites, %d)" % self.ntargets)
        self._check(self._L.bh_sites_set_rf_axis(self._h, nsamp.shape[0], _ptr(nsamp), _ptr(fsamp), _ptr(tshift), _ptr(gauss)))

    def set_sites_laws(self, law, yerr=None):
        """The noise law of every (site, target) for the count table in force (bh_sites_set_laws): law[nsites, ntargets] int32
        (LAW_NOCORR .. LAW_GAUSS; an entry where the site's count is 0 is not read; LAW_GAUSS only on a target whose descriptor
        is LAW_GAUSS) and yerr[nsites, ldy], the sites' errors in the count table's layout, read where the law is
        LAW_NOCORR_SCALED (None: no such pair).  evaluate_sites then evaluates every model under its own site's laws.  Register
        it after set_sites_missing_gauss / set_sites_axes and the receiver-function tables, which drop it as set_targets does,
        and before set_sites_gauss, which it drops: the classes are checked against the laws (-1 for a site under another law)."""
        law = np.ascontiguousarray(law, dtype=np.int32)
        if law.ndim != 2 or law.shape[1] != self.ntargets:
            raise ValueError("law must have shape (nsites, %d)" % self.ntargets)
        if yerr is not None:
            yerr = _f64(yerr)
            if yerr.shape != (law.shape[0], self.ldy):
                raise ValueError("yerr must have shape (nsites, %d)" % self.ldy)
        self._check(self._L.bh_sites_set_laws(self._h, law.shape[0], _ptr(law), _ptr(yerr)))

    def set_sites_gauss(self, target, class_of, rinv, logdet_r):
        """The noise-correlation classes of Gauss-law target `target` for the site table in force (bh_sites_set_gauss):
        class_of[nsites] int32, the class of every site (-1: the site lacks the target); rinv[nclass, n, n] and logdet_r[nclass],
        R^-1 and ln|R| of every class.  evaluate_sites then contracts every model with its site's class's matrix.  Register it
        last: set_targets and every other set_sites* drop it."""
        class_of = np.ascontiguousarray(class_of, dtype=np.int32)
        rinv, logdet_r = _f64(rinv), _f64(logdet_r)
        if class_of.ndim != 1:
            raise ValueError("class_of must have shape (nsites,)")
        if rinv.ndim != 3 or rinv.shape[1] != rinv.shape[2] or logdet_r.shape != rinv.shape[:1]:
            raise ValueError("rinv must have shape (nclass, n, n) and logdet_r (nclass,)")
        self._check(self._L.bh_sites_set_gauss(self._h, int(target), class_of.shape[0], rinv.shape[0], _ptr(class_of), _ptr(rinv),
                                               _ptr(logdet_r)))

    def _set_sites_x(self, entry, n, x, yobs, yerr):
        """set_sites_x / set_sites_x_all: the arrays checked and handed to entry point `entry`"""
        n = np.ascontiguousarray(n, dtype=np.int32)
        x, yobs = _f64(x), _f64(yobs)
        if yobs.ndim != 2 or yobs.shape[1] != self.ldy or yobs.shape[0] < 1:
            raise ValueError("yobs must have shape (nsites, %d)" % self.ldy)
        if x.shape != yobs.shape:
            raise ValueError("x must have the shape of yobs")
        if n.shape != (yobs.shape[0], self.ntargets):
            raise ValueError("n must have shape (nsites, %d)" % self.ntargets)
        if yerr is not None:
            yerr = _f64(yerr)
            if yerr.shape != yobs.shape:
                raise ValueError("yerr must have the shape of yobs")
        self._check(entry(self._h, yobs.shape[0], _ptr(n), _ptr(x), _ptr(yobs), _ptr(yerr)))
        self.nsites = yobs.shape[0]

    def set_sites_rf(self, p, nsv):
        """Receiver-function ray parameter p (s/deg) and near-surface velocity nsv (<= 0: the model's top-layer vs) of every
        site (bh_sites_set_rf): float64 arrays [nsites, ntargets], read in the columns of receiver-function targets only.
        evaluate_sites then gives a model its site's values; set_sites and set_targets drop them."""
        p, nsv = _f64(p), _f64(nsv)
        if p.ndim != 2 or p.shape[1] != self.ntargets or nsv.shape != p.shape:
            raise ValueError("p and nsv must have shape (nsites, %d)" % self.ntargets)
        self._check(self._L.bh_sites_set_rf(self._h, p.shape[0], _ptr(p), _ptr(nsv)))

    def evaluate_sites(self, nlay, h, vp, vs, noise, site, rho=None, layout="layer_major", want_ymod=False):
        """evaluate_batch with model b compared with the observed data of site site[b] (bh_evaluate_sites).  Returns (logL[B],
        misfits[B, nt+1], err[B][, ymod[B, ldy]])."""
        B, Lmax, sl, sb, nlay, (h, vp, vs, rho) = self._model_args(nlay, h, vp, vs, rho, layout)
        nt = self.ntargets
        noise = _f64(noise)
        if noise.shape != (B, 2 * nt):
            raise ValueError("noise must have shape (B, 2*ntargets)")
        site = np.ascontiguousarray(site, dtype=np.int32)
        if site.shape != (B,):
            raise ValueError("site must have shape (B,)")
        logL = np.zeros(B)
        misf = np.zeros((B, nt + 1))
        err = np.zeros(B, dtype=np.int32)
        ymod = np.zeros((B, self.ldy)) if want_ymod else None
        self._check(self._L.bh_evaluate_sites(self._h, HOST, None, B, Lmax, _ptr(nlay), _ptr(h), _ptr(vp), _ptr(vs), _ptr(rho),
                                              sl, sb, _ptr(site), _ptr(noise), _ptr(logL), _ptr(misf), _ptr(err), _ptr(ymod)))
        return (logL, misf, err, ymod) if want_ymod else (logL, misf, err)

    def loglike_batch(self, ymod, noise, fail=None):
        """Likelihood of caller-supplied synthetics ymod[B, ldy] (see bh_loglike_batch)."""
        ymod = _f64(ymod)
        B = ymod.shape[0]
        nt = self.ntargets
        if ymod.shape != (B, self.ldy):
            raise ValueError("ymod must have shape (B, %d)" % self.ldy)
        noise = _f64(noise)
        if noise.shape != (B, 2 * nt):
            raise ValueError("noise must have shape (B, 2*ntargets)")
        if fail is not None:
            fail = np.ascontiguousarray(fail, dtype=np.int32)
            if fail.shape != (nt, B):
                raise ValueError("fail must have shape (ntargets, B)")
        logL = np.zeros(B)
        misf = np.zeros((B, nt + 1))
        err = np.zeros(B, dtype=np.int32)
        self._check(self._L.bh_loglike_batch(self._h, HOST, None, B, _ptr(ymod), _ptr(fail), _ptr(noise),
                                             _ptr(logL), _ptr(misf), _ptr(err)))
        return logL, misf, err

    def set_tuning(self, name, value):
        """An experiment switch of the library (csrc/bh_tuning.h; process-wide, never changes a result)."""
        self._check(self._L.bh_engine_set_tuning(self._h, name.encode(), int(value)))

    def tuning(self, name):
        v = C.c_int(0)
        self._check(self._L.bh_engine_get_tuning(self._h, name.encode(), C.byref(v)))
        return int(v.value)

    def probe_math(self, op, x):
        x = _f64(x).ravel()
        out = np.zeros(x.size // 2 if op in (6, 7) else x.size)
        self._check(self._L.bh_probe_math(self._h, int(op), out.size, x.ctypes.data_as(_d), out.ctypes.data_as(_d)))
        return out

    def probe_swd_secular(self, evaluator, ifunc, mmax, d, a, b, rho, wvno, omega, out=None):
        """bh_probe_swd_secular (include/bh_engine_debug.h): the secular function of ONE model (rows d, a, b, rho: binary32, mtop of
        them, the first mmax the model) at the points (wvno[i], omega[i]).  evaluator 0 the exact arithmetic, 1 fa::*_secular,
        2 lean_rayleigh / lean_love.  `out` (optional): the float64 array written to (left untouched by a refused call)."""
        f = [np.ascontiguousarray(x, dtype=np.float32).ravel() for x in (d, a, b, rho)]
        mtop = f[0].size
        if any(x.size != mtop for x in f):
            raise ValueError("d, a, b, rho must have the same length")
        wvno, omega = _f64(wvno).ravel(), _f64(omega).ravel()
        if wvno.size != omega.size:
            raise ValueError("wvno and omega must have the same length")
        if out is None:
            out = np.zeros(wvno.size)
        if out.dtype != np.float64 or out.size != wvno.size or not out.flags.c_contiguous:
            raise ValueError("out must be a contiguous float64 array of the points' length")
        self._check(self._L.bh_probe_swd_secular(self._h, int(evaluator), int(ifunc), int(mmax), mtop, f[0].ctypes.data, f[1].ctypes.data,
                                                 f[2].ctypes.data, f[3].ctypes.data, wvno.size, wvno.ctypes.data_as(_d),
                                                 omega.ctypes.data_as(_d), out.ctypes.data_as(_d)))
        return out

    # -- device API (raw pointers; asynchronous) ---------------------------------------------
    def swd_batch_dev(self, B, Lmax, nlay, h, vp, vs, rho, sl, sb, K, periods, iwave, igr, vel, err,
                      stream=None, mode=1, flsph=0):
        self._check(self._L.bh_swd_batch(self._h, DEVICE, stream, B, Lmax, nlay, h, vp, vs, rho, sl, sb,
                                         K, periods, iwave, igr, mode, flsph, vel, err))

    def swd_ellip_dev(self, B, Lmax, nlay, h, vp, vs, rho, sl, sb, K, periods, vel, err, hv, flag, have_vel=False, nsteps=2,
                      mismatch=None, cpol=None, stream=None):
        """bh_swd_ellip on device pointers, enqueued on `stream` (None: the engine's); vel / err are written unless have_vel."""
        self._check(self._L.bh_swd_ellip(self._h, DEVICE, stream, B, Lmax, nlay, h, vp, vs, rho, sl, sb, K, periods,
                                         int(bool(have_vel)), vel, err, int(nsteps), hv, mismatch, cpol, flag))

    def rf_batch_dev(self, B, Lmax, nlay, h, vp, vs, rho, sl, sb, p, gauss, nsamp, fsamp, tshift,
                     waveno, nkeep, rf, stream=None, nsv=0.0, qp=None, qs=None):
        self._check(self._L.bh_rf_batch(self._h, DEVICE, stream, B, Lmax, nlay, h, vp, vs, rho, qp, qs,
                                        sl, sb, p, gauss, nsamp, fsamp, tshift, nsv, waveno, nkeep, rf))

    def evaluate_batch_dev(self, B, Lmax, nlay, h, vp, vs, rho, sl, sb, noise, logL, misfits, err,
                           ymod=None, stream=None):
        self._check(self._L.bh_evaluate_batch(self._h, DEVICE, stream, B, Lmax, nlay, h, vp, vs, rho,
                                              sl, sb, noise, logL, misfits, err, ymod))

    def evaluate_sites_dev(self, B, Lmax, nlay, h, vp, vs, rho, sl, sb, site, noise, logL, misfits, err,
                           ymod=None, stream=None):
        """Device pointers; site = int32 [B] (a site out of range: that model fails in band)."""
        self._check(self._L.bh_evaluate_sites(self._h, DEVICE, stream, B, Lmax, nlay, h, vp, vs, rho,
                                              sl, sb, site, noise, logL, misfits, err, ymod))


    def _chain(self, symbol, cfg, state, C_, iiter, *args, named=None):
        """Call the chain-step entry point `symbol` with (stream, cfg, state, C, iiter, *args); an EngineError names it."""
        rc = getattr(self._L, symbol)(self.stream, C.byref(cfg), C.byref(state), int(C_), int(iiter), *args)
        if rc != BH_OK:
            raise EngineError("%s failed (%d)" % (named or symbol, rc))

    def chain_propose(self, cfg, state, C_, iiter):
        self._chain("bh_chain_propose", cfg, state, C_, iiter)

    def chain_accept(self, cfg, state, C_, iiter, logL, misfits):
        self._chain("bh_chain_accept", cfg, state, C_, iiter, logL, misfits)

    def chain_propose_window(self, cfg, state, C_, iiter, depth, ld, absent=None):
        """absent: None, or the device pointer of uint8 [C] -- bit t set: the chain's site lacks target t (bh_chain_propose_window_sites)"""
        if absent is not None:     # (the one method with two symbols: its error names the method's own either way)
            self._chain("bh_chain_propose_window_sites", cfg, state, C_, iiter, int(depth), int(ld), absent, named="bh_chain_propose_window")
        else:
            self._chain("bh_chain_propose_window", cfg, state, C_, iiter, int(depth), int(ld))

    def chain_propose_window_priors(self, cfg, state, C_, iiter, depth, ld, priors, nprior, prior_of, absent=None):
        """bh_chain_propose_window_priors.  priors: device pointer of `nprior` ChainPrior records; prior_of: device pointer of
        int32 [C], the record of each chain; absent: as in chain_propose_window (None: every target present)"""
        self._chain("bh_chain_propose_window_priors", cfg, state, C_, iiter, int(depth), int(ld), priors, int(nprior), prior_of, absent)

    def chain_accept_window_priors(self, cfg, state, C_, iiter, depth, ld, logL, misfits, priors, nprior, prior_of):
        """bh_chain_accept_window_priors (arguments as chain_propose_window_priors)"""
        self._chain("bh_chain_accept_window_priors", cfg, state, C_, iiter, int(depth), int(ld), logL, misfits, priors, int(nprior), prior_of)

    def chain_accept_window_record(self, cfg, state, C_, iiter, depth, ld, logL, misfits, rec):
        """bh_chain_accept_window_record.  rec: a ChainRecord (include/bh_engine_chain_record.h)"""
        self._chain("bh_chain_accept_window_record", cfg, state, C_, iiter, int(depth), int(ld), logL, misfits, C.byref(rec))

    def chain_accept_window_priors_record(self, cfg, state, C_, iiter, depth, ld, logL, misfits, priors, nprior, prior_of, rec):
        """bh_chain_accept_window_priors_record (arguments as chain_accept_window_priors, then the ChainRecord)"""
        self._chain("bh_chain_accept_window_priors_record", cfg, state, C_, iiter, int(depth), int(ld), logL, misfits, priors, int(nprior),
                    prior_of, C.byref(rec))

    def chain_accept_window(self, cfg, state, C_, iiter, depth, ld, logL, misfits):
        self._chain("bh_chain_accept_window", cfg, state, C_, iiter, int(depth), int(ld), logL, misfits)


_default = {}


def default_engine(device=0):
    """Process-wide engine per device (what the plugin classes use)."""
    e = _default.get(device)
    if e is None:
        e = Engine(device)
        _default[device] = e
    return e
