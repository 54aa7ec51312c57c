"""ctypes binding of librlhip.so (include/rlhip.h).

The library is built in-tree (ranklib_amd/lib/librlhip.so) by ranklib_amd/csrc/Makefile.
There is no fallback: if the shared object is missing or no gfx950 device is visible the calls raise
RankLibError, exactly like the reference's unchecked error convention (utilities/RankLibError.java).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RLHIP_LIB") or os.path.join(_HERE, "lib", "librlhip.so")     # RLHIP_LIB: A/B builds (tools/)


class RankLibError(RuntimeError):
    """Mirrors ciir.umass.edu.utilities.RankLibError (utilities/RankLibError.java:9-43)."""


class RlParams(C.Structure):
    _fields_ = [("n_trees", C.c_int32), ("n_leaves", C.c_int32), ("n_threshold", C.c_int32),
                ("min_leaf_support", C.c_int32), ("early_stop_rounds", C.c_int32), ("learning_rate", C.c_float),
                ("metric", C.c_int32), ("metric_k", C.c_int32), ("device", C.c_int32), ("flags", C.c_int32),
                ("ranker", C.c_int32), ("feature_sampling_rate", C.c_float), ("seed", C.c_uint64)]


RL_METRIC = dict(NDCG=0, DCG=1, MAP=2, ERR=3, P=4, RR=5)      # the tree trainer's train metrics (RL_METRIC_* of rlhip.h)
RL_CA_METRIC = dict(NDCG=0, DCG=1, MAP=2, ERR=3, P=4, RR=5)   # the linear rankers' (the same six; LambdaRank keeps its own four, learning.LambdaRank._METRICS)
RL_NORM_KIND = dict(sum=0, zscore=1, linear=2)   # RL_NORM_* of rlhip.h: the names -norm takes
RL_EVAL_METRIC = dict(RL_CA_METRIC, BEST=6)    # eval_lists scores all seven; no trainer accepts BEST


class RlCaParams(C.Structure):
    _fields_ = [("n_restart", C.c_int32), ("n_max_iteration", C.c_int32), ("step_base", C.c_double), ("step_scale", C.c_double),
                ("tolerance", C.c_double), ("regularized", C.c_int32), ("slack", C.c_double), ("metric", C.c_int32),
                ("metric_k", C.c_int32), ("device", C.c_int32), ("seed", C.c_int64), ("err_max", C.c_double)]


class RlCaTraceRec(C.Structure):
    _fields_ = [("kind", C.c_int32), ("restart", C.c_int32), ("feature", C.c_int32), ("dir", C.c_int32), ("j", C.c_int32),
                ("improved", C.c_int32), ("weight", C.c_double), ("score", C.c_double)]


CA_TRACE_DTYPE = np.dtype([("kind", np.int32), ("restart", np.int32), ("feature", np.int32), ("dir", np.int32), ("j", np.int32),
                           ("improved", np.int32), ("weight", np.float64), ("score", np.float64)])
CA_RESTART, CA_PASS, CA_TRIAL, CA_SUCCESS, CA_VALID = 0, 1, 2, 3, 4


class RlAdaParams(C.Structure):
    _fields_ = [("n_iteration", C.c_int32), ("tolerance", C.c_double), ("train_with_enqueue", C.c_int32), ("max_sel_count", C.c_int32),
                ("metric", C.c_int32), ("metric_k", C.c_int32), ("device", C.c_int32), ("err_max", C.c_double)]


ADA_TRACE_DTYPE = np.dtype([("iteration", np.int32), ("kind", np.int32), ("feature", np.int32), ("status", np.int32),
                            ("alpha", np.float64), ("train_score", np.float64), ("valid_score", np.float64)])
ADA_ROUND, ADA_ROLLBACK, ADA_PHASE = 0, 1, 2
ADA_OK, ADA_DAMN, ADA_FREM = 0, 1, 2
ADA_STATUS = {ADA_OK: "OK", ADA_DAMN: "DAMN", ADA_FREM: "F. REM."}


class RlRbParams(C.Structure):
    _fields_ = [("n_iteration", C.c_int32), ("n_threshold", C.c_int32), ("metric", C.c_int32), ("metric_k", C.c_int32),
                ("device", C.c_int32), ("keep_potentials", C.c_int32), ("err_max", C.c_double)]


RB_TRACE_DTYPE = np.dtype([("iteration", np.int32), ("feature", np.int32), ("threshold", np.float64), ("max_r", np.float64),
                           ("r_t", np.float64), ("alpha", np.float64), ("z_t", np.float64), ("train_score", np.float64),
                           ("valid_score", np.float64)])


class RlLrParams(C.Structure):
    _fields_ = [("lambda_", C.c_double), ("metric", C.c_int32), ("metric_k", C.c_int32), ("device", C.c_int32), ("err_max", C.c_double)]


class RlLnParams(C.Structure):
    _fields_ = [("n_epochs", C.c_int32), ("learning_rate", C.c_double), ("metric", C.c_int32), ("metric_k", C.c_int32),
                ("device", C.c_int32), ("err_max", C.c_double)]


class RlLnTraceRec(C.Structure):
    _fields_ = [("epoch", C.c_int32), ("saved", C.c_int32), ("train", C.c_double), ("valid", C.c_double)]


LN_TRACE_DTYPE = np.dtype([("epoch", np.int32), ("saved", np.int32), ("train", np.float64), ("valid", np.float64)])
RL_ERR_NO_BEST = -7                    # rl_ln_learn / rl_rn_learn: no epoch scored above 0.0 on the validation set


class RlRnParams(C.Structure):
    _fields_ = [("n_epochs", C.c_int32), ("learning_rate", C.c_double), ("n_hidden", C.c_int32), ("hidden_sizes", C.POINTER(C.c_int32)),
                ("metric", C.c_int32), ("metric_k", C.c_int32), ("device", C.c_int32), ("err_max", C.c_double)]


RN_TRACE_DTYPE = np.dtype([("epoch", np.int32), ("saved", np.int32), ("misordered", np.int64), ("total_pairs", np.int64),
                           ("train", np.float64), ("valid", np.float64)])

RL_RANKER = dict(MART=0, LAMBDAMART=6)


class RlTree(C.Structure):
    _fields_ = [("n_nodes", C.c_int32), ("cap", C.c_int32), ("feature", C.POINTER(C.c_int32)),
                ("threshold", C.POINTER(C.c_float)), ("left", C.POINTER(C.c_int32)),
                ("right", C.POINTER(C.c_int32)), ("output", C.POINTER(C.c_float)),
                ("deviance", C.POINTER(C.c_double)), ("count", C.POINTER(C.c_int32))]


RL_FLAG_TIMING, RL_FLAG_SERIAL_CHAIN, RL_FLAG_TIMING_NODES, RL_FLAG_JAVA_ORDER, RL_FLAG_FIRST_TIE = 2, 4, 8, 16, 32
RL_FLAG_FAST_LEAF = 1      # leaf sums as the fixed f64 reduction of DESIGN.md 14 instead of the Java's float running sums (opt-in, one GPU)
ARR = dict(LAMBDA=1, WEIGHT=2, SCORE=3, VALID_SCORE=4, NBINS=5, THRESHOLDS=6, BINS=7, ROOT_COUNT=8, ROOT_SUM=9,
           QUANT=10, ROOT_SUM_FIXED=11, NDCG_PER_QUERY=12, CHAIN_STATS=13, CHAIN_MISS=14, GROW_STATS=15, PHASE_CLOCKS=16,
           ROOT_SUM_JAVA=17, GROW_DOCS=18, SPARSE_INFO=19, STEP_LOG=20, TIE_STATS=21, BLOCK_TRACE=22, BUBBLES=23, PIECE_STATS=24, LAUNCH_ARMS=25)
# indices into array("LAUNCH_ARMS") (include/rlhip.h RL_ARM_* / RL_HARM_*; tests/test_abi.py holds the two lists together): which kernel variant the
# host launched.  A k_hist arm is ARM["HIST_ROOT"] + HARM[..] for the root pass, ARM["HIST_CHILD"] + HARM[..] for the child passes
HARM = dict(COMPACT=0, SUB8=1, SUB4=2, NT1024=3, NT512=4, FQ_PACKED=5, FQ_ROWS16=6, PACKED_RUNS=7, PACKED=8, ROWS16_RUNS=9, ROWS16=10, STRIDE=11, COUNT_=12)
ARM = dict(HIST_ROOT=0, HIST_CHILD=12, RANK_TINY=24, RANK_MIXED=25, RANK_WAVE_LONG=26, RANK_WAVE_SHORT=27, RANK_BLOCK=28, RANK_HUGE=29,
           LAM_MART=30, LAM_TINY=31, LAM_FUSED=32, LAM_COMPACT=33, LAM_ERR=34, LAM_MAP=35, LAM_UNFUSED=36, LAM_ON_SIDE=37, LAM_ON_MAIN=38,
           QUANTIZE=39, XPLAN_HOST=40, XPLAN_DEVICE=41, STEPS_ENQUEUED=42, SET_STEP_AHEAD=43, SET_DIST_AHEAD=44, CHILD_GRID_X=45, CHILD_GRID_Y=46, CHILD_LDS=47,
           SET_P8=48, SET_DM_ROOT=49, SET_DM_DIV=50, SET_SUB_CHILD=51, SET_HIST_NT=52, SET_ANY_RUNS=53, SET_CROWS=54, SET_TIE_ON=55, SET_NODE_DIV=56,
           SET_NODE_MIN=57, SET_BALANCE=58, SET_BALANCE_TARGET=59, SET_BALANCE_MIN=60, SET_BALANCE_CAP=61, SET_NODE_CHUNK=62, SET_MAX_CHUNKS=63, REPLAY_TILED=64, REPLAY_DIRECT=65, COUNT_=66)
KERNEL = dict(HIST_ROOT=0, HIST_NODE=1, LAMBDA=2)

# every symbol include/rlhip.h declares (tests/test_abi.py checks the .so exports all of them)
ABI_SYMBOLS = [
    "rl_abi_version", "rl_last_error", "rl_device_count", "rl_params_default", "rl_create", "rl_destroy",
    "rl_set_train", "rl_set_validation", "rl_set_rows", "rl_set_external_judgments", "rl_init", "rl_boost_round", "rl_boost_rounds_async", "rl_sync",
    "rl_finish", "rl_num_trees", "rl_get_tree", "rl_get_round_metrics", "rl_best_validation", "rl_predict",
    "rl_model_to_text", "rl_model_from_text", "rl_model_destroy", "rl_model_num_trees", "rl_model_features",
    "rl_model_predict", "rl_model_predict_device", "rl_model_debug_path", "rl_dist_unique_id", "rl_dist_init", "rl_dist_init_callback", "rl_dist_stats", "rl_bin_stride", "rl_hist_features", "rl_quant_exponent", "rl_get_array", "rl_debug_exp", "rl_debug_rho", "rl_debug_float_chain", "rl_debug_fast_sum",
    "rl_letor_parse", "rl_letor_info", "rl_letor_arrays", "rl_letor_rows", "rl_letor_destroy", "rl_letor_format",
    "rl_get_timing", "rl_reset_timing", "rl_set_timing_flags", "rl_debug_membench", "rl_set_err_max", "rl_tree_capacity",
    "rl_ca_params_default", "rl_ca_create", "rl_ca_destroy", "rl_ca_set_train", "rl_ca_set_validation", "rl_ca_set_external_judgments",
    "rl_ca_learn", "rl_ca_get_weights", "rl_ca_scores", "rl_ca_trace", "rl_ca_predict",
    "rl_ada_params_default", "rl_ada_create", "rl_ada_destroy", "rl_ada_set_train", "rl_ada_set_validation", "rl_ada_set_external_judgments",
    "rl_ada_learn", "rl_ada_get_model", "rl_ada_scores", "rl_ada_trace", "rl_ada_debug_weak_table",
    "rl_rb_params_default", "rl_rb_create", "rl_rb_destroy", "rl_rb_set_train", "rl_rb_set_validation", "rl_rb_set_external_judgments",
    "rl_rb_learn", "rl_rb_get_model", "rl_rb_scores", "rl_rb_trace", "rl_rb_debug_potentials", "rl_rb_predict",
    "rl_lr_params_default", "rl_lr_create", "rl_lr_destroy", "rl_lr_set_train", "rl_lr_set_validation", "rl_lr_set_external_judgments",
    "rl_lr_set_features", "rl_lr_learn", "rl_lr_get_weights", "rl_lr_scores", "rl_lr_debug_gram", "rl_lr_debug_times", "rl_lr_predict",
    "rl_net_create", "rl_net_destroy", "rl_net_predict", "rl_net_predict_device", "rl_net_debug_path",
    "rl_ln_params_default", "rl_ln_create", "rl_ln_destroy", "rl_ln_set_train", "rl_ln_set_validation", "rl_ln_set_external_judgments",
    "rl_ln_set_weights", "rl_ln_learn", "rl_ln_get_weights", "rl_ln_scores", "rl_ln_trace", "rl_ln_debug_doc_scores", "rl_ln_debug_times",
    "rl_rn_params_default", "rl_rn_create", "rl_rn_destroy", "rl_rn_set_train", "rl_rn_set_validation", "rl_rn_set_external_judgments",
    "rl_rn_set_weights", "rl_rn_learn", "rl_rn_get_weights", "rl_rn_scores", "rl_rn_trace", "rl_rn_debug_doc_scores", "rl_rn_debug_times",
    "rl_rn_set_lambdarank",
    "rl_perm_test", "rl_debug_perm_calib",
    "rl_eval_lists", "rl_debug_eval_times",
    "rl_normalize_lists", "rl_debug_normalize_times",
    "rl_model_predict_stages", "rl_model_eval_stages", "rl_debug_stage_times",
    "rl_model_predict_permuted", "rl_model_eval_permuted", "rl_debug_permuted_times",
    "rl_model_cover", "rl_model_cover_rows", "rl_model_get_cover", "rl_model_predict_contribs", "rl_model_predict_leaf_sums", "rl_debug_contrib_times", "rl_debug_contrib_passes",
    "rl_model_predict_shap", "rl_model_shap_limits", "rl_debug_shap_times", "rl_debug_shap_passes",
    "rl_adopt_model_text",
    "rl_refit_model_text", "rl_debug_refit_stats",
    "rl_model_predict_partial", "rl_debug_partial_times",
    "rl_model_predict_interactions", "rl_debug_interact_times", "rl_debug_interact_passes",
]

HOST_ALLREDUCE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32)
HOST_ALLGATHER = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64)
HOST_ALLTOALLV = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64))
DT_NUMPY = {0: np.int64, 1: np.uint64, 2: np.int32, 3: np.uint32, 4: np.float64}

_lib = None


def lib():
    """Load librlhip.so; fail loudly if it has not been built (no CPU fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RankLibError("librlhip.so is missing (%s): run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "or `make -C ranklib_amd/csrc`. There is no CPU fallback." % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, f32p = C.c_void_p, C.c_int32, C.c_int64, C.POINTER(C.c_float)
    L.rl_abi_version.restype = C.c_int
    L.rl_last_error.restype = C.c_char_p
    L.rl_device_count.argtypes = [C.POINTER(i32)]
    L.rl_params_default.argtypes = [C.POINTER(RlParams)]
    L.rl_params_default.restype = None
    L.rl_create.argtypes = [C.POINTER(RlParams), C.POINTER(vp)]
    L.rl_destroy.argtypes = [vp]
    L.rl_destroy.restype = None
    L.rl_set_train.argtypes = [vp, vp, i64, i32, vp, vp, i32, vp, vp]
    L.rl_set_validation.argtypes = [vp, vp, i64, vp, vp, i32, vp]
    L.rl_set_rows.argtypes = [vp, i32, i64, i64, vp]
    L.rl_set_external_judgments.argtypes = [vp, i32, vp, vp]
    L.rl_init.argtypes = [vp]
    L.rl_boost_round.argtypes = [vp, C.POINTER(RlTree), f32p, f32p, C.POINTER(i32)]
    L.rl_boost_rounds_async.argtypes = [vp, i32]
    L.rl_sync.argtypes = [vp]
    L.rl_finish.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.rl_num_trees.argtypes = [vp, C.POINTER(i32)]
    L.rl_tree_capacity.argtypes = [vp, C.POINTER(i32)]
    L.rl_get_tree.argtypes = [vp, i32, C.POINTER(RlTree)]
    L.rl_get_round_metrics.argtypes = [vp, i32, f32p, f32p]
    L.rl_best_validation.argtypes = [vp, C.POINTER(i32), C.POINTER(C.c_double)]
    L.rl_predict.argtypes = [vp, vp, i64, vp]
    L.rl_model_to_text.argtypes = [vp, C.c_char_p, i64, C.POINTER(i64)]
    L.rl_model_from_text.argtypes = [C.c_char_p, i32, C.POINTER(vp)]
    L.rl_model_destroy.argtypes = [vp]
    L.rl_model_destroy.restype = None
    L.rl_model_num_trees.argtypes = [vp, C.POINTER(i32)]
    L.rl_model_features.argtypes = [vp, vp, i32, C.POINTER(i32)]
    L.rl_model_predict.argtypes = [vp, vp, i64, i32, vp]
    L.rl_model_predict_device.argtypes = [vp, vp, i64, i32, vp, vp]
    if hasattr(L, "rl_model_debug_path"):   # (A/B builds of older sources lack it)
        L.rl_model_debug_path.argtypes = [vp, C.POINTER(i32)]
    L.rl_dist_unique_id.argtypes = [vp]
    L.rl_dist_init.argtypes = [vp, vp, i32, i32]
    L.rl_dist_stats.argtypes = [vp, vp]
    L.rl_dist_init_callback.argtypes = [vp, i32, i32, HOST_ALLREDUCE, HOST_ALLGATHER, HOST_ALLTOALLV, vp]
    L.rl_bin_stride.argtypes = [vp, C.POINTER(i32)]
    L.rl_hist_features.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), i32]
    L.rl_quant_exponent.argtypes = [vp, C.POINTER(i32)]
    L.rl_get_array.argtypes = [vp, i32, vp, i64]
    L.rl_debug_exp.argtypes = [vp, i32, vp, vp]
    if hasattr(L, "rl_debug_rho"):      # (A/B builds of older sources selected with RLHIP_LIB lack the probe; tests/test_abi.py checks the in-tree library's exports)
        L.rl_debug_rho.argtypes = [vp, vp, i32, vp, vp]
    L.rl_debug_float_chain.argtypes = [i32, vp, i64, vp, i32, vp, vp]
    if hasattr(L, "rl_debug_fast_sum"):      # (A/B builds of older sources lack it)
        L.rl_debug_fast_sum.argtypes = [i32, vp, i64, vp, i32, vp, vp]
    L.rl_letor_parse.argtypes = [vp, i64, C.POINTER(vp)]
    L.rl_letor_info.argtypes = [vp, C.POINTER(i64), C.POINTER(i32), C.POINTER(i64)]
    L.rl_letor_arrays.argtypes = [vp] * 10
    L.rl_letor_rows.argtypes = [vp, vp, i64]
    L.rl_letor_destroy.argtypes = [vp]
    L.rl_letor_destroy.restype = None
    if hasattr(L, "rl_letor_format"):   # (A/B builds of older sources write LETOR text in Python)
        L.rl_letor_format.argtypes = [vp, i64, i64, vp, vp, vp, i64, vp, vp, vp, vp, vp, i64, C.POINTER(i64)]
    L.rl_get_timing.argtypes = [vp, i32, C.POINTER(C.c_double), C.POINTER(i64), C.POINTER(C.c_double)]
    L.rl_reset_timing.argtypes = [vp]
    L.rl_set_err_max.argtypes = [C.c_double]
    L.rl_set_timing_flags.argtypes = [vp, i32]
    L.rl_debug_membench.argtypes = [i32, i32, i64, i32, i32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    for pre, params in (("rl_ca_", RlCaParams), ("rl_ada_", RlAdaParams), ("rl_rb_", RlRbParams), ("rl_lr_", RlLrParams),
                        ("rl_ln_", RlLnParams), ("rl_rn_", RlRnParams)):
        if not hasattr(L, pre + "create"):      # (A/B builds of older sources lack the later linear rankers)
            continue
        fn = lambda name: getattr(L, pre + name)      # noqa: E731
        fn("params_default").argtypes = [C.POINTER(params)]
        fn("params_default").restype = None
        fn("create").argtypes = [C.POINTER(params), C.POINTER(vp)]
        fn("destroy").argtypes = [vp]
        fn("destroy").restype = None
        fn("set_train").argtypes = [vp, vp, i64, i32, vp, vp, i32, vp]
        fn("set_validation").argtypes = [vp, vp, i64, vp, vp, i32, vp]
        fn("set_external_judgments").argtypes = [vp, i32, vp, vp]
        fn("learn").argtypes = [vp]
        fn("scores").argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    if hasattr(L, "rl_ca_create"):
        L.rl_ca_get_weights.argtypes = [vp, vp, i32]
        L.rl_ca_trace.argtypes = [vp, vp, i64, C.POINTER(i64)]
        L.rl_ca_predict.argtypes = [i32, vp, vp, i32, vp, i64, i32, vp]
    if hasattr(L, "rl_ada_create"):
        L.rl_ada_get_model.argtypes = [vp, vp, vp, i32, C.POINTER(i32)]
        L.rl_ada_trace.argtypes = [vp, vp, i64, C.POINTER(i64)]
        L.rl_ada_debug_weak_table.argtypes = [vp, vp, i64]
    if hasattr(L, "rl_rb_create"):
        L.rl_rb_get_model.argtypes = [vp, vp, vp, vp, i32, C.POINTER(i32)]
        L.rl_rb_trace.argtypes = [vp, vp, i64, C.POINTER(i64)]
        L.rl_rb_debug_potentials.argtypes = [vp, i32, vp, i64]
        L.rl_rb_predict.argtypes = [i32, vp, vp, vp, i32, vp, i64, i32, vp]
    if hasattr(L, "rl_lr_create"):
        L.rl_lr_set_features.argtypes = [vp, i32, vp, i32]
        L.rl_lr_get_weights.argtypes = [vp, vp, i32, C.POINTER(i32)]
        L.rl_lr_debug_gram.argtypes = [vp, vp, vp, i32, C.POINTER(i32)]
        L.rl_lr_debug_times.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(i32)]
        L.rl_lr_predict.argtypes = [i32, vp, i32, vp, i32, vp, i64, i32, vp]
    if hasattr(L, "rl_ln_create"):
        L.rl_ln_set_weights.argtypes = [vp, vp, i32]
        L.rl_ln_get_weights.argtypes = [vp, vp, i32, C.POINTER(i32)]
        L.rl_ln_trace.argtypes = [vp, vp, i64, C.POINTER(i64)]
        L.rl_ln_debug_doc_scores.argtypes = [vp, i32, vp, i64]
        L.rl_ln_debug_times.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    if hasattr(L, "rl_rn_create"):
        L.rl_rn_set_weights.argtypes = [vp, vp, i32]
        L.rl_rn_get_weights.argtypes = [vp, vp, i32, C.POINTER(i32)]
        L.rl_rn_trace.argtypes = [vp, vp, i64, C.POINTER(i64)]
        L.rl_rn_debug_doc_scores.argtypes = [vp, i32, vp, i64]
        L.rl_rn_debug_times.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        if hasattr(L, "rl_rn_set_lambdarank"):
            L.rl_rn_set_lambdarank.argtypes = [vp, i32]
    if hasattr(L, "rl_net_create"):
        L.rl_net_create.argtypes = [i32, vp, i32, vp, i32, vp, i32, C.POINTER(vp)]
        L.rl_net_destroy.argtypes = [vp]
        L.rl_net_destroy.restype = None
        L.rl_net_predict.argtypes = [vp, vp, i64, i32, vp]
        L.rl_net_predict_device.argtypes = [vp, vp, i64, i32, vp, vp]
        L.rl_net_debug_path.argtypes = [vp, C.POINTER(i32)]
    if hasattr(L, "rl_perm_test"):      # (A/B builds of older sources lack the Analyzer's test)
        L.rl_perm_test.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, i64, i64, i64, vp, vp, vp]
        L.rl_debug_perm_calib.argtypes = [C.c_int, vp, vp, C.c_int, i64, i64, i64, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                          C.POINTER(i64)]
    if hasattr(L, "rl_eval_lists"):     # (A/B builds of older sources rank and score on the host)
        L.rl_eval_lists.argtypes = [i32, i32, i32, C.c_double, vp, vp, i64, vp, i32, vp, vp, vp, vp, vp, vp]
        L.rl_debug_eval_times.argtypes = [C.POINTER(C.c_double)]
    if hasattr(L, "rl_normalize_lists"):    # (A/B builds of older sources normalise on the host)
        L.rl_normalize_lists.argtypes = [i32, i32, vp, i64, i32, vp, vp, i32, vp, i32, i32]
        L.rl_debug_normalize_times.argtypes = [C.POINTER(C.c_double)]
    if hasattr(L, "rl_model_eval_stages"):  # (A/B builds of older sources score one truncated model per stage)
        L.rl_model_predict_stages.argtypes = [vp, vp, i64, i32, vp, i32, vp]
        L.rl_model_eval_stages.argtypes = [vp, vp, i64, i32, vp, vp, i32, vp, vp, vp, i32, i32, C.c_double, vp, i32, i64, vp, vp, vp]
        L.rl_debug_stage_times.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double)]
    if hasattr(L, "rl_model_eval_permuted"):  # (A/B builds of older sources score one permuted copy per cell)
        L.rl_model_predict_permuted.argtypes = [vp, vp, i64, i32, vp, i32, vp, i32, vp, vp]
        L.rl_model_eval_permuted.argtypes = [vp, vp, i64, i32, vp, vp, i32, vp, vp, vp, i32, i32, C.c_double, vp, i32, vp, i32, i64, vp, vp, vp, vp, vp]
        L.rl_debug_permuted_times.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double)]
    if hasattr(L, "rl_model_predict_contribs"):  # (A/B builds of older sources have no contributions)
        L.rl_model_cover.argtypes = [vp, vp, i64, i32, i32]
        L.rl_model_cover_rows.argtypes = [vp, C.POINTER(i64)]
        L.rl_model_get_cover.argtypes = [vp, i32, vp, vp, i32, C.POINTER(i32)]
        L.rl_model_predict_contribs.argtypes = [vp, vp, i64, i32, vp, i32, i64, vp]
        L.rl_model_predict_leaf_sums.argtypes = [vp, vp, i64, i32, vp]
        L.rl_debug_contrib_times.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.rl_debug_contrib_passes.argtypes = [C.POINTER(i32)]
    if hasattr(L, "rl_model_predict_shap"):   # (A/B builds of older sources have Saabas contributions only)
        L.rl_model_predict_shap.argtypes = [vp, vp, i64, i32, vp, i32, i64, vp]
        L.rl_model_shap_limits.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
        L.rl_debug_shap_times.argtypes = [C.POINTER(C.c_double)]
        L.rl_debug_shap_passes.argtypes = [C.POINTER(i32)]
    if hasattr(L, "rl_adopt_model_text"):     # (A/B builds of older sources cannot resume)
        L.rl_adopt_model_text.argtypes = [vp, C.c_char_p, i64, C.POINTER(i32)]
    if hasattr(L, "rl_refit_model_text"):     # (A/B builds of older sources cannot refit)
        L.rl_refit_model_text.argtypes = [vp, C.c_char_p, C.c_float, C.POINTER(i32)]
        L.rl_debug_refit_stats.argtypes = [vp, C.POINTER(i64)]
    if hasattr(L, "rl_model_predict_partial"):  # (A/B builds of older sources have no partial dependence)
        L.rl_model_predict_partial.argtypes = [vp, vp, i64, i32, vp, i32, vp, vp, i64, vp, vp, vp, vp]
        L.rl_debug_partial_times.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double)]
    if hasattr(L, "rl_model_predict_interactions"):  # (A/B builds of older sources have no interaction values)
        L.rl_model_predict_interactions.argtypes = [vp, vp, i64, i32, vp, i32, i64, vp]
        L.rl_debug_interact_times.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.rl_debug_interact_passes.argtypes = [C.POINTER(i32)]
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise RankLibError("%s (rlhip status %d)" % (lib().rl_last_error().decode("utf-8", "replace"), rc))


def device_count():
    n = C.c_int32(0)
    rc = lib().rl_device_count(C.byref(n))
    return n.value if rc == 0 else 0


class FlatTree:
    """One regression tree in pre-order (root 0, left subtree first)."""

    def __init__(self, cap):
        self.cap = cap
        self.feature = np.full(cap, -1, np.int32)
        self.threshold = np.zeros(cap, np.float32)
        self.left = np.full(cap, -1, np.int32)
        self.right = np.full(cap, -1, np.int32)
        self.output = np.zeros(cap, np.float32)
        self.deviance = np.zeros(cap, np.float64)
        self.count = np.zeros(cap, np.int32)
        self.n_nodes = 0

    def c(self):
        def p(a, t):
            return a.ctypes.data_as(C.POINTER(t))
        return RlTree(0, self.cap, p(self.feature, C.c_int32), p(self.threshold, C.c_float), p(self.left, C.c_int32),
                      p(self.right, C.c_int32), p(self.output, C.c_float), p(self.deviance, C.c_double),
                      p(self.count, C.c_int32))

    def trimmed(self):
        n = self.n_nodes
        return dict(feature=self.feature[:n].copy(), threshold=self.threshold[:n].copy(), left=self.left[:n].copy(),
                    right=self.right[:n].copy(), output=self.output[:n].copy(), deviance=self.deviance[:n].copy(),
                    count=self.count[:n].copy())


def debug_exp(x):
    x = np.ascontiguousarray(x, np.float64)
    a, b = np.zeros_like(x), np.zeros_like(x)
    check(lib().rl_debug_exp(x.ctypes.data, len(x), a.ctypes.data, b.ctypes.data))
    return a, b


def debug_rho(x, den=None):
    """rl_debug_rho: (fast, ref) of rho(x) = 1 / (1 + exp(x)), or of x / den when den is given"""
    x = np.ascontiguousarray(x, np.float64)
    if den is not None:
        den = np.ascontiguousarray(den, np.float64)
        assert den.shape == x.shape
    a, b = np.zeros_like(x), np.zeros_like(x)
    check(lib().rl_debug_rho(x.ctypes.data, den.ctypes.data if den is not None else None, len(x), a.ctypes.data, b.ctypes.data))
    return a, b


def letor_parse(data):
    """Native LETOR parser (rl_letor_*): `data` = the file's bytes.  Returns a dict of per-line arrays, the dense row matrix
    (NaN = not named on the line) and the flags of the lines the caller has to parse itself."""
    buf = C.create_string_buffer(data, len(data)) if not isinstance(data, C.Array) else data
    h = C.c_void_p()
    check(lib().rl_letor_parse(buf, len(data), C.byref(h)))
    try:
        n, mf, ns = C.c_int64(), C.c_int32(), C.c_int64()
        check(lib().rl_letor_info(h, C.byref(n), C.byref(mf), C.byref(ns)))
        n, mf = n.value, mf.value
        out = dict(n=n, max_fid=mf, n_slow=ns.value, labels=np.zeros(n, np.float32), last_fid=np.zeros(n, np.int32),
                   qid_off=np.zeros(n, np.int64), qid_len=np.zeros(n, np.int32), desc_off=np.zeros(n, np.int64), desc_len=np.zeros(n, np.int32),
                   line_off=np.zeros(n, np.int64), line_len=np.zeros(n, np.int32), slow=np.zeros(n, np.uint8))
        check(lib().rl_letor_arrays(h, *[out[k].ctypes.data for k in ("labels", "last_fid", "qid_off", "qid_len", "desc_off", "desc_len",
                                                                       "line_off", "line_len", "slow")]))
        X = np.empty((n, mf + 1), np.float32)
        if n:
            check(lib().rl_letor_rows(h, X.ctypes.data, mf + 1))
        out["X"] = X
        return out
    finally:
        lib().rl_letor_destroy(h)


def letor_format(X, row_len, labels, strings, qid_off, qid_len, desc_off, desc_len, buf=None):
    """Native LETOR writer (rl_letor_format): the text of DataPoint.toString plus a newline for every row of X [n][stride]; row i has
    row_len[i] cells (column 0 unused), its qid and description are (offset, length) into the bytes `strings`.  Returns the text as a
    uint8 array.  buf: a uint8 array to format into (reused by a caller that writes chunk after chunk; the result is then a view of it);
    when it is too small the call is repeated with the size the first one reported."""
    X = np.ascontiguousarray(X, np.float32)
    n, stride = X.shape
    row_len, qid_len, desc_len = (np.ascontiguousarray(a, np.int32) for a in (row_len, qid_len, desc_len))
    qid_off, desc_off = np.ascontiguousarray(qid_off, np.int64), np.ascontiguousarray(desc_off, np.int64)
    labels = np.ascontiguousarray(labels, np.float32)
    if not (len(row_len) == len(labels) == len(qid_off) == len(qid_len) == len(desc_off) == len(desc_len) == n):
        raise RankLibError("rlhip: letor_format takes one entry per row in every array")
    need = C.c_int64(0)
    while True:
        cap = 0 if buf is None else buf.size
        check(lib().rl_letor_format(X.ctypes.data, n, stride, row_len.ctypes.data, labels.ctypes.data, strings, len(strings), qid_off.ctypes.data,
                                    qid_len.ctypes.data, desc_off.ctypes.data, desc_len.ctypes.data, None if buf is None else buf.ctypes.data,
                                    cap, C.byref(need)))
        if need.value <= cap:
            return buf[:need.value] if buf is not None else np.empty(0, np.uint8)      # a view of buf: written out before the next call
        buf = np.empty(need.value, np.uint8)


def debug_float_chain(x, seg_start=None, device=0):
    """Java float running sums of the segments of x on the GPU (rl_chain.inc); returns (float32 sums, int32[4] stats)."""
    x = np.ascontiguousarray(x, np.float64)
    seg = np.ascontiguousarray([0, len(x)] if seg_start is None else seg_start, np.int64)
    out = np.zeros(len(seg) - 1, np.float32)
    stats = np.zeros(4, np.int32)
    check(lib().rl_debug_float_chain(device, x.ctypes.data, len(x), seg.ctypes.data, len(seg) - 1, out.ctypes.data, stats.ctypes.data))
    return out, stats


def debug_fast_sum(x, seg_start=None, device=0):
    """RL_FLAG_FAST_LEAF's fixed f64 reduction R of the segments of x on the GPU (rl_fast_leaf.inc, the trainer's two kernels over the
    identity list); returns (float64 R per segment, its float32 rounding)."""
    x = np.ascontiguousarray(x, np.float64)
    seg = np.ascontiguousarray([0, len(x)] if seg_start is None else seg_start, np.int64)
    out64 = np.zeros(len(seg) - 1, np.float64)
    out32 = np.zeros(len(seg) - 1, np.float32)
    check(lib().rl_debug_fast_sum(device, x.ctypes.data, len(x), seg.ctypes.data, len(seg) - 1, out64.ctypes.data, out32.ctypes.data))
    return out64, out32


def set_err_max(max_gain):
    """ERRScorer.MAX for trainers created afterwards (rl_set_err_max)"""
    check(lib().rl_set_err_max(float(max_gain)))


def membench(mode, nbytes, stride=1, iters=10, device=0):
    """rl_debug_membench: (avg ms per launch, algorithmic bytes per launch); mode: 0 copy, 1 read, 2 write, 3 32-byte row gather;
    4..9 LDS atomics (consecutive bins / random bins / same address / random + count / three 32-bit / one 32-bit): nbytes = atomic groups per thread, returns (ms, groups per launch)"""
    ms, b = C.c_double(0), C.c_double(0)
    check(lib().rl_debug_membench(device, mode, nbytes, stride, iters, C.byref(ms), C.byref(b)))
    return ms.value, b.value


class Trainer:
    """Thin object wrapper over the rl_trainer handle (one GPU)."""

    def __init__(self, n_trees=1000, n_leaves=10, learning_rate=0.1, n_threshold=256, min_leaf_support=1,
                 early_stop_rounds=100, metric_k=10, device=0, flags=0, metric="NDCG", ranker="LAMBDAMART",
                 feature_sampling_rate=1.0, seed=0):
        L = lib()
        self.p = RlParams()
        L.rl_params_default(C.byref(self.p))
        self.p.n_trees, self.p.n_leaves, self.p.learning_rate = n_trees, n_leaves, learning_rate
        self.p.n_threshold, self.p.min_leaf_support, self.p.early_stop_rounds = n_threshold, min_leaf_support, early_stop_rounds
        self.p.metric_k, self.p.device, self.p.flags = metric_k, device, flags
        self.p.feature_sampling_rate, self.p.seed = feature_sampling_rate, seed
        self.p.metric, self.p.ranker = RL_METRIC[metric.upper()], RL_RANKER[ranker.upper()]
        self.h = C.c_void_p()
        check(L.rl_create(C.byref(self.p), C.byref(self.h)))
        self.cap = max(3, 2 * n_leaves - 1)          # the root always splits once (RegressionTree.java:62-67); -leaf -1: set_train sizes it
        self.N = self.F = self.Q = 0
        self.Nv = 0
        self.has_valid = False

    @staticmethod
    def _prep(X, labels, qoff, qkey, F=None):
        X = np.ascontiguousarray(X, dtype=np.float32)
        if X.ndim != 2:
            raise RankLibError("X must be [n_docs, n_features]")
        labels = np.ascontiguousarray(labels, dtype=np.float32)
        qoff = np.ascontiguousarray(qoff, dtype=np.int32)
        qk = None if qkey is None else np.ascontiguousarray(qkey, dtype=np.int32)
        return X, labels, qoff, qk

    def set_train(self, X, labels, qoff, feature_ids=None, qkey=None, chunk_rows=None):
        """chunk_rows: deliver the rows through rl_set_rows in blocks of that many documents (what the JNI shim does)"""
        X, labels, qoff, qk = self._prep(X, labels, qoff, qkey)
        fid = None if feature_ids is None else np.ascontiguousarray(feature_ids, dtype=np.int32)
        self.N, self.F = X.shape
        self.Q = len(qoff) - 1
        if self.p.n_leaves == -1:
            self.cap = max(3, 2 * max(1, self.N // max(1, self.p.min_leaf_support)) - 1)
        check(lib().rl_set_train(self.h, None if chunk_rows else X.ctypes.data, self.N, self.F, labels.ctypes.data, qoff.ctypes.data, self.Q,
                                 None if fid is None else fid.ctypes.data, None if qk is None else qk.ctypes.data))
        if chunk_rows:
            self.set_rows(X, False, chunk_rows)

    def set_rows(self, X, validation, chunk_rows):
        for a in range(0, X.shape[0], chunk_rows):
            blk = np.ascontiguousarray(X[a:a + chunk_rows])
            check(lib().rl_set_rows(self.h, 1 if validation else 0, a, blk.shape[0], blk.ctypes.data))

    def set_external_judgments(self, validation, ideal_dcg=None, rel_doc_count=None):
        """-qrel: per list, its qid's idealGains entry from the judgment file (NaN = none) / its relDocCount (0 = qid not in the file)"""
        idl = None if ideal_dcg is None else np.ascontiguousarray(ideal_dcg, dtype=np.float64)
        rdc = None if rel_doc_count is None else np.ascontiguousarray(rel_doc_count, dtype=np.int32)
        check(lib().rl_set_external_judgments(self.h, 1 if validation else 0, None if idl is None else idl.ctypes.data,
                                              None if rdc is None else rdc.ctypes.data))

    def set_validation(self, X, labels, qoff, qkey=None):
        X, labels, qoff, qk = self._prep(X, labels, qoff, qkey)
        if X.shape[1] != self.F:
            raise RankLibError("validation set must have the training set's feature columns")
        self.Nv = X.shape[0]
        check(lib().rl_set_validation(self.h, X.ctypes.data, self.Nv, labels.ctypes.data, qoff.ctypes.data,
                                      len(qoff) - 1, None if qk is None else qk.ctypes.data))
        self.has_valid = True

    def dist_unique_id(self):
        """128 bytes for ncclCommInitRank: call on rank 0, broadcast out of band"""
        buf = C.create_string_buffer(128)
        check(lib().rl_dist_unique_id(buf))
        return buf.raw

    def dist_init(self, uid, rank, n_ranks):
        """RCCL transport; every rank passes ITS shard of the queries to set_train (before init)"""
        check(lib().rl_dist_init(self.h, uid, rank, n_ranks))

    def dist_stats(self):
        """[all-reduce calls, all-reduce bytes, all-gather calls, all-gather bytes received, all-to-all calls, all-to-all bytes received from
        other ranks, calls / bytes received of the lazy tie-break's exchanges] of this rank so far"""
        out = np.zeros(8, np.int64)
        check(lib().rl_dist_stats(self.h, out.ctypes.data))
        return out

    def dist_init_callback(self, rank, n_ranks, allreduce, allgather, alltoallv=None):
        """host transport: allreduce(np_array, op) reduces in place, allgather(np_uint8_in) -> np_uint8 [n_ranks*len],
        alltoallv(list of n_ranks np_uint8 arrays to send, list of n_ranks byte counts to receive) -> list of n_ranks np_uint8 arrays received
        (None: emulated with all-gathers)"""
        def _ar(user, ptr, count, dtype, op):
            try:
                arr = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), (count * np.dtype(DT_NUMPY[dtype]).itemsize,)).view(DT_NUMPY[dtype])
                allreduce(arr, op)
                return 0
            except Exception as e:          # noqa: BLE001 -- must not propagate through the C frame
                print("host all-reduce callback failed:", e)
                return 1

        def _ag(user, pin, pout, nbytes):
            try:
                src = np.ctypeslib.as_array(C.cast(pin, C.POINTER(C.c_uint8)), (nbytes,))
                dst = np.ctypeslib.as_array(C.cast(pout, C.POINTER(C.c_uint8)), (nbytes * n_ranks,))
                dst[:] = allgather(src)
                return 0
            except Exception as e:          # noqa: BLE001
                print("host all-gather callback failed:", e)
                return 1

        def _aa(user, psend, scount, sdispl, precv, rcount, rdispl):
            try:
                sb = max([sdispl[p] + scount[p] for p in range(n_ranks)] + [1])
                rb = max([rdispl[p] + rcount[p] for p in range(n_ranks)] + [1])
                snd = np.ctypeslib.as_array(C.cast(psend, C.POINTER(C.c_uint8)), (sb,))
                rcv = np.ctypeslib.as_array(C.cast(precv, C.POINTER(C.c_uint8)), (rb,))
                got = alltoallv([snd[sdispl[p]:sdispl[p] + scount[p]] for p in range(n_ranks)], [int(rcount[p]) for p in range(n_ranks)])
                for p in range(n_ranks):
                    if len(got[p]) != rcount[p]:
                        raise ValueError("rank %d sent %d bytes, %d expected" % (p, len(got[p]), rcount[p]))
                    rcv[rdispl[p]:rdispl[p] + rcount[p]] = got[p]
                return 0
            except Exception as e:          # noqa: BLE001
                print("host all-to-all callback failed:", e)
                return 1
        self._cb = (HOST_ALLREDUCE(_ar), HOST_ALLGATHER(_ag), HOST_ALLTOALLV(_aa) if alltoallv is not None else HOST_ALLTOALLV())      # keep alive; HOST_ALLTOALLV() is a NULL pointer
        check(lib().rl_dist_init_callback(self.h, rank, n_ranks, self._cb[0], self._cb[1], self._cb[2], None))

    def init(self):
        check(lib().rl_init(self.h))
        cap = C.c_int32(0)
        check(lib().rl_tree_capacity(self.h, C.byref(cap)))      # -leaf -1: 2 * floor(N_global / mls) - 1
        self.cap = cap.value

    def boost_round(self, want_tree=True):
        t = FlatTree(self.cap) if want_tree else None
        ct = t.c() if t else None
        tm, vm, stop = C.c_float(0), C.c_float(0), C.c_int32(0)
        check(lib().rl_boost_round(self.h, C.byref(ct) if t else None, C.byref(tm), C.byref(vm), C.byref(stop)))
        if t:
            t.n_nodes = ct.n_nodes
        return t, np.float32(tm.value), (np.float32(vm.value) if self.has_valid else None), bool(stop.value)

    def adopt_model_text(self, text, scratch_bytes=0):
        """resume: the trees of `text` (what model_text() wrote) become this trainer's first rounds, replayed on its data; after
        init(), before the first round.  Returns the early-stop test at the last adopted round; round_metrics(r) holds the adopted rounds' values"""
        if not hasattr(lib(), "rl_adopt_model_text"):
            raise RankLibError("this librlhip.so has no rl_adopt_model_text: it cannot resume")
        stop = C.c_int32(0)
        check(lib().rl_adopt_model_text(self.h, None if text is None else text.encode("ascii"), scratch_bytes, C.byref(stop)))
        return bool(stop.value)

    def refit_model_text(self, text, decay=0.0):
        """refit: the trees of `text` keep their structure and get new leaf values from this trainer's data, blended with the old ones
        by `decay` in [0, 1) (0: the new values alone); after init(), before the first round.  Returns the early-stop test at the last refit
        round; round_metrics(r) holds the refit rounds' values, boost_round() goes on behind them"""
        if not hasattr(lib(), "rl_refit_model_text"):
            raise RankLibError("this librlhip.so has no rl_refit_model_text: it cannot refit")
        stop = C.c_int32(0)
        check(lib().rl_refit_model_text(self.h, None if text is None else text.encode("ascii"), float(decay), C.byref(stop)))
        return bool(stop.value)

    def refit_stats(self):
        """rl_debug_refit_stats: (routing launches through the LDS tile, routing launches from global memory, leaves that kept their old output)"""
        out = (C.c_int64 * 3)()
        check(lib().rl_debug_refit_stats(self.h, out))
        return tuple(int(v) for v in out)

    def boost_rounds_async(self, n):
        check(lib().rl_boost_rounds_async(self.h, n))

    def sync(self):
        check(lib().rl_sync(self.h))

    def finish(self):
        ts, vs = C.c_double(0), C.c_double(0)
        check(lib().rl_finish(self.h, C.byref(ts), C.byref(vs)))
        return ts.value, (vs.value if self.has_valid else None)

    def num_trees(self):
        n = C.c_int32(0)
        check(lib().rl_num_trees(self.h, C.byref(n)))
        return n.value

    def get_tree(self, i):
        t = FlatTree(self.cap)
        ct = t.c()
        check(lib().rl_get_tree(self.h, i, C.byref(ct)))
        t.n_nodes = ct.n_nodes
        return t

    def round_metrics(self, r):
        tm, vm = C.c_float(0), C.c_float(0)
        check(lib().rl_get_round_metrics(self.h, r, C.byref(tm), C.byref(vm)))
        return np.float32(tm.value), (np.float32(vm.value) if self.has_valid else None)

    def best_validation(self):
        b, s = C.c_int32(0), C.c_double(0)
        check(lib().rl_best_validation(self.h, C.byref(b), C.byref(s)))
        return b.value, s.value

    def predict(self, X):
        X = np.ascontiguousarray(X, dtype=np.float32)
        out = np.zeros(X.shape[0], np.float32)
        check(lib().rl_predict(self.h, X.ctypes.data, X.shape[0], out.ctypes.data))
        return out

    def model_text(self):
        need = C.c_int64(0)
        check(lib().rl_model_to_text(self.h, None, 0, C.byref(need)))
        buf = C.create_string_buffer(need.value)
        check(lib().rl_model_to_text(self.h, buf, need.value, C.byref(need)))
        return buf.value.decode("ascii")

    def bin_stride(self):
        s = C.c_int32(0)
        check(lib().rl_bin_stride(self.h, C.byref(s)))
        return s.value

    def quant_exponent(self):
        e = C.c_int32(0)
        check(lib().rl_quant_exponent(self.h, C.byref(e)))
        return e.value

    def hist_features(self):
        """(number of histogram features, column behind each): the data set's features unless a threshold table has more than 4095 entries (rlhip.h)"""
        n = C.c_int32(0)
        check(lib().rl_hist_features(self.h, C.byref(n), None, 0))
        cols = np.zeros(n.value, np.int32)
        check(lib().rl_hist_features(self.h, C.byref(n), cols.ctypes.data_as(C.POINTER(C.c_int32)), n.value))
        return n.value, cols

    def array(self, name):
        which = ARR[name]
        TS = self.bin_stride()
        F_hist = self.hist_features()[0] if name in ("NBINS", "THRESHOLDS", "BINS", "ROOT_COUNT", "ROOT_SUM", "ROOT_SUM_FIXED", "ROOT_SUM_JAVA") else self.F
        shapes = {
            "LAMBDA": ((self.N,), np.float64), "WEIGHT": ((self.N,), np.float64), "SCORE": ((self.N,), np.float64),
            "VALID_SCORE": ((self.Nv,), np.float64), "NBINS": ((F_hist,), np.int32),
            "THRESHOLDS": ((F_hist, TS), np.float32), "BINS": ((F_hist, self.N), np.uint16),
            "ROOT_COUNT": ((F_hist, TS), np.int32), "ROOT_SUM": ((F_hist, TS), np.float64), "ROOT_SUM_JAVA": ((F_hist, TS), np.float64),
            "QUANT": ((self.N,), np.int64), "ROOT_SUM_FIXED": ((F_hist, TS, 2), np.int64),
            "NDCG_PER_QUERY": ((self.Q,), np.float64), "CHAIN_STATS": ((6,), np.int32), "GROW_STATS": ((4,), np.int32), "GROW_DOCS": ((4,), np.int64), "BUBBLES": ((4,), np.int64), "PIECE_STATS": ((2,), np.int64), "SPARSE_INFO": ((8,), np.int64), "PHASE_CLOCKS": ((64, 32), np.int64), "BLOCK_TRACE": ((64, 3, 2048, 8), np.int64), "STEP_LOG": ((8 + 8 * 8192,), np.int32), "TIE_STATS": ((10,), np.int64), "LAUNCH_ARMS": ((ARM["COUNT_"],), np.int64), "CHAIN_MISS": ((2, self.cap + 1), np.int32),
        }
        shape, dt = shapes[name]
        out = np.zeros(shape, dt)
        check(lib().rl_get_array(self.h, which, out.ctypes.data, out.nbytes))
        return out

    def timing(self, kernel):
        ms, n, b = C.c_double(0), C.c_int64(0), C.c_double(0)
        check(lib().rl_get_timing(self.h, KERNEL[kernel], C.byref(ms), C.byref(n), C.byref(b)))
        return ms.value, n.value, b.value

    def reset_timing(self):
        check(lib().rl_reset_timing(self.h))

    def set_timing_flags(self, flags):
        check(lib().rl_set_timing_flags(self.h, flags))

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            lib().rl_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


MODEL_PATH_NONE, MODEL_PATH_TILED, MODEL_PATH_GENERIC = 0, 1, 2
MODEL_PATH_PERMUTED = 3             # rl_model_predict_permuted / rl_model_eval_permuted: one kernel for every model
PERMUTED_BATCH = 16                 # RL_PERMUTED_BATCH (rlhip.h): cells k_model_permuted_scores takes per document at a time
MODEL_PATH_COVER, MODEL_PATH_CONTRIBS = 4, 5      # rl_model_cover (k_model_cover) / rl_model_predict_contribs (k_model_contribs)
MODEL_PATH_SHAP = 6                               # rl_model_predict_shap (k_model_shap)
MODEL_PATH_PARTIAL = 7                            # rl_model_predict_partial (k_model_partial_scores, k_partial_reduce)
MODEL_PATH_INTERACT = 8                           # rl_model_predict_interactions (k_model_shap, k_model_interact, k_interact_finish)
PARTIAL_BATCH = 16                                # RL_PARTIAL_BATCH (rlhip.h): cells of one column k_model_partial_scores takes per document at a time
PARTIAL_SUM_BLOCK = 256                           # RL_PARTIAL_SUM_BLOCK (rlhip.h): the documents of one partial sum, part of the definition


class Model:
    """A scoring-only ensemble loaded from RankLib model text (rl_model_*)."""

    def __init__(self, text, device=0):
        self.h = C.c_void_p()
        check(lib().rl_model_from_text(text.encode("ascii"), device, C.byref(self.h)))

    def num_trees(self):
        n = C.c_int32(0)
        check(lib().rl_model_num_trees(self.h, C.byref(n)))
        return n.value

    def features(self):
        n = C.c_int32(0)
        check(lib().rl_model_features(self.h, None, 0, C.byref(n)))
        ids = np.zeros(max(1, n.value), np.int32)
        check(lib().rl_model_features(self.h, ids.ctypes.data, n.value, C.byref(n)))
        return ids[:n.value]

    def predict_rows(self, rows):
        """rows[:, f] holds feature ID f (column 0 unused, like DataPoint.fVals)"""
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        out = np.zeros(rows.shape[0], np.float32)
        check(lib().rl_model_predict(self.h, rows.ctypes.data, rows.shape[0], rows.shape[1], out.ctypes.data))
        return out

    def predict_device(self, dX_ptr, n_docs, row_stride, dOut_ptr, stream=None):
        """rows / scores are device pointers (e.g. torch tensors' data_ptr()); enqueued, not synchronised"""
        check(lib().rl_model_predict_device(self.h, C.c_void_p(dX_ptr), n_docs, row_stride, C.c_void_p(dOut_ptr),
                                            C.c_void_p(stream) if stream else None))

    @staticmethod
    def _stage_args(rows, stages):
        L = lib()
        if not hasattr(L, "rl_model_eval_stages"):
            raise RankLibError("rlhip: this librlhip.so has no staged evaluation (rl_model_eval_stages)")
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        st = np.ascontiguousarray(stages, dtype=np.int32)
        if rows.ndim != 2 or st.ndim != 1:
            raise RankLibError("rlhip: staged evaluation takes rows [n_docs][row_stride] and stages [n_stages]")
        return L, rows, st

    def predict_stages(self, rows, stages):
        """rl_model_predict_stages: f32 [len(stages)][n_docs], the scores of the model's first stages[i] trees (stages: tree counts,
        strictly increasing, each in [1, num_trees()]); rows as in predict_rows"""
        L, rows, st = self._stage_args(rows, stages)
        out = np.zeros((st.size, rows.shape[0]), np.float32)
        check(L.rl_model_predict_stages(self.h, rows.ctypes.data, rows.shape[0], rows.shape[1], st.ctypes.data, int(st.size), out.ctypes.data))
        return out

    def eval_stages(self, rows, labels, qoff, metric, k, stages, err_max=16.0, qkey=None, ideal_dcg=None, rel_doc_count=None, scratch_bytes=0):
        """rl_model_eval_stages: every list ranked and scored, as eval_lists does it, under the model's first stages[i] trees, all stages
        in one call.  Returns (f64 values [len(stages)][n_lists], uint8 NaN flags of the same shape -- a flagged cell holds 0.0 and was
        not ranked --, f64 ideal DCG per list, NaN unless the metric is NDCG).  The other arguments are eval_lists'."""
        L, rows, st = self._stage_args(rows, stages)
        m = str(metric).upper()
        if m not in RL_EVAL_METRIC:
            raise RankLibError("rlhip: eval_stages metric must be one of NDCG, DCG, MAP, ERR, P, RR, BEST (got %s)" % metric)
        lab = np.ascontiguousarray(labels, dtype=np.float32)
        qo = np.ascontiguousarray(qoff, dtype=np.int32)
        if lab.shape != (rows.shape[0],) or qo.ndim != 1 or qo.size < 1:
            raise RankLibError("rlhip: eval_stages takes rows [n_docs][row_stride], labels [n_docs] and qoff [n_lists + 1]")
        nl = int(qo.size) - 1

        def per_list(a, dtype, what):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dtype)
            if a.shape != (nl,):
                raise RankLibError("rlhip: eval_stages takes %s [n_lists]" % what)
            return a
        qk, idl, rdc = per_list(qkey, np.int32, "qkey"), per_list(ideal_dcg, np.float64, "ideal_dcg"), per_list(rel_doc_count, np.int32, "rel_doc_count")
        out = np.zeros((st.size, max(1, nl)), np.float64)
        nan = np.zeros((st.size, max(1, nl)), np.uint8)
        ideal = np.zeros(max(1, nl), np.float64)
        ptr = lambda a: None if a is None else a.ctypes.data      # noqa: E731
        check(L.rl_model_eval_stages(self.h, rows.ctypes.data, rows.shape[0], rows.shape[1], lab.ctypes.data, qo.ctypes.data, nl, ptr(qk),
                                     ptr(idl), ptr(rdc), RL_EVAL_METRIC[m], int(k), float(err_max), st.ctypes.data, int(st.size),
                                     int(scratch_bytes), out.ctypes.data, nan.ctypes.data, ideal.ctypes.data))
        return out[:, :nl], nan[:, :nl], ideal[:nl]

    @staticmethod
    def _permuted_args(rows, columns, donor):
        L = lib()
        if not hasattr(L, "rl_model_eval_permuted"):
            raise RankLibError("rlhip: this librlhip.so has no permuted evaluation (rl_model_eval_permuted)")
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        cols = np.ascontiguousarray(columns, dtype=np.int32)
        don = np.ascontiguousarray(donor, dtype=np.int32)
        if don.ndim == 1:
            don = don[None, :]
        if rows.ndim != 2 or cols.ndim != 1 or don.ndim != 2 or don.shape[1] != rows.shape[0]:
            raise RankLibError("rlhip: permuted evaluation takes rows [n_docs][row_stride], columns [n_columns] and donor [n_repeats][n_docs]")
        return L, rows, cols, np.ascontiguousarray(don)

    def predict_permuted(self, rows, columns, donor):
        """rl_model_predict_permuted: (f32 base scores [n_docs], f32 [len(columns)][n_repeats][n_docs]) -- cell (c, r) holds the scores of
        rows with column columns[c] of row i taken from row donor[r][i]; donor [n_repeats][n_docs] (or [n_docs]: one repeat), any map into
        [0, n_docs); rows as in predict_rows"""
        L, rows, cols, don = self._permuted_args(rows, columns, donor)
        base = np.zeros(rows.shape[0], np.float32)
        out = np.zeros((cols.size, don.shape[0], rows.shape[0]), np.float32)
        check(L.rl_model_predict_permuted(self.h, rows.ctypes.data, rows.shape[0], rows.shape[1], cols.ctypes.data, int(cols.size), don.ctypes.data,
                                          int(don.shape[0]), base.ctypes.data, out.ctypes.data))
        return base, out

    def eval_permuted(self, rows, labels, qoff, metric, k, columns, donor, err_max=16.0, qkey=None, ideal_dcg=None, rel_doc_count=None,
                      scratch_bytes=0):
        """rl_model_eval_permuted: every list ranked and scored, as eval_lists does it, under the unpermuted rows and under every
        (column, repeat) cell of predict_permuted, in one call.  Returns (f64 base values [n_lists], uint8 base NaN flags [n_lists],
        f64 values [len(columns)][n_repeats][n_lists], uint8 NaN flags of the same shape -- a flagged cell holds 0.0 and was not ranked --,
        f64 ideal DCG per list, NaN unless the metric is NDCG).  The other arguments are eval_lists'."""
        L, rows, cols, don = self._permuted_args(rows, columns, donor)
        m = str(metric).upper()
        if m not in RL_EVAL_METRIC:
            raise RankLibError("rlhip: eval_permuted metric must be one of NDCG, DCG, MAP, ERR, P, RR, BEST (got %s)" % metric)
        lab = np.ascontiguousarray(labels, dtype=np.float32)
        qo = np.ascontiguousarray(qoff, dtype=np.int32)
        if lab.shape != (rows.shape[0],) or qo.ndim != 1 or qo.size < 1:
            raise RankLibError("rlhip: eval_permuted takes rows [n_docs][row_stride], labels [n_docs] and qoff [n_lists + 1]")
        nl = int(qo.size) - 1

        def per_list(a, dtype, what):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dtype)
            if a.shape != (nl,):
                raise RankLibError("rlhip: eval_permuted takes %s [n_lists]" % what)
            return a
        qk, idl, rdc = per_list(qkey, np.int32, "qkey"), per_list(ideal_dcg, np.float64, "ideal_dcg"), per_list(rel_doc_count, np.int32, "rel_doc_count")
        w = max(1, nl)
        base, bnan = np.zeros(w, np.float64), np.zeros(w, np.uint8)
        out = np.zeros((cols.size, don.shape[0], w), np.float64)
        nan = np.zeros((cols.size, don.shape[0], w), np.uint8)
        ideal = np.zeros(w, np.float64)
        ptr = lambda a: None if a is None else a.ctypes.data      # noqa: E731
        check(L.rl_model_eval_permuted(self.h, rows.ctypes.data, rows.shape[0], rows.shape[1], lab.ctypes.data, qo.ctypes.data, nl, ptr(qk),
                                       ptr(idl), ptr(rdc), RL_EVAL_METRIC[m], int(k), float(err_max), cols.ctypes.data, int(cols.size),
                                       don.ctypes.data, int(don.shape[0]), int(scratch_bytes), base.ctypes.data, bnan.ctypes.data,
                                       out.ctypes.data, nan.ctypes.data, ideal.ctypes.data))
        return base[:nl], bnan[:nl], out[:, :, :nl], nan[:, :, :nl], ideal[:nl]

    @staticmethod
    def _contrib_rows(rows):
        L = lib()
        if not hasattr(L, "rl_model_predict_contribs"):
            raise RankLibError("rlhip: this librlhip.so has no feature contributions (rl_model_predict_contribs)")
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        if rows.ndim != 2:
            raise RankLibError("rlhip: feature contributions take rows [n_docs][row_stride]")
        return L, rows, (rows if rows.size else np.zeros(1, np.float32))      # (no rows: still a pointer that is not null)

    def cover(self, rows, accumulate=False):
        """rl_model_cover: count, per node, the rows of a background file whose walk visits it, and make the node values from the counts
        (DESIGN.md 26).  accumulate: add to the counts of earlier calls instead of replacing them.  rows as in predict_rows."""
        L, rows, buf = self._contrib_rows(rows)
        check(L.rl_model_cover(self.h, buf.ctypes.data, rows.shape[0], rows.shape[1], 1 if accumulate else 0))

    def cover_rows(self):
        """rl_model_cover_rows: the background rows counted so far"""
        n = C.c_int64(0)
        check(lib().rl_model_cover_rows(self.h, C.byref(n)))
        return n.value

    def cover_of(self, tree):
        """rl_model_get_cover: (uint64 covers, float64 node values) of the nodes of one tree, in the pre-order of the model text"""
        L, n = lib(), C.c_int32(0)
        L.rl_model_get_cover(self.h, int(tree), None, None, -1, C.byref(n))       # (refused: cap is below; the node count is still set)
        counts, values = np.zeros(max(1, n.value), np.uint64), np.zeros(max(1, n.value), np.float64)
        check(L.rl_model_get_cover(self.h, int(tree), counts.ctypes.data, values.ctypes.data, n.value, C.byref(n)))
        return counts[:n.value], values[:n.value]

    def predict_contribs(self, rows, columns=None, scratch_bytes=0):
        """rl_model_predict_contribs: (float64 [n_docs][C + 2], the C column ids).  Column c < C holds the contribution of feature
        columns[c] to every row's score, column C what the features not asked for contribute, column C + 1 the bias: Saabas path
        attribution over the covers of the last cover() calls.  columns=None: the model's features(), and column C is +0.0.  A row's
        columns sum to the f64 sum of its weighted leaf outputs -- predict_rows' float chain up to float rounding."""
        return self._predict_slots("rl_model_predict_contribs", rows, columns, scratch_bytes)

    def predict_shap(self, rows, columns=None, scratch_bytes=0):
        """rl_model_predict_shap: predict_contribs' layout with exact path-dependent TreeSHAP values in place of Saabas' path attribution
        (DESIGN.md 27): every row meets every leaf of every tree, about two orders of magnitude more work."""
        if not hasattr(lib(), "rl_model_predict_shap"):
            raise RankLibError("rlhip: this librlhip.so has no exact contributions (rl_model_predict_shap)")
        return self._predict_slots("rl_model_predict_shap", rows, columns, scratch_bytes)

    def shap_limits(self):
        """rl_model_shap_limits: (the most distinct features on one root-to-leaf path of the model, the most predict_shap takes)"""
        d, p = C.c_int32(0), C.c_int32(0)
        check(lib().rl_model_shap_limits(self.h, C.byref(d), C.byref(p)))
        return d.value, p.value

    def predict_interactions(self, rows, columns=None, scratch_bytes=0):
        """rl_model_predict_interactions: (float64 [n_docs][C + 2][C + 2], the C column ids) -- SHAP interaction values.
        Cell [i][j], i != j, is what features ids[i] and ids[j] do together that neither does alone, i the conditioned and j the
        attributed slot; the diagonal is the SHAP value of predict_shap less the row's other cells, so row i sums to it; [C + 1][C + 1]
        is the bias, the rest of its row and column +0.0.  About the mean element count of a leaf times predict_shap's work."""
        if not hasattr(lib(), "rl_model_predict_interactions"):
            raise RankLibError("rlhip: this librlhip.so has no interaction values (rl_model_predict_interactions)")
        return self._predict_slots("rl_model_predict_interactions", rows, columns, scratch_bytes, square=True)

    def _predict_slots(self, entry, rows, columns, scratch_bytes, square=False):
        L, rows, buf = self._contrib_rows(rows)
        if columns is None:
            ids, cols, nc = [int(f) for f in self.features()], None, 0
        else:
            cols = np.ascontiguousarray(columns, dtype=np.int32)
            if cols.ndim != 1:
                raise RankLibError("rlhip: feature contributions take columns [n_columns]")
            ids, nc = [int(c) for c in cols], int(cols.size)
            if not nc:
                cols = np.zeros(1, np.int32)          # (an empty list is refused by the library, by name: it must not arrive as NULL)
        out = np.zeros((rows.shape[0],) + (len(ids) + 2,) * (2 if square else 1), np.float64)
        obuf = out if out.size else np.zeros(1, np.float64)
        check(getattr(L, entry)(self.h, buf.ctypes.data, rows.shape[0], rows.shape[1], None if cols is None else cols.ctypes.data, nc,
                                int(scratch_bytes), obuf.ctypes.data))
        return out, ids

    def leaf_sums(self, rows):
        """rl_model_predict_leaf_sums: float64 [n_docs], per row the f64 sum of weight * leaf output over the trees -- what the row's
        contributions sum to up to f64 rounding"""
        L, rows, buf = self._contrib_rows(rows)
        out = np.zeros(max(1, rows.shape[0]), np.float64)
        check(L.rl_model_predict_leaf_sums(self.h, buf.ctypes.data, rows.shape[0], rows.shape[1], out.ctypes.data))
        return out[:rows.shape[0]]

    def predict_partial(self, rows, columns, grids, ice=False, scratch_bytes=0):
        """rl_model_predict_partial: partial dependence and ICE curves.  grids: one array of f32 grid values per entry of
        columns, each strictly ascending; cell j is the j-th value of the grids laid end to end.  Returns (f32 base scores [n_docs],
        f64 mean [cells] -- the partial-dependence values --, f64 shift2 [cells], the mean squared move away from the base, and f32
        ice [cells][n_docs] or None): cell j holds the scores of rows, padded with zeros to any width, with its column set to its grid
        value.  The sums take the fixed order of include/rlhip.h; rows as in predict_rows."""
        L = lib()
        if not hasattr(L, "rl_model_predict_partial"):
            raise RankLibError("rlhip: this librlhip.so has no partial dependence (rl_model_predict_partial)")
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        cols = np.ascontiguousarray(columns, dtype=np.int32)
        gs = [np.ascontiguousarray(g, dtype=np.float32) for g in grids]
        if rows.ndim != 2 or cols.ndim != 1 or len(gs) != cols.size or any(g.ndim != 1 for g in gs):
            raise RankLibError("rlhip: partial dependence takes rows [n_docs][row_stride], columns [n_columns] and one 1-d grid per column")
        off = np.zeros(cols.size + 1, np.int32)
        np.cumsum([g.size for g in gs], out=off[1:])
        grid = np.concatenate(gs + [np.zeros(1, np.float32)])      # (never an empty buffer: the library names what is wrong)
        cells = int(off[-1])
        base = np.zeros(max(1, rows.shape[0]), np.float32)
        mean, shift2 = np.zeros(max(1, cells), np.float64), np.zeros(max(1, cells), np.float64)
        out = np.zeros((cells, rows.shape[0]), np.float32) if ice else None
        buf = rows if rows.size else np.zeros(1, np.float32)
        cbuf = cols if cols.size else np.zeros(1, np.int32)
        check(L.rl_model_predict_partial(self.h, buf.ctypes.data, rows.shape[0], rows.shape[1], cbuf.ctypes.data, int(cols.size), off.ctypes.data,
                                         grid.ctypes.data, int(scratch_bytes), base.ctypes.data, mean.ctypes.data, shift2.ctypes.data,
                                         out.ctypes.data if ice and out.size else None))
        return base[:rows.shape[0]], mean[:cells], shift2[:cells], out

    def path(self):
        """MODEL_PATH_* of the last predict call: which kernel it took"""
        p = C.c_int32(0)
        check(lib().rl_model_debug_path(self.h, C.byref(p)))
        return p.value

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            lib().rl_model_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


NET_PATH_NONE, NET_PATH_LDS, NET_PATH_GLOBAL = 0, 1, 2


class NetModel:
    """A scoring-only neural network on the device (rl_net_*): the forward pass of RankNet, LambdaRank and ListNet models.
    weights: per layer l = 1 .. len(hidden_sizes) + 1 a row-major [n_l][n_{l-1} + 1] matrix, row j = neuron j's inLinks with the
    bias last (the input order of include/rlhip.h, not a model file's)."""

    def __init__(self, feature_ids, hidden_sizes, weights, device=0):
        L = lib()
        if not hasattr(L, "rl_net_create"):
            raise RankLibError("rlhip: this librlhip.so has no neural-net scoring (rl_net_*)")
        fid = np.ascontiguousarray(feature_ids, dtype=np.int32)
        hid = np.ascontiguousarray(hidden_sizes, dtype=np.int32)
        w = np.ascontiguousarray(weights, dtype=np.float64)
        keep = hid if hid.size else np.zeros(1, np.int32)
        self.h = C.c_void_p()
        check(L.rl_net_create(int(device), fid.ctypes.data if fid.size else None, fid.size, keep.ctypes.data, hid.size,
                              w.ctypes.data if w.size else None, w.size, C.byref(self.h)))

    def predict_rows(self, rows):
        """rows[:, f] holds feature ID f (column 0 unused, like DataPoint.fVals); f64 scores"""
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        out = np.zeros(rows.shape[0], np.float64)
        check(lib().rl_net_predict(self.h, rows.ctypes.data, rows.shape[0], rows.shape[1], out.ctypes.data))
        return out

    def predict_device(self, dX_ptr, n_docs, row_stride, dOut_ptr, stream=None):
        """rows (f32) / scores (f64) are device pointers (e.g. torch tensors' data_ptr()); enqueued, not synchronised"""
        check(lib().rl_net_predict_device(self.h, C.c_void_p(dX_ptr), n_docs, row_stride, C.c_void_p(dOut_ptr),
                                          C.c_void_p(stream) if stream else None))

    def path(self):
        """NET_PATH_* of the last predict call: which kernel variant it took"""
        p = C.c_int32(0)
        check(lib().rl_net_debug_path(self.h, C.byref(p)))
        return p.value

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            lib().rl_net_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _LinearTrainer:
    """What the handles of the four linear rankers and of ListNet training share (rl_linear.inc): a subclass names its C prefix, the ranker as the messages call
    it and its trace records, and fills its own parameters."""
    _prefix = _name = _trace_dtype = None

    def _fn(self, name):
        return getattr(lib(), self._prefix + name)

    def _open(self, params, metric, metric_k, device, err_max, **own):
        """creates the handle: the ranker's defaults, the common parameters, then its own"""
        self.p = params()
        self._fn("params_default")(C.byref(self.p))
        m = metric.upper()
        if m not in RL_CA_METRIC:
            raise RankLibError("rlhip: the %s train metric must be one of NDCG, DCG, MAP, ERR, P, RR (got %s)" % (self._name, metric))
        self.p.metric, self.p.metric_k, self.p.device, self.p.err_max = RL_CA_METRIC[m], int(metric_k), int(device), float(err_max)
        for k, v in own.items():
            setattr(self.p, k, v)
        self.h = C.c_void_p()
        check(self._fn("create")(C.byref(self.p), C.byref(self.h)))
        self.F = self.Q = self.N = 0
        self.has_valid = False

    def set_train(self, X, labels, qoff, qkey=None):
        X, labels, qoff, qk = Trainer._prep(X, labels, qoff, qkey)
        self.F, self.Q, self.N = X.shape[1], len(qoff) - 1, X.shape[0]
        check(self._fn("set_train")(self.h, X.ctypes.data, X.shape[0], self.F, labels.ctypes.data, qoff.ctypes.data, len(qoff) - 1,
                                    None if qk is None else qk.ctypes.data))

    def set_validation(self, X, labels, qoff, qkey=None):
        X, labels, qoff, qk = Trainer._prep(X, labels, qoff, qkey)
        if X.shape[1] != self.F:
            raise RankLibError("validation set must have the training set's feature columns")
        check(self._fn("set_validation")(self.h, X.ctypes.data, X.shape[0], labels.ctypes.data, qoff.ctypes.data, len(qoff) - 1,
                                         None if qk is None else qk.ctypes.data))
        self.has_valid = True

    def set_external_judgments(self, validation, ideal_dcg=None, rel_doc_count=None):
        idl = None if ideal_dcg is None else np.ascontiguousarray(ideal_dcg, dtype=np.float64)
        rdc = None if rel_doc_count is None else np.ascontiguousarray(rel_doc_count, dtype=np.int32)
        check(self._fn("set_external_judgments")(self.h, 1 if validation else 0, None if idl is None else idl.ctypes.data,
                                                 None if rdc is None else rdc.ctypes.data))

    def learn(self):
        check(self._fn("learn")(self.h))

    def scores(self):
        ts, vs = C.c_double(0), C.c_double(0)
        check(self._fn("scores")(self.h, C.byref(ts), C.byref(vs)))
        return ts.value, (vs.value if self.has_valid else None)

    def trace(self):
        """structured array (the class's trace dtype) of what learn() did, in the Java's order"""
        n = C.c_int64(0)
        check(self._fn("trace")(self.h, None, 0, C.byref(n)))
        out = np.zeros(n.value, self._trace_dtype)
        if n.value:
            check(self._fn("trace")(self.h, out.ctypes.data, n.value, C.byref(n)))
        return out

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self._fn("destroy")(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CoorAscentTrainer(_LinearTrainer):
    """Thin object wrapper over the rl_ca handle: CoorAscent.learn() on one GPU (rl_ca.hip).
    trace(): CA_TRACE_DTYPE, one record per restart, pass, trial, success and validation score."""
    _prefix, _name, _trace_dtype = "rl_ca_", "Coordinate Ascent", CA_TRACE_DTYPE

    def __init__(self, n_restart=5, n_max_iteration=25, step_base=0.05, step_scale=2.0, tolerance=0.001, regularized=False, slack=0.001,
                 metric="NDCG", metric_k=10, device=0, seed=0, err_max=16.0):
        self._open(RlCaParams, metric, metric_k, device, err_max, n_restart=int(n_restart), n_max_iteration=int(n_max_iteration),
                   step_base=float(step_base), step_scale=float(step_scale), tolerance=float(tolerance),
                   regularized=1 if regularized else 0, slack=float(slack),
                   seed=((int(seed) + (1 << 63)) % (1 << 64)) - (1 << 63))      # a Java long

    def weights(self):
        w = np.zeros(max(1, self.F), np.float64)
        check(lib().rl_ca_get_weights(self.h, w.ctypes.data, len(w)))
        return w[:self.F]


class AdaRankTrainer(_LinearTrainer):
    """Thin object wrapper over the rl_ada handle: AdaRank.learn() on one GPU (rl_ada.inc in rl_ca.hip).
    trace(): ADA_TRACE_DTYPE, one record per phase start, round and rollback."""
    _prefix, _name, _trace_dtype = "rl_ada_", "AdaRank", ADA_TRACE_DTYPE

    def __init__(self, n_iteration=500, tolerance=0.002, train_with_enqueue=True, max_sel_count=5, metric="NDCG", metric_k=10, device=0,
                 err_max=16.0):
        self._open(RlAdaParams, metric, metric_k, device, err_max, n_iteration=int(n_iteration), tolerance=float(tolerance),
                   train_with_enqueue=1 if train_with_enqueue else 0, max_sel_count=int(max_sel_count))

    def model(self):
        """(feature indices, weights) of the final ensemble, in ensemble order (an index may repeat)"""
        n = C.c_int32(0)
        check(lib().rl_ada_get_model(self.h, None, None, 0, C.byref(n)))
        fid, w = np.zeros(max(1, n.value), np.int32), np.zeros(max(1, n.value), np.float64)
        check(lib().rl_ada_get_model(self.h, fid.ctypes.data, w.ctypes.data, n.value, C.byref(n)))
        return fid[:n.value], w[:n.value]

    def weak_table(self):
        """[F, Q] f64: scorer.score(WeakRanker(f).rank(list q)) as the GPU built it"""
        out = np.zeros((self.F, self.Q), np.float64)
        check(lib().rl_ada_debug_weak_table(self.h, out.ctypes.data, out.size))
        return out


class RankBoostTrainer(_LinearTrainer):
    """Thin object wrapper over the rl_rb handle: RankBoost.init() and learn() on one GPU (rl_rb.inc in rl_ca.hip).
    trace(): RB_TRACE_DTYPE, one record per round."""
    _prefix, _name, _trace_dtype = "rl_rb_", "RankBoost", RB_TRACE_DTYPE

    def __init__(self, n_iteration=300, n_threshold=10, metric="NDCG", metric_k=10, device=0, err_max=16.0, keep_potentials=0):
        self._open(RlRbParams, metric, metric_k, device, err_max, n_iteration=int(n_iteration), n_threshold=int(n_threshold),
                   keep_potentials=int(keep_potentials))

    def model(self):
        """(feature indices, thresholds, weights) of the final ensemble, in ensemble order (an index may repeat)"""
        n = C.c_int32(0)
        check(lib().rl_rb_get_model(self.h, None, None, None, 0, C.byref(n)))
        m = max(1, n.value)
        fid, thr, w = np.zeros(m, np.int32), np.zeros(m, np.float64), np.zeros(m, np.float64)
        check(lib().rl_rb_get_model(self.h, fid.ctypes.data, thr.ctypes.data, w.ctypes.data, n.value, C.byref(n)))
        return fid[:n.value], thr[:n.value], w[:n.value]

    def potentials(self, round):       # noqa: A002
        """[N] f64: the potentials of round `round` (1 .. keep_potentials), every list in getCorrectRanking()'s order"""
        out = np.zeros(self.N, np.float64)
        check(lib().rl_rb_debug_potentials(self.h, int(round), out.ctypes.data, out.size))
        return out


class LinearRegTrainer(_LinearTrainer):
    """Thin object wrapper over the rl_lr handle: LinearRegRank.learn() on one GPU (rl_lr.inc in rl_ca.hip).  It keeps no trace."""
    _prefix, _name = "rl_lr_", "Linear Regression"

    def __init__(self, lambda_=1E-10, metric="NDCG", metric_k=10, device=0, err_max=16.0):
        if not hasattr(lib(), "rl_lr_create"):
            raise RankLibError("rlhip: this librlhip.so has no Linear Regression (rl_lr_*)")
        self._open(RlLrParams, metric, metric_k, device, err_max, lambda_=float(lambda_))

    def set_train(self, X, labels, qoff, qkey=None):
        """X[:, f] = getFeatureValue(f + 1): the fit reads columns 0 .. nVar - 2, whatever the feature list says"""
        super().set_train(X, labels, qoff, qkey)

    def set_features(self, n_var=0, eval_cols=None):
        """n_var: the Java's nVar (0 = every column); eval_cols: the columns eval() reads (features[i] - 1; -1 reads 0), None = all"""
        cols = None if eval_cols is None else np.ascontiguousarray(eval_cols, dtype=np.int32)
        keep = np.zeros(1, np.int32) if cols is not None and cols.size == 0 else cols      # an empty list is still a list: a real pointer
        check(lib().rl_lr_set_features(self.h, int(n_var), None if keep is None else keep.ctypes.data, 0 if cols is None else cols.size))

    def weights(self):
        n = C.c_int32(0)
        check(lib().rl_lr_get_weights(self.h, None, 0, C.byref(n)))
        w = np.zeros(max(1, n.value), np.float64)
        check(lib().rl_lr_get_weights(self.h, w.ctypes.data, n.value, C.byref(n)))
        return w[:n.value]

    def gram(self):
        """(xTx [nVar, nVar], xTy [nVar]) as accumulated, before the ridge term"""
        n = C.c_int32(0)
        check(lib().rl_lr_debug_gram(self.h, None, None, 0, C.byref(n)))
        xtx, xty = np.zeros((n.value, n.value), np.float64), np.zeros(n.value, np.float64)
        check(lib().rl_lr_debug_gram(self.h, xtx.ctypes.data, xty.ctypes.data, n.value, C.byref(n)))
        return xtx, xty

    def times(self):
        """dict: gram_ms (device events), solve_ms, score_ms (host clocks) and the register block of the last learn()"""
        g, s, e, rb = C.c_double(0), C.c_double(0), C.c_double(0), C.c_int32(0)
        check(lib().rl_lr_debug_times(self.h, C.byref(g), C.byref(s), C.byref(e), C.byref(rb)))
        return dict(gram_ms=g.value, solve_ms=s.value, score_ms=e.value, register_block=rb.value)


class NoBestModelError(RankLibError):
    """rl_ln_learn / rl_rn_learn returned RL_ERR_NO_BEST: with a validation set, no epoch scored above 0.0 (learning.ListNet and RankNet
    turn it into the Java's message)"""


class ListNetTrainer(_LinearTrainer):
    """Thin object wrapper over the rl_ln handle: ListNet.learn() on one GPU (rl_ln.inc in rl_ca.hip).  The start weights are the
    caller's (set_weights: inputs in order, the bias last).  trace(): LN_TRACE_DTYPE, one record per epoch."""
    _prefix, _name, _trace_dtype = "rl_ln_", "ListNet", LN_TRACE_DTYPE

    def __init__(self, n_epochs=1500, learning_rate=0.00001, metric="NDCG", metric_k=10, device=0, err_max=16.0):
        if not hasattr(lib(), "rl_ln_create"):
            raise RankLibError("rlhip: this librlhip.so has no ListNet training (rl_ln_*)")
        self._open(RlLnParams, metric, metric_k, device, err_max, n_epochs=int(n_epochs), learning_rate=float(learning_rate))

    def set_weights(self, w):
        w = np.ascontiguousarray(w, dtype=np.float64)
        check(self._fn("set_weights")(self.h, w.ctypes.data, w.size))

    def learn(self):
        rc = self._fn("learn")(self.h)
        if rc == RL_ERR_NO_BEST:
            raise NoBestModelError("%s (rlhip status %d)" % (lib().rl_last_error().decode("utf-8", "replace"), rc))
        check(rc)

    def weights(self):
        n = C.c_int32(0)
        check(self._fn("get_weights")(self.h, None, 0, C.byref(n)))
        w = np.zeros(max(1, n.value), np.float64)
        check(self._fn("get_weights")(self.h, w.ctypes.data, n.value, C.byref(n)))
        return w[:n.value]

    def doc_scores(self, validation=False):
        """[N] f64: the final weights' output for every document of the set, as k_ln_score wrote it"""
        out = np.zeros(max(1, self.Nv if validation else self.N), np.float64)
        check(self._fn("debug_doc_scores")(self.h, 1 if validation else 0, out.ctypes.data, out.size))
        return out[:self.Nv if validation else self.N]

    def set_validation(self, X, labels, qoff, qkey=None):
        super().set_validation(X, labels, qoff, qkey)
        self.Nv = np.asarray(X).shape[0]

    def times(self):
        """dict: epoch_ms (all k_ln_epoch launches, device events), score_ms (scoring + ranking after every epoch, host clock)"""
        e, s = C.c_double(0), C.c_double(0)
        check(self._fn("debug_times")(self.h, C.byref(e), C.byref(s)))
        return dict(epoch_ms=e.value, score_ms=s.value)


class RankNetTrainer(ListNetTrainer):
    """Thin object wrapper over the rl_rn handle: RankNet.learn() on one GPU (rl_rn.inc in rl_ca.hip).  hidden_sizes: the hidden layers'
    neuron counts ([] = -layer 0).  The start weights are the caller's (set_weights, NetModel's layout: per layer a row-major
    [n_l][n_{l-1} + 1], the bias last); weights() returns the same layout.  trace(): RN_TRACE_DTYPE, one record per epoch.
    lambdarank=True: the handle trains LambdaRank (rl_rn_set_lambdarank: the lists re-ranked by the current weights, pairs in both
    directions weighted by the train metric's swap change; NDCG, DCG, MAP or ERR)."""
    _prefix, _name, _trace_dtype = "rl_rn_", "RankNet", RN_TRACE_DTYPE

    def __init__(self, n_epochs=100, learning_rate=0.00005, hidden_sizes=(10,), metric="NDCG", metric_k=10, device=0, err_max=16.0,
                 lambdarank=False):
        if not hasattr(lib(), "rl_rn_create"):
            raise RankLibError("rlhip: this librlhip.so has no RankNet training (rl_rn_*)")
        if lambdarank and not hasattr(lib(), "rl_rn_set_lambdarank"):
            raise RankLibError("rlhip: this librlhip.so has no LambdaRank training (rl_rn_set_lambdarank)")
        if lambdarank:
            self._name = "LambdaRank"
        self.hidden = [int(v) for v in hidden_sizes]
        hid = np.ascontiguousarray(self.hidden if self.hidden else [0], dtype=np.int32)      # a real pointer for an empty list too
        self._open(RlRnParams, metric, metric_k, device, err_max, n_epochs=int(n_epochs), learning_rate=float(learning_rate),
                   n_hidden=len(self.hidden), hidden_sizes=hid.ctypes.data_as(C.POINTER(C.c_int32)))
        if lambdarank:
            try:
                check(lib().rl_rn_set_lambdarank(self.h, 1))
            except RankLibError:
                self.close()
                raise


def _predict_arrays(feature_ids, weights, rows):
    """the predict functions' arguments as the library takes them, and the f64 scores to fill"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    return (rows, np.ascontiguousarray(feature_ids, dtype=np.int32), np.ascontiguousarray(weights, dtype=np.float64),
            np.zeros(rows.shape[0], np.float64))


def ca_predict(feature_ids, weights, rows, device=0):
    """CoorAscent.eval on the GPU: rows[:, f] holds feature ID f (column 0 unused, like DataPoint.fVals); f64 scores"""
    rows, fid, w, out = _predict_arrays(feature_ids, weights, rows)
    check(lib().rl_ca_predict(int(device), fid.ctypes.data, w.ctypes.data, len(w), rows.ctypes.data, rows.shape[0], rows.shape[1],
                              out.ctypes.data))
    return out


def rb_predict(feature_ids, thresholds, weights, rows, device=0):
    """RankBoost.eval on the GPU: rows as ca_predict's; f64 scores"""
    rows, fid, w, out = _predict_arrays(feature_ids, weights, rows)
    thr = np.ascontiguousarray(thresholds, dtype=np.float64)
    check(lib().rl_rb_predict(int(device), fid.ctypes.data, thr.ctypes.data, w.ctypes.data, len(w), rows.ctypes.data, rows.shape[0],
                              rows.shape[1], out.ctypes.data))
    return out


def lr_predict(feature_ids, weights, rows, device=0):
    """LinearRegRank.eval on the GPU: weights[-1] first, then weights[t] * rows[:, feature_ids[t]]; rows as ca_predict's; f64 scores"""
    L = lib()
    if not hasattr(L, "rl_lr_predict"):
        raise RankLibError("rlhip: this librlhip.so has no Linear Regression (rl_lr_*)")
    rows, fid, w, out = _predict_arrays(feature_ids, weights, rows)
    keep = fid if fid.size else np.zeros(1, np.int32)
    check(L.rl_lr_predict(int(device), keep.ctypes.data, fid.size, w.ctypes.data, len(w), rows.ctypes.data, rows.shape[0], rows.shape[1],
                          out.ctypes.data))
    return out


def perm_test(base, targets, seed, perm_begin=0, perm_count=10000, want_pdiff=False, device=0):
    """rl_perm_test (rl_perm.inc): the Analyzer's randomisation test on the GPU.  base [n], targets [n_targets][n] in the baseline
    HashMap's iteration order; returns (int64 counts [n_targets], f64 trueDiff [n_targets], f64 pDiff [n_targets][perm_count] or None)"""
    L = lib()
    if not hasattr(L, "rl_perm_test"):
        raise RankLibError("rlhip: this librlhip.so has no randomisation test (rl_perm_test)")
    b = np.ascontiguousarray(base, dtype=np.float64)
    t = np.ascontiguousarray(targets, dtype=np.float64)
    if b.ndim != 1 or t.ndim != 2 or t.shape[1] != b.shape[0]:
        raise RankLibError("rlhip: perm_test takes base [n] and targets [n_targets][n]")
    n, nt = int(b.shape[0]), int(t.shape[0])
    count, td = np.zeros(max(1, nt), np.int64), np.zeros(max(1, nt), np.float64)
    pd = np.zeros((nt, int(perm_count)), np.float64) if want_pdiff and nt >= 1 and n >= 1 and 1 <= perm_count <= 2 ** 31 - 1 else None
    check(L.rl_perm_test(int(device), b.ctypes.data, t.ctypes.data, n, nt, int(seed), int(perm_begin), int(perm_count),
                         count.ctypes.data, td.ctypes.data, None if pd is None else pd.ctypes.data))
    return count[:nt], td[:nt], pd


def perm_calib(chain_adds=1 << 22, base=None, target=None, seed=0, perm_count=1, device=0):
    """rl_debug_perm_calib: (ns per dependent f64 add on the device, ms of the Java's loop as written on one host thread, its count)"""
    ns, ms, cnt = C.c_double(0), C.c_double(0), C.c_int64(0)
    b = None if base is None else np.ascontiguousarray(base, dtype=np.float64)
    t = None if target is None else np.ascontiguousarray(target, dtype=np.float64)
    check(lib().rl_debug_perm_calib(int(device), None if b is None else b.ctypes.data, None if t is None else t.ctypes.data,
                                    0 if b is None else len(b), int(seed), int(perm_count), int(chain_adds), C.byref(ns), C.byref(ms),
                                    C.byref(cnt)))
    return ns.value, ms.value, cnt.value


def eval_lists(scores, labels, qoff, metric, k, err_max=16.0, qkey=None, ideal_dcg=None, rel_doc_count=None, want_pos=False, device=0):
    """rl_eval_lists (rl_eval.inc): every list ranked stable and descending by its scores and scored by the metric, on the GPU.  scores
    [n_docs] f64, labels [n_docs], qoff [n_lists + 1]; metric: a name of RL_EVAL_METRIC.  Returns (f64 metric per list, int32 0-based
    position of every document in its list's ranking or None, f64 ideal DCG per list -- NaN unless the metric is NDCG)"""
    L = lib()
    if not hasattr(L, "rl_eval_lists"):
        raise RankLibError("rlhip: this librlhip.so has no test-time evaluation (rl_eval_lists)")
    m = str(metric).upper()
    if m not in RL_EVAL_METRIC:
        raise RankLibError("rlhip: eval_lists metric must be one of NDCG, DCG, MAP, ERR, P, RR, BEST (got %s)" % metric)
    sc = np.ascontiguousarray(scores, dtype=np.float64)
    lab = np.ascontiguousarray(labels, dtype=np.float32)
    qo = np.ascontiguousarray(qoff, dtype=np.int32)
    if sc.ndim != 1 or lab.shape != sc.shape or qo.ndim != 1 or qo.size < 1:
        raise RankLibError("rlhip: eval_lists takes scores [n_docs], labels [n_docs] and qoff [n_lists + 1]")
    nl = int(qo.size) - 1

    def per_list(a, dtype, what):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dtype)
        if a.shape != (nl,):
            raise RankLibError("rlhip: eval_lists takes %s [n_lists]" % what)
        return a
    qk, idl, rdc = per_list(qkey, np.int32, "qkey"), per_list(ideal_dcg, np.float64, "ideal_dcg"), per_list(rel_doc_count, np.int32, "rel_doc_count")
    out, ideal = np.zeros(max(1, nl), np.float64), np.zeros(max(1, nl), np.float64)
    pos = np.zeros(max(1, sc.size), np.int32) if want_pos else None
    ptr = lambda a: None if a is None else a.ctypes.data      # noqa: E731
    check(L.rl_eval_lists(int(device), RL_EVAL_METRIC[m], int(k), float(err_max), sc.ctypes.data, lab.ctypes.data, int(sc.size), qo.ctypes.data,
                          nl, ptr(qk), ptr(idl), ptr(rdc), out.ctypes.data, ptr(pos), ideal.ctypes.data))
    return out[:nl], None if pos is None else pos[:sc.size], ideal[:nl]


def eval_kernel_ms():
    """rl_debug_eval_times: ms of the kernels of this thread's last eval_lists call, between device events"""
    ms = C.c_double(0)
    check(lib().rl_debug_eval_times(C.byref(ms)))
    return ms.value


def stage_times():
    """rl_debug_stage_times: (walk ms, rank ms) of this thread's last predict_stages / eval_stages call, between device events"""
    w, r = C.c_double(0), C.c_double(0)
    check(lib().rl_debug_stage_times(C.byref(w), C.byref(r)))
    return w.value, r.value


def contrib_times():
    """rl_debug_contrib_times: (cover ms, walk ms) of this thread's last cover / predict_contribs calls, between device events"""
    c, w = C.c_double(0), C.c_double(0)
    check(lib().rl_debug_contrib_times(C.byref(c), C.byref(w)))
    return c.value, w.value


def contrib_passes():
    """rl_debug_contrib_passes: the column passes of this thread's last predict_contribs call"""
    p = C.c_int32(0)
    check(lib().rl_debug_contrib_passes(C.byref(p)))
    return p.value


def shap_times():
    """rl_debug_shap_times: walk ms of this thread's last predict_shap call, between device events"""
    w = C.c_double(0)
    check(lib().rl_debug_shap_times(C.byref(w)))
    return w.value


def shap_passes():
    """rl_debug_shap_passes: the column passes of this thread's last predict_shap call"""
    p = C.c_int32(0)
    check(lib().rl_debug_shap_passes(C.byref(p)))
    return p.value


def interact_times():
    """rl_debug_interact_times: (walk ms, shap ms) of this thread's last predict_interactions call, between device events"""
    w, s = C.c_double(0), C.c_double(0)
    check(lib().rl_debug_interact_times(C.byref(w), C.byref(s)))
    return w.value, s.value


def interact_passes():
    """rl_debug_interact_passes: the column passes k_model_interact took in this thread's last predict_interactions call"""
    p = C.c_int32(0)
    check(lib().rl_debug_interact_passes(C.byref(p)))
    return p.value


def partial_times():
    """rl_debug_partial_times: (walk ms, reduce ms) of this thread's last predict_partial call, between device events"""
    w, r = C.c_double(0.0), C.c_double(0.0)
    check(lib().rl_debug_partial_times(C.byref(w), C.byref(r)))
    return w.value, r.value


def permuted_times():
    """rl_debug_permuted_times: (walk ms, rank ms) of this thread's last predict_permuted / eval_permuted call, between device events"""
    w, r = C.c_double(0), C.c_double(0)
    check(lib().rl_debug_permuted_times(C.byref(w), C.byref(r)))
    return w.value, r.value


NORM_CHUNK_BYTES = 1 << 30           # rows of X one rl_normalize_lists call uploads (whole lists; a longer list is a call of its own)


def normalize_lists(X, qoff, cols, kind, row_len=None, times=1, chunk_bytes=NORM_CHUNK_BYTES, device=0):
    """rl_normalize_lists (rl_norm.inc): every list of X normalised IN PLACE on the GPU, column by column as the Java's normalisers do.
    X [n_docs, stride]: a C-contiguous, writable float32 matrix whose rows are DataPoint.fVals (column 0 unused); qoff [n_lists + 1]; cols:
    the feature ids, without duplicates; kind: sum, zscore or linear; row_len: None, or [n_docs] = len(fVals) of every row; times: that
    many applications in a row.  The rows go in chunks of whole lists of at most chunk_bytes (a longer list is a chunk of its own); the
    lists are independent, so the cut changes no bit.  Returns the number of native calls."""
    L = lib()
    if not hasattr(L, "rl_normalize_lists"):
        raise RankLibError("rlhip: this librlhip.so has no normaliser (rl_normalize_lists)")
    k = str(kind).lower()
    if k not in RL_NORM_KIND:
        raise RankLibError("rlhip: normalize_lists kind must be one of sum, zscore, linear (got %s)" % kind)
    if not (isinstance(X, np.ndarray) and X.dtype == np.float32 and X.ndim == 2 and X.flags.c_contiguous and X.flags.writeable):
        raise RankLibError("rlhip: normalize_lists takes a writable C-contiguous float32 matrix [n_docs, stride] (it is normalised in place)")
    qo = np.ascontiguousarray(qoff, dtype=np.int32)
    co = np.ascontiguousarray(cols, dtype=np.int32)
    rl = None if row_len is None else np.ascontiguousarray(row_len, dtype=np.int32)
    n, stride = X.shape
    if qo.ndim != 1 or qo.size < 2 or co.ndim != 1 or (rl is not None and rl.shape != (n,)):
        raise RankLibError("rlhip: normalize_lists takes qoff [n_lists + 1], cols [n_cols] and row_len [n_docs]")
    nl = int(qo.size) - 1
    row_bytes = stride * 4
    # chunk ends: the last list whose end stays within the budget from the chunk's first row, at least one list
    calls, a = 0, 0
    whole = n * row_bytes <= chunk_bytes or not (qo[0] == 0 and qo[-1] == n and np.all(np.diff(qo) > 0))   # bad offsets: the C call's message
    while a < nl:
        if whole:
            b = nl
        else:
            b = int(np.searchsorted(qo, int(qo[a]) + max(1, chunk_bytes // row_bytes), side="right")) - 1
            b = min(nl, max(b, a + 1))
        r0, r1 = (0, n) if whole else (int(qo[a]), int(qo[b]))
        q = qo if whole else np.ascontiguousarray(qo[a:b + 1] - qo[a])
        rlc = None if rl is None else rl[r0:r1]
        check(L.rl_normalize_lists(int(device), RL_NORM_KIND[k], X.ctypes.data + r0 * row_bytes, r1 - r0, stride,
                                   None if rlc is None else rlc.ctypes.data, q.ctypes.data, b - a, co.ctypes.data, int(co.size), int(times)))
        calls += 1
        a = b
    return calls


def normalize_kernel_ms():
    """rl_debug_normalize_times: ms of the kernel of this thread's last rl_normalize_lists call, between device events"""
    ms = C.c_double(0)
    check(lib().rl_debug_normalize_times(C.byref(ms)))
    return ms.value
