"""ctypes binding of libsbr_rnn.so + `RNNEngine`, the object that stands where the
reference keeps its three Theano callables and the Lasagne parameter list
(neural_networks/rnn_base.py:185 train_function, :196-211 test_function, :188-194
predict_function, :476/:515 get/set_all_param_values).

There is NO CPU path here: if the HIP library is missing or no GPU is visible the
constructor raises.  PyTorch is used for plumbing only (device arena allocation, current
stream, torch.distributed all-reduce of the gradient section in data-parallel runs).
"""
import ctypes
import os

import numpy as np

# HIP multiplexes streams onto this many hardware queues (default 4); the engine's side stream, torch's streams and
# RCCL's must not pile onto one queue.  Read when the HIP runtime initialises, i.e. it only helps when this module is
# imported before the first device call.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsbr_rnn.so")

SBR_MAX_LAYERS = 4
SBR_ABI_VERSION = 11
SBR_N_PHASES = 8
PHASE_NAMES = ("gather", "rec_fwd", "output", "rec_bwd", "wgrad", "scatter", "update", "total")

CELLS = {"LSTM": 0, "GRU": 1, "Vanilla": 2}                     # --r_t, recurrent_layers.py:9
LOSSES = {"CCE": 0, "Blackout": 1, "BPR": 2, "TOP1": 3,          # --loss, command_parser.py:43
          "hinge": 4, "logit": 5, "logsig": 6,                   # ... RNNMargin's multi-target losses (command_parser.py:118-119)
          "SCCE": 7, "BPRelu": 8, "lin": 9}                      # ... RNNCluster's further sampled losses (its "CCE" is SCCE here)
MARGIN_LOSSES = ("hinge", "logit", "logsig")
SAMPLED_LOSSES = ("Blackout", "BPR", "TOP1", "SCCE", "BPRelu", "lin")      # the last three: RNNCluster's (rnn_cluster.py:158-175)
UPDATERS = {"adagrad": 0, "adadelta": 1, "rmsprop": 2, "nesterov": 3, "adam": 4}   # --u_m
FLAG_SIMPLE_REC = 1
FLAG_SIMPLE_GEMM = 2
FLAG_ATOMIC_SCATTER = 4
FLAG_PROFILE_REC = 8
FLAG_F32_MFMA = 16
FLAG_SPARSE_UPDATE = 32      # row-sparse optimizer steps for every block that exists (default: where a step cannot touch every row)
FLAG_DENSE_UPDATE = 64       # never: lasagne's dense pass over every parameter
FLAG_BF16_PROJECTION = 128   # output projection on plain bf16 operands (one MFMA per block) -- training forward of CCE, predict, top-k
FLAG_BF16_LAYERS = 256       # the dense GEMMs between stacked layers (input projection of layer >= 2 and its backward pair) on plain bf16 operands
# sbr_evaluate's exclusion modes (include/sbr_rnn.h)
EVAL_EXCL_NONE, EVAL_EXCL_VIEWED, EVAL_EXCL_WINDOW, EVAL_EXCL_WINDOW_ZERO = 0, 1, 2, 3
EVAL_EXCL_PREFIX = 4         # sbr_evaluate_positions only: at position p the distinct items in front of p are never ranked
# sbr_cluster_evaluate's roads (include/sbr_rnn.h)
CEVAL_LISTS, CEVAL_PRODUCT = 0, 1
# sbr_sessions_rank's exclusion modes (include/sbr_rnn.h): nothing, the item fed last, the kept history of the slot
SESSION_EXCL_NONE, SESSION_EXCL_LAST, SESSION_EXCL_HISTORY = 0, 1, 2


class SbrEvalOut(ctypes.Structure):
    """sbr_eval_out: the host arrays of one ranking's results (sbr_cluster_evaluate)"""
    _fields_ = [("ids", ctypes.c_void_p), ("n_pred", ctypes.c_void_p), ("hits", ctypes.c_void_p), ("first_hit", ctypes.c_void_p),
                ("hitmask", ctypes.c_void_p), ("item_hits", ctypes.c_void_p)]

    @classmethod
    def of(cls, rec):
        """over the arrays of an _eval_record dict (which must outlive the call)"""
        return cls(*[_ptr(rec[name]) for name, _ in cls._fields_])


class SbrConfig(ctypes.Structure):
    _fields_ = [("abi_version", ctypes.c_int32), ("cell", ctypes.c_int32), ("n_layers", ctypes.c_int32),
                ("layers", ctypes.c_int32 * SBR_MAX_LAYERS), ("n_items", ctypes.c_int32),
                ("input_size", ctypes.c_int32), ("n_feat", ctypes.c_int32), ("max_length", ctypes.c_int32),
                ("batch_size", ctypes.c_int32), ("local_batch", ctypes.c_int32), ("row_offset", ctypes.c_int32),
                ("loss", ctypes.c_int32), ("n_samples", ctypes.c_int32), ("updater", ctypes.c_int32),
                ("learning_rate", ctypes.c_float), ("rho", ctypes.c_float), ("beta1", ctypes.c_float),
                ("beta2", ctypes.c_float), ("regularization", ctypes.c_float), ("grad_clip", ctypes.c_float),
                ("flags", ctypes.c_int32), ("embedding_size", ctypes.c_int32), ("bidirectional", ctypes.c_int32),
                ("balance", ctypes.c_float), ("n_targets", ctypes.c_int32), ("unique", ctypes.c_int32)]


# every symbol include/sbr_rnn.h declares (tests check the library exports all of them)
EXPORTS = ["sbr_last_error", "sbr_abi_version", "sbr_arena_bytes", "sbr_create", "sbr_destroy", "sbr_num_params",
           "sbr_param_shape", "sbr_describe_param", "sbr_set_params", "sbr_get_params", "sbr_get_grads", "sbr_section", "sbr_set_batch",
           "sbr_set_default_target",
           "sbr_train_step", "sbr_train_step_lagged", "sbr_cost_lagged", "sbr_lagged_flush", "sbr_zero_grads", "sbr_forward", "sbr_loss_backward_output", "sbr_backward_recurrent",
           "sbr_apply_update", "sbr_read_cost", "sbr_predict_scores", "sbr_topk", "sbr_rank", "sbr_rank_candidates", "sbr_debug_buffer",
           "sbr_copy_to_host", "sbr_synchronize", "sbr_enable_timing", "sbr_phase_times", "sbr_chain_times", "sbr_query",
           "sbr_set_deferred_join", "sbr_join_side", "sbr_debug_gemm", "sbr_debug_scatter", "sbr_debug_occupy", "sbr_flush_lazy", "sbr_sparse_info", "sbr_sparse_pack",
           "sbr_sparse_unpack_add", "sbr_dense_ranges", "sbr_sparse_pack_device", "sbr_sparse_unpack_add_all",
           "sbr_cluster_create", "sbr_cluster_destroy", "sbr_cluster_set_params", "sbr_cluster_get_params", "sbr_cluster_get_grads",
           "sbr_cluster_set_scale", "sbr_cluster_forward_backward", "sbr_cluster_apply_update", "sbr_cluster_select",
           "sbr_cluster_mask_scores", "sbr_cluster_hard", "sbr_cluster_lists", "sbr_cluster_rank",
           "sbr_cluster_train_step_lagged", "sbr_cluster_last_ids",
           "sbr_dataset_create", "sbr_dataset_destroy", "sbr_dataset_set_tables", "sbr_dataset_set_options", "sbr_dataset_noise_pass", "sbr_dataset_current_sequences", "sbr_dataset_set_target_bias",
           "sbr_plan_rows_host", "sbr_dataset_plan_pass",
           "sbr_dataset_plan_segments", "sbr_plan_pass_host", "sbr_build_batch", "sbr_evaluate", "sbr_cluster_evaluate", "sbr_evaluate_ranks",
           "sbr_evaluate_positions", "sbr_evaluate_candidates", "sbr_eval_negatives_host",
           "sbr_evaluate_logprob", "sbr_evaluate_positions_logprob", "sbr_debug_row_logprob",
           "sbr_state_bytes", "sbr_state_save", "sbr_state_load", "sbr_cluster_state_bytes", "sbr_cluster_state_save",
           "sbr_cluster_state_load", "sbr_dataset_state_bytes", "sbr_dataset_state_save", "sbr_dataset_state_load",
           "sbr_sessions_create", "sbr_sessions_destroy", "sbr_sessions_reset", "sbr_sessions_advance", "sbr_sessions_replay", "sbr_sessions_replay_ranks", "sbr_sessions_adopt",
           "sbr_sessions_rank", "sbr_sessions_rank_candidates", "sbr_sessions_read", "sbr_sessions_write",
           "sbr_sessions_record_layout", "sbr_sessions_export", "sbr_sessions_import"]

_lib = None


def load_library(path=None):
    """dlopen libsbr_rnn.so (import torch first so one HIP runtime serves both)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or os.environ.get("SBR_LIB") or LIB_PATH      # SBR_LIB: another build of the library (kernel experiments)
    try:        # torch bundles its own libamdhip64: it must be the one already loaded when the extension binds to HIP,
        import torch  # noqa: F401  otherwise two runtimes coexist and this library sees no device
    except ImportError:
        pass
    if not os.path.exists(path):
        raise RuntimeError("HIP extension %s is missing: build it with __graft_entry__.build() "
                           "(there is no CPU fallback)" % path)
    lib = ctypes.CDLL(path)
    lib.sbr_last_error.restype = ctypes.c_char_p
    vp, i32p, f32p = ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
    lib.sbr_arena_bytes.argtypes = [ctypes.POINTER(SbrConfig), ctypes.POINTER(ctypes.c_size_t)]
    lib.sbr_create.argtypes = [ctypes.POINTER(SbrConfig), vp, ctypes.c_size_t, vp, ctypes.POINTER(vp)]
    lib.sbr_destroy.argtypes = [vp]
    lib.sbr_destroy.restype = None
    lib.sbr_num_params.argtypes = [vp]
    lib.sbr_param_shape.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int)]
    lib.sbr_describe_param.argtypes = [ctypes.POINTER(SbrConfig), ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t,
                                       ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int)]
    for fn in (lib.sbr_set_params, lib.sbr_get_params, lib.sbr_get_grads):
        fn.argtypes = [vp, ctypes.c_int, ctypes.POINTER(vp)]
    lib.sbr_section.argtypes = [vp, ctypes.c_int, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t),
                                ctypes.POINTER(ctypes.c_size_t)]
    lib.sbr_set_batch.argtypes = [vp, vp, vp, vp, vp, vp, ctypes.c_int, ctypes.c_int]
    lib.sbr_set_default_target.argtypes = [vp, vp]
    lib.sbr_train_step.argtypes = [vp, f32p]
    lib.sbr_train_step_lagged.argtypes = [vp, f32p, i32p]
    lib.sbr_cost_lagged.argtypes = [vp, f32p, i32p]
    lib.sbr_lagged_flush.argtypes = [vp, f32p, i32p]
    for fn in (lib.sbr_zero_grads, lib.sbr_forward, lib.sbr_loss_backward_output, lib.sbr_backward_recurrent,
               lib.sbr_apply_update, lib.sbr_synchronize):
        fn.argtypes = [vp]
    lib.sbr_read_cost.argtypes = [vp, f32p]
    lib.sbr_predict_scores.argtypes = [vp, ctypes.c_int, vp]
    lib.sbr_topk.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp]
    lib.sbr_rank.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp]
    lib.sbr_rank_candidates.argtypes = [vp, ctypes.c_int, vp, vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp]
    lib.sbr_debug_buffer.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t)]
    lib.sbr_copy_to_host.argtypes = [vp, vp, vp, ctypes.c_size_t]
    lib.sbr_enable_timing.argtypes = [vp, ctypes.c_int]
    lib.sbr_phase_times.argtypes = [vp, f32p]
    lib.sbr_chain_times.argtypes = [vp, ctypes.c_int, f32p, ctypes.POINTER(ctypes.c_int)]
    i64p = ctypes.POINTER(ctypes.c_int64)
    lib.sbr_query.argtypes = [vp, ctypes.c_char_p, i64p]
    lib.sbr_debug_scatter.argtypes = [vp, ctypes.c_int, f32p, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
    lib.sbr_debug_occupy.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.sbr_debug_gemm.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_int64, vp, ctypes.c_int64, ctypes.c_int64, vp, ctypes.c_int64,
                                   ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, vp, vp, ctypes.c_size_t, ctypes.c_int32]
    lib.sbr_flush_lazy.argtypes = [vp]
    lib.sbr_sparse_info.argtypes = [vp, ctypes.c_int, i64p, i64p, i64p]
    lib.sbr_sparse_pack.argtypes = [vp, ctypes.c_int, vp, vp, i32p]
    lib.sbr_sparse_unpack_add.argtypes = [vp, ctypes.c_int, vp, vp, ctypes.c_int]
    lib.sbr_dense_ranges.argtypes = [vp, ctypes.c_int, i64p, i64p, ctypes.POINTER(ctypes.c_int)]
    lib.sbr_set_deferred_join.argtypes = [vp, ctypes.c_int]
    lib.sbr_join_side.argtypes = [vp]
    lib.sbr_cluster_create.restype = vp
    lib.sbr_cluster_create.argtypes = [vp, vp]
    lib.sbr_cluster_destroy.restype = None
    lib.sbr_cluster_destroy.argtypes = [vp]
    for fn in (lib.sbr_cluster_set_params, lib.sbr_cluster_get_params, lib.sbr_cluster_get_grads):
        fn.argtypes = [vp, vp, vp]
    lib.sbr_cluster_set_scale.argtypes = [vp, ctypes.c_float]
    lib.sbr_cluster_forward_backward.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_int, f32p]
    lib.sbr_cluster_apply_update.argtypes = [vp]
    lib.sbr_cluster_select.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp]
    lib.sbr_cluster_mask_scores.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, vp, vp]
    lib.sbr_cluster_hard.argtypes = [vp, vp]
    lib.sbr_cluster_lists.argtypes = [vp, vp, vp]
    lib.sbr_cluster_rank.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, vp, vp]
    lib.sbr_cluster_train_step_lagged.argtypes = [vp, vp, vp, ctypes.c_int, ctypes.c_uint64, f32p, i32p]
    lib.sbr_cluster_last_ids.argtypes = [vp, vp, ctypes.c_int]
    lib.sbr_dataset_create.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_int32, vp, ctypes.POINTER(vp)]
    lib.sbr_dataset_destroy.argtypes = [vp]
    lib.sbr_dataset_set_tables.argtypes = [vp, vp, vp]
    lib.sbr_dataset_set_options.argtypes = [vp, vp, ctypes.c_int]
    lib.sbr_dataset_noise_pass.argtypes = [vp, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_uint64]
    lib.sbr_dataset_current_sequences.argtypes = [vp, vp, vp, vp]
    lib.sbr_dataset_set_target_bias.argtypes = [vp, vp, ctypes.c_int32, ctypes.c_uint64]
    lib.sbr_plan_rows_host.argtypes = [vp, vp, vp, vp, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, vp, ctypes.c_uint64,
                                       vp, vp, vp, i32p, ctypes.c_int64, vp, vp, vp, i64p, i64p]
    lib.sbr_dataset_plan_pass.argtypes = [vp, vp, ctypes.c_int32, i64p]
    lib.sbr_dataset_plan_segments.argtypes = [vp, i64p, ctypes.POINTER(i32p), ctypes.POINTER(i32p), ctypes.POINTER(i32p),
                                              ctypes.POINTER(i32p)]
    lib.sbr_plan_pass_host.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_int32, vp, vp, i32p, vp, vp, vp, vp, i64p, i64p]
    lib.sbr_build_batch.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_uint64]
    lib.sbr_evaluate.argtypes = [vp, vp, vp, ctypes.c_int64, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, vp, vp]
    lib.sbr_evaluate_ranks.argtypes = [vp, vp, vp, ctypes.c_int64, ctypes.c_int, vp, vp, ctypes.c_int64, vp]
    lib.sbr_evaluate_positions.argtypes = [vp, vp, vp, ctypes.c_int64, ctypes.c_int, ctypes.c_int, vp, vp, vp, ctypes.c_int64]
    lib.sbr_evaluate_logprob.argtypes = [vp, vp, vp, ctypes.c_int64, ctypes.c_int, vp, vp, ctypes.c_int64, vp, vp, vp]
    lib.sbr_evaluate_positions_logprob.argtypes = [vp, vp, vp, ctypes.c_int64, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, vp, ctypes.c_int64]
    lib.sbr_debug_row_logprob.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, vp, ctypes.c_int32, vp, vp]
    lib.sbr_evaluate_candidates.argtypes = [vp, vp, vp, ctypes.c_int64, ctypes.c_int, vp, vp, ctypes.c_int32, ctypes.c_uint64, vp, vp, vp,
                                            ctypes.c_int64, vp, vp]
    lib.sbr_eval_negatives_host.argtypes = [vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64, vp, vp, vp]
    lib.sbr_cluster_evaluate.argtypes = [vp, vp, vp, vp, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(SbrEvalOut),
                                         ctypes.POINTER(SbrEvalOut), vp, vp, vp]
    szp = ctypes.POINTER(ctypes.c_size_t)
    for stem in ("sbr_state", "sbr_cluster_state", "sbr_dataset_state"):
        getattr(lib, stem + "_bytes").argtypes = [vp, szp]
        getattr(lib, stem + "_save").argtypes = [vp, vp, ctypes.c_size_t, szp]
        getattr(lib, stem + "_load").argtypes = [vp, vp, ctypes.c_size_t]
    lib.sbr_sessions_create.argtypes = [vp, ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(vp)]
    lib.sbr_sessions_destroy.restype = None
    lib.sbr_sessions_destroy.argtypes = [vp]
    lib.sbr_sessions_reset.argtypes = [vp, vp, ctypes.c_int64]
    lib.sbr_sessions_advance.argtypes = [vp, vp, vp, vp, ctypes.c_int64]
    lib.sbr_sessions_replay.argtypes = [vp, vp, ctypes.c_int64, vp, vp, vp]
    lib.sbr_sessions_replay_ranks.argtypes = [vp, vp, ctypes.c_int64, vp, vp, vp, ctypes.c_int, ctypes.c_int64, vp, vp, vp]
    lib.sbr_sessions_adopt.argtypes = [vp, vp, ctypes.c_int32]
    lib.sbr_sessions_rank.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp]
    lib.sbr_sessions_rank_candidates.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_int, vp, vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp]
    lib.sbr_sessions_read.argtypes = [vp, ctypes.c_int32, ctypes.c_int32, vp, vp, i64p, vp]
    lib.sbr_sessions_write.argtypes = [vp, ctypes.c_int32, ctypes.c_int32, vp, vp]
    lib.sbr_sessions_record_layout.argtypes = [ctypes.POINTER(SbrConfig), ctypes.c_int32, szp, ctypes.POINTER(ctypes.c_uint64)]
    lib.sbr_sessions_export.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_int64, vp, ctypes.c_size_t]
    lib.sbr_sessions_import.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_int64, vp, ctypes.c_size_t]
    if path == LIB_PATH:
        _lib = lib
    return lib


class SbrError(RuntimeError):
    pass


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def position_counts(lengths, max_length, min_history=1):
    """n_pos of sbr_evaluate_positions (UserPrefix, csrc/sbr_common.h) for sequences of these lengths: the first
    F = min(L - 1, max_length) items are fed and the positions min_history .. F evaluated -- max(0, F - min_history + 1) of them"""
    lengths = np.asarray(lengths, dtype=np.int64)
    fed = np.minimum(np.maximum(lengths - 1, 0), int(max_length))
    return np.maximum(0, fed - int(min_history) + 1)


EVAL_MAX_NEGATIVES = 4096    # SBR_EVAL_MAX_NEGATIVES (include/sbr_rnn.h)


def _neg_cdf_arg(neg_cdf, n_items):
    """evaluate_candidates' / sampled_negatives' neg_cdf in the C-ABI's type: float64 (n_items,), or None"""
    if neg_cdf is None:
        return None
    neg_cdf = np.ascontiguousarray(np.asarray(neg_cdf, dtype=np.float64).reshape(-1))
    if neg_cdf.shape != (n_items,):
        raise ValueError("neg_cdf must have n_items=%d entries, got %r" % (n_items, neg_cdf.shape))
    return neg_cdf


def sampled_negatives(seq, user, n_items, n_negatives, seed, neg_cdf=None):
    """The negatives RNNEngine.evaluate_candidates(n_negatives=, seed=, neg_cdf=) draws for dataset user `user` whose whole uploaded
    sequence is `seq` (sbr_eval_negatives_host: pure host code, no device) -- the documented way to reproduce a published candidate
    set.  Returns the accepted ids in draw order, int32; fewer than n_negatives when the attempt cap of 16 * n_negatives + 256 ends
    the draw first."""
    lib = load_library()
    seq = np.ascontiguousarray(np.asarray(seq, dtype=np.int32).reshape(-1))
    n_negatives = int(n_negatives)
    if not 1 <= n_negatives <= min(int(n_items) - 1, EVAL_MAX_NEGATIVES):     # (the library checks it too: here before `out` is sized by it)
        raise ValueError("n_negatives=%d outside [1,min(N - 1,%d)]" % (n_negatives, EVAL_MAX_NEGATIVES))
    neg_cdf = _neg_cdf_arg(neg_cdf, int(n_items))
    out, n_out = np.empty(n_negatives, dtype=np.int32), ctypes.c_int32()
    rc = lib.sbr_eval_negatives_host(_ptr(seq) if len(seq) else None, len(seq), int(user), int(n_items), n_negatives,
                                     int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(neg_cdf), _ptr(out), ctypes.byref(n_out))
    if rc != 0:
        raise SbrError(lib.sbr_last_error().decode())
    return out[:n_out.value].copy()


def _check_k(k, n_items):
    k = int(k)
    if not 1 <= k <= n_items:       # (the library checks it too: here before the result arrays are sized by k)
        raise ValueError("k=%d outside [1,N=%d]" % (k, n_items))
    return k


def _excl_csr(exclude, n):
    """rank()'s per-row `exclude` lists as the CSR sbr_rank takes: (int32 ids, int64 offsets), or (None, None)"""
    if exclude is None:
        return None, None
    lists = [np.zeros(0, dtype=np.int32) if e is None else np.asarray(e, dtype=np.int32).reshape(-1) for e in exclude]
    if len(lists) != n:
        raise ValueError("exclude must hold one id list per row: %d lists for %d rows" % (len(lists), n))
    off_arr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(e) for e in lists], out=off_arr[1:])
    ids_arr = np.ascontiguousarray(np.concatenate(lists + [np.zeros(1, dtype=np.int32)]))   # (never empty: its pointer is not NULL)
    return ids_arr, off_arr


def _csr_args(excl_ids, excl_off, rows):
    """rank_csr()'s lists in the C-ABI's types"""
    if excl_ids is not None:
        excl_ids = np.ascontiguousarray(np.asarray(excl_ids, dtype=np.int32))
    if excl_off is not None:
        excl_off = np.ascontiguousarray(np.asarray(excl_off, dtype=np.int64))
        if excl_off.shape != (rows + 1,):
            raise ValueError("excl_off must have %d entries (rows + 1), got %r" % (rows + 1, excl_off.shape))
    return excl_ids, excl_off


def _cand_csr(candidates, n):
    """rank_candidates()'s `candidates` as the CSR sbr_rank_candidates takes: (int32 ids, int64 offsets, shared).  A single 1-D array
    of ids is ONE list shared by all n rows; anything else holds one id list per row (None or empty: no candidates).  Every list
    comes out strictly ascending: sorted and de-duplicated (np.unique)."""
    shared = isinstance(candidates, np.ndarray) and candidates.ndim == 1 and candidates.dtype != object
    if not shared and len(candidates) > 0 and all(np.ndim(c) == 0 and c is not None for c in candidates):
        shared = True                                                 # a plain list of ids
    if shared:
        lists = [candidates]
    else:
        lists = list(candidates)
        if len(lists) != n:
            raise ValueError("candidates must hold one id list per row: %d lists for %d rows" % (len(lists), n))
    lists = [np.zeros(0, dtype=np.int32) if c is None else np.unique(np.asarray(c, dtype=np.int32).reshape(-1)) for c in lists]
    off_arr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(c) for c in lists], out=off_arr[1:])
    ids_arr = np.ascontiguousarray(np.concatenate(lists + [np.zeros(1, dtype=np.int32)]))   # (never empty: its pointer is not NULL)
    return ids_arr, off_arr, shared


def _cand_args(cand_ids, cand_off, shared, rows):
    """rank_candidates_csr()'s lists in the C-ABI's types"""
    if cand_ids is not None:
        cand_ids = np.ascontiguousarray(np.asarray(cand_ids, dtype=np.int32))
    if cand_off is not None:
        cand_off = np.ascontiguousarray(np.asarray(cand_off, dtype=np.int64))
        want = 2 if shared else rows + 1
        if cand_off.shape != (want,):
            raise ValueError("cand_off must have %d entries (%s), got %r" % (want, "a shared list" if shared else "rows + 1", cand_off.shape))
    return cand_ids, cand_off


def _eval_record(n, k, n_items, want_mask, want_ids):
    """the host arrays of one ranking's per-user results (RNNEngine.evaluate's return value)"""
    return {"n_pred": np.empty(n, np.int32), "hits": np.empty(n, np.int32), "first_hit": np.empty(n, np.int32),
            "item_hits": np.empty(n_items, np.int32),
            "hitmask": np.empty((n, (k + 31) // 32), np.uint32) if want_mask else None,
            "ids": np.empty((n, k), np.int32) if want_ids else None}


def _state_get(check, lib, stem, obj):
    """the blob of `obj` (bytes): <stem>_bytes for the size, <stem>_save into a buffer of that size (include/sbr_rnn.h "Training state")"""
    n, w = ctypes.c_size_t(), ctypes.c_size_t()
    check(getattr(lib, stem + "_bytes")(obj, ctypes.byref(n)))
    buf = np.empty(n.value, dtype=np.uint8)
    check(getattr(lib, stem + "_save")(obj, buf.ctypes.data, n.value, ctypes.byref(w)))
    return buf[:w.value].tobytes()


def _state_set(check, lib, stem, obj, blob):
    buf = np.frombuffer(bytes(blob), dtype=np.uint8)
    check(getattr(lib, stem + "_load")(obj, buf.ctypes.data if len(buf) else None, len(buf)))


def mask_to_lengths(mask):
    """The reference's masks are prefix masks (rnn_one_hot.py:100-101: mask[i, :len] = 1);
    the engine takes lengths.  Anything else is rejected loudly."""
    mask = np.asarray(mask)
    lengths = (mask != 0).sum(axis=1).astype(np.int32)
    if not np.array_equal(mask != 0, np.arange(mask.shape[1])[None, :] < lengths[:, None]):
        raise ValueError("mask must be a left-aligned prefix mask (rows of ones followed by zeros)")
    return lengths


def plan_pass_host(lengths, order, batch_size, pending=None, lib=None):
    """The batch plan of one pass over the users (sbr_plan_pass_host; no GPU needed): which user contributes how many
    rows to which batch, exactly as the reference fills its batches (rnn_base.py:394-415).
    Returns (segments, n_batches, pending): segments = int array (n, 4) of (user, k, first_row, batch) for the complete
    batches; pending = [(user, k), ...] of the trailing partial batch, to be passed to the next pass."""
    lib = lib or load_library()
    lengths = np.ascontiguousarray(lengths, dtype=np.int64)
    n = len(lengths)
    order_a = None if order is None else np.ascontiguousarray(order, dtype=np.int32)
    pending = list(pending or [])
    pu, pk = np.zeros(batch_size, np.int32), np.zeros(batch_size, np.int32)
    for i, (u, k) in enumerate(pending):
        pu[i], pk[i] = u, k
    npend = ctypes.c_int32(len(pending))
    cap = n + len(pending) + 1
    su, sk, sr, sb = (np.zeros(cap, np.int32) for _ in range(4))
    ns, nb = ctypes.c_int64(), ctypes.c_int64()
    rc = lib.sbr_plan_pass_host(lengths.ctypes.data, None if order_a is None else order_a.ctypes.data, n, batch_size,
                                pu.ctypes.data, pk.ctypes.data, ctypes.byref(npend), su.ctypes.data, sk.ctypes.data,
                                sr.ctypes.data, sb.ctypes.data, ctypes.byref(ns), ctypes.byref(nb))
    if rc != 0:
        raise ValueError(lib.sbr_last_error().decode("utf-8", "replace"))
    seg = np.stack([su[:ns.value], sk[:ns.value], sr[:ns.value], sb[:ns.value]], axis=1)
    return seg, nb.value, [(int(pu[i]), int(pk[i])) for i in range(npend.value)]


def plan_rows_host(items, offsets, order, batch_size, n_targets=1, shuffle=False, keep_prob=None, seed=0, pending=None, lengths=None,
                   lib=None):
    """The rows of one pass planned on the host (sbr_plan_rows_host; no GPU needed): the reference's _gen_mini_batch with a
    target selection that can come back empty (--target_bias).  Returns (rows, n_batches, pending): rows = int array
    (n, 2 + n_targets) of (user, split, target positions...), batch-major; pending = the carried rows in the same format."""
    lib = lib or load_library()
    items = np.ascontiguousarray(items, dtype=np.int32)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n = len(offsets) - 1
    lens = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.int64)
    order_a = None if order is None else np.ascontiguousarray(order, dtype=np.int32)
    kp = None if keep_prob is None else np.ascontiguousarray(keep_prob, dtype=np.float32)
    pend = np.zeros((0, 2 + n_targets), np.int32) if pending is None else np.asarray(pending, dtype=np.int32).reshape(-1, 2 + n_targets)
    pu, ps, pt = np.zeros(batch_size, np.int32), np.zeros(batch_size, np.int32), np.zeros(batch_size * n_targets, np.int32)
    pu[:len(pend)], ps[:len(pend)] = pend[:, 0], pend[:, 1]
    pt[:len(pend) * n_targets] = pend[:, 2:].reshape(-1)
    npend = ctypes.c_int32(len(pend))
    L = (offsets[1:] - offsets[:-1]) if lens is None else lens
    cap = int(batch_size + np.minimum(batch_size, np.maximum(0, L - 2)).sum())
    ru, rs, rt = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap * n_targets, np.int32)
    nr, nb = ctypes.c_int64(), ctypes.c_int64()
    rc = lib.sbr_plan_rows_host(items.ctypes.data, offsets.ctypes.data, None if lens is None else lens.ctypes.data,
                                None if order_a is None else order_a.ctypes.data, n, int(batch_size), int(n_targets), 1 if shuffle else 0,
                                None if kp is None else kp.ctypes.data, int(seed) & 0xFFFFFFFFFFFFFFFF, pu.ctypes.data, ps.ctypes.data,
                                pt.ctypes.data, ctypes.byref(npend), cap, ru.ctypes.data, rs.ctypes.data, rt.ctypes.data,
                                ctypes.byref(nr), ctypes.byref(nb))
    if rc != 0:
        raise ValueError(lib.sbr_last_error().decode("utf-8", "replace"))
    rows = np.concatenate([ru[:nr.value, None], rs[:nr.value, None], rt[:nr.value * n_targets].reshape(-1, n_targets)], axis=1)
    k = npend.value
    pending = np.concatenate([pu[:k, None], ps[:k, None], pt[:k * n_targets].reshape(-1, n_targets)], axis=1)
    return rows, nb.value, pending


class DeviceDataset(object):
    """The training sequences in HBM (CSR) + the per-pass batch plan (sbr_dataset_* in include/sbr_rnn.h)."""

    def __init__(self, engine, items, offsets, n_items):
        self.engine, self.lib = engine, engine.lib
        items = np.ascontiguousarray(items, dtype=np.int32)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        self.n_users, self.n_batches = len(offsets) - 1, 0
        self.offsets = offsets      # host copy (n_users + 1 words): sizes evaluate_ranks' result
        d = ctypes.c_void_p()
        with engine.torch.cuda.device(engine.device):
            engine._check(self.lib.sbr_dataset_create(items.ctypes.data, offsets.ctypes.data, self.n_users, int(n_items),
                                                      ctypes.c_void_p(engine.stream.cuda_stream), ctypes.byref(d)))
        self.d = d

    def set_tables(self, pop_db=None, sample_cdf=None):
        a = None if pop_db is None else np.ascontiguousarray(pop_db, dtype=np.float32)
        c = None if sample_cdf is None else np.ascontiguousarray(sample_cdf, dtype=np.float64)
        self.engine._check(self.lib.sbr_dataset_set_tables(self.d, None if a is None else a.ctypes.data,
                                                           None if c is None else c.ctypes.data))

    def set_options(self, ratings=None, shuffle_targets=False):
        """ratings (nnz,) parallel to the items: --rf feeds item index + rating index (model: n_feat 2, input_size N + 10);
        shuffle_targets: --shuffle_targets (sbr_dataset_set_options)."""
        r = None if ratings is None else np.ascontiguousarray(ratings, dtype=np.float32)
        self.engine._check(self.lib.sbr_dataset_set_options(self.d, None if r is None else r.ctypes.data, 1 if shuffle_targets else 0))

    def set_target_bias(self, keep_prob=None, n_targets=1, seed=0):
        """--target_bias: keep_prob (n_items,) = (min(pop) / pop) ** bias; the rows of a pass are then planned on the host
        (sbr_dataset_set_target_bias).  None switches back to device-drawn rows."""
        kp = None if keep_prob is None else np.ascontiguousarray(keep_prob, dtype=np.float32)
        self.engine._check(self.lib.sbr_dataset_set_target_bias(self.d, None if kp is None else kp.ctypes.data, int(n_targets),
                                                                int(seed) & 0xFFFFFFFFFFFFFFFF))

    def noise_pass(self, dropout=0.0, swap=0.0, shuf=0.0, shuf_std=0.0, ratings_perturb=0.0, seed=0):
        """Sequence noise for the pass planned next (sbr_dataset_noise_pass; SequenceNoise.__call__)."""
        with self.engine.torch.cuda.device(self.engine.device):
            self.engine._check(self.lib.sbr_dataset_noise_pass(self.d, float(dropout), float(swap), float(shuf), float(shuf_std),
                                                               float(ratings_perturb), int(seed) & 0xFFFFFFFFFFFFFFFF))

    def current_sequences(self, nnz):
        """(items, rating_index, lengths) the next planned pass reads: the noised copy behind noise_pass (tests / tooling)."""
        items, rate = np.zeros(max(1, int(nnz)), np.int32), np.zeros(max(1, int(nnz)), np.int32)
        lens = np.zeros(self.n_users, np.int32)
        with self.engine.torch.cuda.device(self.engine.device):
            self.engine._check(self.lib.sbr_dataset_current_sequences(self.d, items.ctypes.data, rate.ctypes.data, lens.ctypes.data))
        return items[:int(nnz)], rate[:int(nnz)], lens

    def plan_pass(self, order, batch_size):
        o = None if order is None else np.ascontiguousarray(order, dtype=np.int32)
        nb = ctypes.c_int64()
        self.engine._check(self.lib.sbr_dataset_plan_pass(self.d, None if o is None else o.ctypes.data, int(batch_size),
                                                          ctypes.byref(nb)))
        self.n_batches = nb.value
        return nb.value

    def segments(self):
        n = ctypes.c_int64()
        ptrs = [ctypes.POINTER(ctypes.c_int32)() for _ in range(4)]
        self.engine._check(self.lib.sbr_dataset_plan_segments(self.d, ctypes.byref(n), *[ctypes.byref(p) for p in ptrs]))
        return np.stack([np.ctypeslib.as_array(p, shape=(n.value,)).copy() if n.value else np.zeros(0, np.int32)
                         for p in ptrs], axis=1)

    def get_state(self):
        """What makes the next plan_pass reproduce its plan, as bytes (sbr_dataset_state_save): the rows the last planned pass
        carried over, the host row planner's pass counter, the batch size.  Not the sequences, tables and options."""
        return _state_get(self.engine._check, self.lib, "sbr_dataset_state", self.d)

    def set_state(self, blob):
        """sbr_dataset_state_load: ValueError (nothing changed) for a blob of another dataset; plan the next pass afterwards."""
        _state_set(self.engine._check, self.lib, "sbr_dataset_state", self.d, blob)

    def close(self):
        if getattr(self, "d", None):
            self.lib.sbr_dataset_destroy(self.d)
            self.d = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def make_config(cell="GRU", layers=(50,), n_items=None, max_length=30, batch_size=16, loss="CCE", n_samples=0,
                updater="adam", learning_rate=0.001, rho=0.9, beta1=0.9, beta2=0.999, regularization=0.0, grad_clip=100.0,
                input_size=None, n_feat=1, local_batch=None, row_offset=0, flags=0, embedding_size=0, bidirectional=False,
                balance=1.0, n_targets=1, unique=True):
    """sbr_config for the options RNNBase.__init__ / prepare_model fix (include/sbr_rnn.h)."""
    if cell not in CELLS:
        raise ValueError("Unknown layer type")                      # recurrent_layers.py:90
    if loss not in LOSSES:
        raise ValueError("Unknown loss for the RNN model")          # command_parser.py:123
    if updater not in UPDATERS:
        raise ValueError("Unknown update option")                   # update_manager.py:22
    layers = [int(h) for h in layers]
    if len(layers) > SBR_MAX_LAYERS:
        raise ValueError("at most %d recurrent layers" % SBR_MAX_LAYERS)
    cfg = SbrConfig()
    cfg.abi_version = SBR_ABI_VERSION
    cfg.cell = CELLS[cell]
    cfg.n_layers = len(layers)
    for i, hsz in enumerate(layers):
        cfg.layers[i] = hsz
    cfg.n_items = int(n_items)
    cfg.input_size = int(input_size if input_size is not None else n_items)
    cfg.n_feat = int(n_feat)
    cfg.max_length = int(max_length)
    cfg.batch_size = int(batch_size)
    cfg.local_batch = int(local_batch if local_batch is not None else batch_size)
    cfg.row_offset = int(row_offset)
    cfg.loss = LOSSES[loss]
    cfg.n_samples = int(n_samples) if loss in SAMPLED_LOSSES else 0
    cfg.balance, cfg.n_targets, cfg.unique = float(balance), max(1, int(n_targets)) if loss in MARGIN_LOSSES else 1, 1 if unique else 0
    cfg.updater = UPDATERS[updater]
    cfg.learning_rate, cfg.rho, cfg.beta1, cfg.beta2 = learning_rate, rho, beta1, beta2
    cfg.regularization = regularization
    cfg.grad_clip = grad_clip
    cfg.flags = int(flags)
    sp = os.environ.get("SBR_SPARSE_UPDATE")             # 1 / 0 force the row-sparse optimizer on / off (include/sbr_rnn.h)
    if sp is not None and not cfg.flags & (FLAG_SPARSE_UPDATE | FLAG_DENSE_UPDATE):
        cfg.flags |= FLAG_SPARSE_UPDATE if sp not in ("0", "") else FLAG_DENSE_UPDATE
    cfg.embedding_size = max(0, int(embedding_size))     # --r_emb: a size < 1 means no embedding layer
    cfg.bidirectional = 1 if bidirectional else 0        # --r_bi
    return cfg


def describe_params(cfg, lib=None):
    """[(name, shape)] of lasagne.layers.get_all_param_values(l_out) for a configuration (sbr_describe_param: host only,
    no GPU needed)."""
    lib = lib or load_library()
    out, i = [], 0
    name = ctypes.create_string_buffer(96)
    while True:
        dims, nd = (ctypes.c_int64 * 2)(), ctypes.c_int()
        if lib.sbr_describe_param(ctypes.byref(cfg), i, name, 96, dims, ctypes.byref(nd)) != 0:
            if i == 0:
                raise ValueError(lib.sbr_last_error().decode("utf-8", "replace"))
            return out
        out.append((name.value.decode(), tuple(int(d) for d in dims[:nd.value])))
        i += 1


def initial_values(descs, rng, last_layer_init=1.0):
    """Random-init arrays in get_all_param_values order by the initialisers the reference's layers name [3P]: gate weights
    and peepholes of the LSTM / GRU / index-input Vanilla layers Normal(std 0.1) (sparse_lstm.py:143-171 Gate defaults),
    biases and initial states 0, stock RecurrentLayer weights (dense Vanilla layers) init.Uniform() = U(-0.01, 0.01),
    EmbeddingLayer W init.Normal() = std 0.01, output W GlorotUniform(gain) (rnn_one_hot.py:65, rnn_sampling.py:131),
    output b 0.  rng: numpy Generator or RandomState."""
    out = []
    for name, shp in descs:
        base = name.split(".", 1)[1]
        if name == "out.W":
            lim = last_layer_init * np.sqrt(6.0 / (shp[0] + shp[1]))
            a = rng.uniform(-lim, lim, size=shp)
        elif name == "emb.W":
            a = rng.normal(0.0, 0.01, size=shp)
        elif base in ("input_to_hidden.W", "hidden_to_hidden.W"):
            a = rng.uniform(-0.01, 0.01, size=shp)
        elif base.startswith("W_"):
            a = rng.normal(0.0, 0.1, size=shp)
        else:
            a = np.zeros(shp)
        out.append(np.asarray(a, dtype=np.float32))
    return out


class RNNEngine(object):
    """Device-resident model + optimizer state behind the reference's callables.

    train_function / test_function / predict_function take the same tuples the Theano
    functions take (rnn_one_hot.py:61,106; rnn_sampling.py:128,194); `exclude` is accepted
    and ignored in training exactly like the reference (rnn_base.py:185
    on_unused_input='ignore') and derived on the device for the test path.
    """

    def __init__(self, cell="GRU", layers=(50,), n_items=None, max_length=30, batch_size=16, loss="CCE",
                 n_samples=0, updater="adam", learning_rate=0.001, rho=0.9, beta1=0.9, beta2=0.999,
                 regularization=0.0, grad_clip=100.0, input_size=None, n_feat=1, local_batch=None, row_offset=0,
                 flags=0, device=None, embedding_size=0, bidirectional=False, balance=1.0, n_targets=1, unique=True):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("RNNEngine needs a HIP device (MI355X); there is no CPU fallback")
        self.torch = torch
        self.lib = load_library()
        if cell not in CELLS:
            raise ValueError("Unknown layer type")                      # recurrent_layers.py:90
        if loss not in LOSSES:
            raise ValueError("Unknown loss for the RNN model")          # command_parser.py:123
        if updater not in UPDATERS:
            raise ValueError("Unknown update option")                   # update_manager.py:22
        layers = [int(h) for h in layers]
        cfg = make_config(cell=cell, layers=layers, n_items=n_items, max_length=max_length, batch_size=batch_size, loss=loss,
                          n_samples=n_samples, updater=updater, learning_rate=learning_rate, rho=rho, beta1=beta1, beta2=beta2,
                          regularization=regularization, grad_clip=grad_clip, input_size=input_size, n_feat=n_feat,
                          local_batch=local_batch, row_offset=row_offset, flags=flags, embedding_size=embedding_size,
                          bidirectional=bidirectional, balance=balance, n_targets=n_targets, unique=unique)
        self.cfg = cfg
        self.n_targets = cfg.n_targets
        self.cell, self.layers, self.loss = cell, layers, loss
        self.n_items, self.max_length = cfg.n_items, cfg.max_length
        self.batch_size, self.local_batch, self.n_feat = cfg.batch_size, cfg.local_batch, cfg.n_feat
        self.n_samples = cfg.n_samples

        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        nbytes = ctypes.c_size_t()
        self._check(self.lib.sbr_arena_bytes(ctypes.byref(cfg), ctypes.byref(nbytes)))
        self.arena_bytes = nbytes.value
        with torch.cuda.device(self.device):
            self.arena = torch.empty((nbytes.value + 3) // 4, dtype=torch.float32, device=self.device)
            self.stream = torch.cuda.current_stream(self.device)
            handle = ctypes.c_void_p()
            self._check(self.lib.sbr_create(ctypes.byref(cfg), ctypes.c_void_p(self.arena.data_ptr()),
                                            ctypes.c_size_t(self.arena.numel() * 4),
                                            ctypes.c_void_p(self.stream.cuda_stream), ctypes.byref(handle)))
        self.h = handle
        # data-parallel guard (parallel.DataParallel sets it with more than one rank): calls that bring lazily stepped rows of the
        # row-sparse blocks up to date must then be made by every rank at the same step, through DataParallel's collectives
        self.dp_guard = False
        self._dp_collective = False
        self.n_params = self.lib.sbr_num_params(self.h)
        self.param_descs = describe_params(cfg, self.lib)
        self.param_shapes = []
        for i in range(self.n_params):
            dims = (ctypes.c_int64 * 2)()
            nd = ctypes.c_int()
            self._check(self.lib.sbr_param_shape(self.h, i, dims, ctypes.byref(nd)))
            self.param_shapes.append(tuple(int(d) for d in dims[:nd.value]))
        self._sections = {}
        self.evaluate_calls = 0      # calls of evaluate() so far (tests: which road an evaluation took)

    # ---------------------------------------------------------------- plumbing
    def _check(self, rc):
        if rc != 0:
            msg = self.lib.sbr_last_error().decode("utf-8", "replace")
            if rc == -1:
                raise ValueError(msg)
            raise SbrError("libsbr_rnn error %d: %s" % (rc, msg))

    def close(self):
        if getattr(self, "h", None):
            self.lib.sbr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ptr_array(self, arrays):
        arr = (ctypes.c_void_p * len(arrays))()
        for i, a in enumerate(arrays):
            arr[i] = a.ctypes.data
        return arr

    def build_batch(self, dataset, batch, seed):
        """Native batch builder: planned batch `batch` of `dataset` becomes the current batch (no host arrays)."""
        self._check(self.lib.sbr_build_batch(self.h, dataset.d, int(batch), ctypes.c_uint64(int(seed) & (2 ** 64 - 1))))

    def current_batch(self):
        """Host copies of the current batch held in the engine's own buffers (tests/tooling):
        X (B,T), lengths (B,), target, pop (B,), samples (S,)."""
        out = {}
        for name, rows in (("X", self.local_batch * self.max_length * self.n_feat), ("lengths", self.local_batch),
                           ("target", self.batch_size if self.n_samples else self.local_batch * self.n_targets), ("pop", self.local_batch),
                           ("samples", self.n_samples)):
            if rows == 0:
                continue
            buf = self.debug_buffer("batch_" + name)[:rows]
            out[name] = buf if name == "pop" else buf.view(np.int32)
        out["X"] = out["X"].reshape(self.local_batch, self.max_length, self.n_feat)
        return out

    def section(self, which):
        """torch view of a flat arena section: 'params', 'grads' (last element = cost), 'state'.
        Returns (tensor, split) where split = first float of the output-layer part."""
        # (always through the library: for 'params' / 'state' the call also brings lazily updated rows up to date)
        idx = {"params": 0, "grads": 1, "state": 2}[which]
        ptr, n, split = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_size_t()
        self._check(self.lib.sbr_section(self.h, idx, ctypes.byref(ptr), ctypes.byref(n), ctypes.byref(split)))
        if which not in self._sections:
            off = (ptr.value - self.arena.data_ptr()) // 4
            self._sections[which] = (self.arena[off:off + n.value], split.value)
        return self._sections[which]

    # ---------------------------------------------------------------- parameters
    def set_all_param_values(self, values):
        """lasagne.layers.set_all_param_values(l_out, values) (rnn_base.py:515)."""
        if len(values) != self.n_params:
            raise ValueError("mismatch: got %d values to set %d parameters" % (len(values), self.n_params))
        arrays = []
        for v, shp in zip(values, self.param_shapes):
            a = np.ascontiguousarray(np.asarray(v, dtype=np.float32))
            if a.shape != shp:
                raise ValueError("mismatch: parameter has shape %r but value to set has shape %r" % (shp, a.shape))
            arrays.append(a)
        self._check(self.lib.sbr_set_params(self.h, len(arrays), self._ptr_array(arrays)))

    def get_state(self):
        """The whole training state of the engine as bytes (sbr_state_save): parameters, optimizer state, step count, the `last`
        words of lazily stepped rows -- read without a flush, so the run goes on as if the call had not been made.  SbrError
        (SBR_ESTATE) inside an open training step or with a lagged cost pending: flush_lagged() first."""
        with self.torch.cuda.device(self.device):
            return _state_get(self._check, self.lib, "sbr_state", self.h)

    def set_state(self, blob):
        """sbr_state_load: the engine stands at the step boundary the blob was taken at (no current batch, no gradients).  ValueError,
        with the engine untouched, for a blob that is truncated, foreign, or of another architecture or updater.  The same blob
        serves every data-parallel replica."""
        with self.torch.cuda.device(self.device):
            _state_set(self._check, self.lib, "sbr_state", self.h, blob)

    def _get(self, fn):
        arrays = [np.empty(shp, dtype=np.float32) for shp in self.param_shapes]
        self._check(fn(self.h, len(arrays), self._ptr_array(arrays)))
        return arrays

    def _rank_local_flush(self, what):
        """predict / top-k / export / flush replay the zero-gradient steps lazily stepped rows have missed; WHERE a replay is split
        changes float32 roundings, so with several data-parallel ranks a rank-local call would fork the replicas."""
        if self.dp_guard and not self._dp_collective and self.query("sparse_blocks") > 0:
            raise RuntimeError("%s on one data-parallel rank only would bring lazily stepped rows up to date on this replica alone: "
                               "call DataParallel.%s on every rank at the same step (sequence-based-recommendations_amd/parallel.py)"
                               % (what, what))

    def get_all_param_values(self):
        """lasagne.layers.get_all_param_values(l_out) (rnn_base.py:476)."""
        self._rank_local_flush("get_all_param_values")
        return self._get(self.lib.sbr_get_params)

    def get_all_grad_values(self):
        return self._get(self.lib.sbr_get_grads)

    # ---------------------------------------------------------------- batches
    def set_batch(self, X, mask=None, target=None, samples=None, target_popularity=None, lengths=None):
        X = np.ascontiguousarray(np.asarray(X, dtype=np.int32))
        if X.ndim == 2:
            X = X[:, :, None]
        n_rows = X.shape[0]
        if X.shape[1] != self.max_length or X.shape[2] != self.n_feat:
            raise ValueError("X must have shape (rows, %d, %d), got %r" % (self.max_length, self.n_feat, X.shape))
        if lengths is None:
            lengths = mask_to_lengths(mask)
        lengths = np.ascontiguousarray(np.asarray(lengths, dtype=np.int32))
        tgt = None if target is None else np.ascontiguousarray(np.asarray(target, dtype=np.int32))
        smp = None if samples is None else np.ascontiguousarray(np.asarray(samples, dtype=np.int32))
        pop = None if target_popularity is None else np.ascontiguousarray(np.asarray(target_popularity, dtype=np.float32))
        if tgt is not None and self.loss in MARGIN_LOSSES:
            # RNNMargin: (rows, n_targets) positives per row, -1 where a row has fewer (rnn_margin.py:112-147)
            if tgt.ndim == 1:
                tgt = tgt[:, None]
            if tgt.shape[0] != n_rows or tgt.shape[1] > self.n_targets:
                raise ValueError("targets must have shape (%d, <= %d), got %r" % (n_rows, self.n_targets, tgt.shape))
            if tgt.shape[1] < self.n_targets:
                tgt = np.concatenate([tgt, -np.ones((n_rows, self.n_targets - tgt.shape[1]), dtype=np.int32)], axis=1)
            tgt = np.ascontiguousarray(tgt)
        elif tgt is not None:
            need = self.batch_size if self.loss in SAMPLED_LOSSES else n_rows
            if tgt.shape[0] != need:
                raise ValueError("target must have %d entries, got %d" % (need, tgt.shape[0]))
        if self.loss in SAMPLED_LOSSES and smp is not None and smp.shape[0] != self.n_samples:
            raise ValueError("samples must have %d entries" % self.n_samples)
        self._check(self.lib.sbr_set_batch(self.h, _ptr(X), _ptr(lengths), _ptr(tgt), _ptr(smp), _ptr(pop), n_rows, 0))
        return n_rows

    def set_default_target(self, default_target=None):
        """RNNMargin --pb: the default target of every item (RNNMargin._default_target, rnn_margin.py:149-161); None = zeros."""
        a = None if default_target is None else np.ascontiguousarray(np.asarray(default_target, dtype=np.float32))
        if a is not None and a.shape != (self.n_items,):
            raise ValueError("default_target must have %d entries" % self.n_items)
        self._check(self.lib.sbr_set_default_target(self.h, None if a is None else ctypes.c_void_p(a.ctypes.data)))

    def set_batch_device(self, X, lengths, target, samples, target_popularity, n_rows):
        """Same, inputs already resident in HBM (torch int32/float32 tensors on this device)."""
        dp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
        self._check(self.lib.sbr_set_batch(self.h, dp(X), dp(lengths), dp(target), dp(samples), dp(target_popularity),
                                           int(n_rows), 1))

    # ---------------------------------------------------------------- the reference's callables
    def train_function(self, X, mask, target, *rest):
        """cost = train_function(X, mask, target, [samples,] target_popularity, exclude)."""
        if self.loss in MARGIN_LOSSES:      # RNNMargin: target = the positives (rows, n_targets); no popularity weights, no samples
            pop = samples = None
        elif self.loss == "CCE":
            pop = rest[0] if len(rest) > 0 else None
            samples = None
        else:
            samples = rest[0]
            pop = rest[1] if len(rest) > 1 else None
        self.set_batch(X, mask, target, samples, pop)
        return self.train_step(sync=True)

    def train_step(self, sync=True):
        if sync:
            cost = ctypes.c_float()
            self._check(self.lib.sbr_train_step(self.h, ctypes.byref(cost)))
            return float(cost.value)
        self._check(self.lib.sbr_train_step(self.h, None))
        return None

    def train_step_lagged(self):
        """Enqueue a step; returns the cost of the PREVIOUS lagged call (None on the first): the training loop's
        form, the host never waits for the step it has just enqueued.  flush_lagged() returns the last one."""
        cost, have = ctypes.c_float(), ctypes.c_int32()
        self._check(self.lib.sbr_train_step_lagged(self.h, ctypes.byref(cost), ctypes.byref(have)))
        return float(cost.value) if have.value else None

    def cost_lagged(self):
        """Behind apply_update() of a phase-by-phase step (parallel.DataParallel.train_step): enqueues the report of that step's
        cost -- the global one once the gradient section has been all-reduced -- and returns the cost the PREVIOUS lagged call
        reported (None on the first); read_cost() without the wait for the stream.  flush_lagged() returns the last one."""
        cost, have = ctypes.c_float(), ctypes.c_int32()
        self._check(self.lib.sbr_cost_lagged(self.h, ctypes.byref(cost), ctypes.byref(have)))
        return float(cost.value) if have.value else None

    def flush_lagged(self):
        cost, have = ctypes.c_float(), ctypes.c_int32()
        self._check(self.lib.sbr_lagged_flush(self.h, ctypes.byref(cost), ctypes.byref(have)))
        return float(cost.value) if have.value else None

    def forward_backward(self):
        """Gradients without the update (parity tests, data-parallel)."""
        for fn in (self.lib.sbr_zero_grads, self.lib.sbr_forward, self.lib.sbr_loss_backward_output,
                   self.lib.sbr_backward_recurrent):
            self._check(fn(self.h))
        return self.read_cost()

    # phases of one step (data-parallel: all-reduce the gradient section between them)
    def zero_grads(self):
        self._check(self.lib.sbr_zero_grads(self.h))

    def forward(self):
        self._check(self.lib.sbr_forward(self.h))

    def loss_backward_output(self):
        self._check(self.lib.sbr_loss_backward_output(self.h))

    def backward_recurrent(self):
        self._check(self.lib.sbr_backward_recurrent(self.h))

    def apply_update(self):
        self._check(self.lib.sbr_apply_update(self.h))

    def read_cost(self):
        cost = ctypes.c_float()
        self._check(self.lib.sbr_read_cost(self.h, ctypes.byref(cost)))
        return float(cost.value)

    def predict_function(self, X, mask):
        """scores (rows, N): softmax probabilities for CCE, raw activations for sampled heads."""
        self._rank_local_flush("predict_function")
        n = self.set_batch(X, mask)
        out = np.empty((n, self.n_items), dtype=np.float32)
        self._check(self.lib.sbr_predict_scores(self.h, 0, ctypes.c_void_p(out.ctypes.data)))
        return out

    def test_probabilities(self, X, mask):
        n = self.set_batch(X, mask)
        out = np.empty((n, self.n_items), dtype=np.float32)
        self._check(self.lib.sbr_predict_scores(self.h, 1, ctypes.c_void_p(out.ctypes.data)))
        return out

    def test_function(self, theano_inputs, k=10, exclude_seen=True):
        """ids = test_function(theano_inputs, k) (rnn_base.py:205-209): ordered top-k of
        softmax * (1 - exclude), for every row (the reference feeds one row at a time)."""
        self._rank_local_flush("test_function")
        X, mask = theano_inputs[0], theano_inputs[1]
        n = self.set_batch(X, mask)
        ids = np.empty((n, k), dtype=np.int32)
        # exclude_seen: True / 1 = viewed items can never be ranked (top_k_recommendations, rnn_base.py:154-155); 2 = the compiled
        # test function's scores * (1 - exclude) (:201-202): the same ranking except for RNNMargin's raw outputs
        self._check(self.lib.sbr_topk(self.h, int(k), int(exclude_seen), ctypes.c_void_p(ids.ctypes.data)))
        return ids

    def rank(self, X, mask, k, exclude=None, exclude_input=True, return_scores=False):
        """Ordered top-k of any depth 1 <= k <= n_items for every row (sbr_rank): ids (rows, k) int32, score descending, ties to
        the lowest id, -1 where a row runs out of rankable items; with return_scores also their float32 scores (raw activations,
        no softmax; -inf in the unfilled places).  exclude: per row, the ids never to rank (any length, duplicates allowed, None
        or empty for none) -- top_k_recommendations' exclude= and the part of a history that no longer fits the input window;
        exclude_input: also the items of the row's input window, as test_function(exclude_seen=True) does."""
        self._rank_local_flush("rank")
        n = self.set_batch(X, mask)
        ids_arr, off_arr = _excl_csr(exclude, n)
        return self.rank_csr(n, k, ids_arr, off_arr, exclude_input=exclude_input, return_scores=return_scores)

    def rank_csr(self, rows, k, excl_ids=None, excl_off=None, exclude_input=True, return_scores=False):
        """sbr_rank on the batch already set (`rows` rows); the lists as the C-ABI takes them: int32 ids and int64 offsets
        (rows + 1 of them), or None for both."""
        self._rank_local_flush("rank")
        k = _check_k(k, self.n_items)
        ids = np.empty((rows, k), dtype=np.int32)
        scores = np.empty((rows, k), dtype=np.float32) if return_scores else None
        excl_ids, excl_off = _csr_args(excl_ids, excl_off, rows)
        self._check(self.lib.sbr_rank(self.h, k, int(bool(exclude_input)), _ptr(excl_ids), _ptr(excl_off), _ptr(ids), _ptr(scores)))
        return (ids, scores) if return_scores else ids

    def rank_candidates(self, X, mask, k, candidates, exclude=None, exclude_input=True, return_scores=False):
        """rank() restricted to candidate lists (sbr_rank_candidates): for every row the ordered top-k among ITS candidates only,
        without scoring the whole catalogue.  candidates: a sequence of per-row id arrays (any order, duplicates allowed: each is
        sorted and de-duplicated; None or empty: nothing to rank), or a single 1-D array of ids, one list shared by every row.  ids
        (rows, k) int32 and, with return_scores, float32 scores exactly as rank() at k = n_items returns them filtered to the row's
        list; -1 / -inf where a row has fewer than k rankable candidates.  exclude / exclude_input: rank()'s."""
        self._rank_local_flush("rank_candidates")
        n = self.set_batch(X, mask)
        cand_ids, cand_off, shared = _cand_csr(candidates, n)
        ids_arr, off_arr = _excl_csr(exclude, n)
        return self.rank_candidates_csr(n, k, cand_ids, cand_off, shared, ids_arr, off_arr, exclude_input=exclude_input,
                                        return_scores=return_scores)

    def rank_candidates_csr(self, rows, k, cand_ids, cand_off, shared, excl_ids=None, excl_off=None, exclude_input=True,
                            return_scores=False):
        """sbr_rank_candidates on the batch already set (`rows` rows); the lists as the C-ABI takes them: every candidate list
        strictly ascending, int32 ids and int64 offsets (rows + 1 of them, or 2 with shared)."""
        self._rank_local_flush("rank_candidates")
        k = _check_k(k, self.n_items)
        ids = np.empty((rows, k), dtype=np.int32)
        scores = np.empty((rows, k), dtype=np.float32) if return_scores else None
        cand_ids, cand_off = _cand_args(cand_ids, cand_off, shared, rows)
        excl_ids, excl_off = _csr_args(excl_ids, excl_off, rows)
        self._check(self.lib.sbr_rank_candidates(self.h, k, _ptr(cand_ids), _ptr(cand_off), int(bool(shared)), int(bool(exclude_input)),
                                                 _ptr(excl_ids), _ptr(excl_off), _ptr(ids), _ptr(scores)))
        return (ids, scores) if return_scores else ids

    def evaluate(self, dataset, users, k, exclude_mode, want_ids=False, want_mask=True):
        """Whole users of a DeviceDataset evaluated on the device (sbr_evaluate): each user's sequence is split in the middle, the
        last max_length items of the viewed half go in, the ranking to depth k is compared with the rest.  exclude_mode: one of
        EVAL_EXCL_*.  Returns a dict of int32 arrays over the n users, in the order given: "n_pred" (places filled), "hits"
        (|set(goal) & set(top-k)|), "first_hit" (goal[0] among the top-k), "item_hits" (n_items,: how often an item was a correct
        prediction), "hitmask" (uint32 (n, ceil(k / 32)): bit p = the id at place p is a goal item; None without want_mask) and
        "ids" ((n, k), exactly rank()'s, -1 in the unfilled places; None without want_ids)."""
        self._rank_local_flush("evaluate")
        users = np.ascontiguousarray(np.asarray(users, dtype=np.int32).reshape(-1))
        n, k = len(users), _check_k(k, self.n_items)
        out = _eval_record(n, k, self.n_items, want_mask, want_ids)
        self.evaluate_calls += 1
        with self.torch.cuda.device(self.device):
            rec = SbrEvalOut.of(out)
            self._check(self.lib.sbr_evaluate(self.h, dataset.d, _ptr(users) if n else None, n, k, int(exclude_mode),
                                              rec.ids, rec.n_pred, rec.hits, rec.first_hit, rec.hitmask, rec.item_hits))
        return out

    def evaluate_ranks(self, dataset, users, exclude_mode):
        """The place of every goal item in the complete ranking of its user (sbr_evaluate_ranks): users are split, fed and excluded
        as by evaluate(); no k.  Returns a dict: "goal_off" (int64 (n + 1,): user j's goal places are [goal_off[j], goal_off[j + 1]),
        in sequence order), "ranks" (int32 (goal_off[-1],): the index of the goal item in evaluate(k=n_items)'s ids of that user,
        -1 for an item that is never ranked) and "n_rankable" (int32 (n,): that call's n_pred)."""
        self._rank_local_flush("evaluate_ranks")
        users = np.ascontiguousarray(np.asarray(users, dtype=np.int32).reshape(-1))
        n = len(users)
        off, cap = np.asarray(dataset.offsets, dtype=np.int64), 0      # the dataset's host offsets size the result
        if n and users.min() >= 0 and users.max() < len(off) - 1:      # (otherwise the library rejects the users: nothing is written)
            lens = off[1:][users] - off[:-1][users]
            cap = int((lens - lens // 2).sum())
        out = {"ranks": np.empty(cap, dtype=np.int32), "goal_off": np.zeros(n + 1, dtype=np.int64), "n_rankable": np.empty(n, dtype=np.int32)}
        self.evaluate_calls += 1
        with self.torch.cuda.device(self.device):
            self._check(self.lib.sbr_evaluate_ranks(self.h, dataset.d, _ptr(users) if n else None, n, int(exclude_mode), _ptr(out["goal_off"]),
                                                    _ptr(out["ranks"]), cap, _ptr(out["n_rankable"])))
        return out

    def evaluate_positions(self, dataset, users, exclude_mode, min_history=1):
        """The place of the NEXT item at every position of every user's sequence, from one forward pass per chunk
        (sbr_evaluate_positions): user j's first F = min(L - 1, max_length) items are fed from the start of the sequence, and for
        every p = min_history .. F the item x_p is ranked among the scores of the state after p items.  exclude_mode:
        EVAL_EXCL_NONE, or EVAL_EXCL_PREFIX (the items in front of p are never ranked).  Returns a dict: "pos_off" (int64 (n + 1,):
        user j's positions are [pos_off[j], pos_off[j + 1]), in order of p), "ranks" (int32 (pos_off[-1],): the number of
        rankable items in front of x_p, -1 when x_p is not rankable) and "n_rankable" (int32 (pos_off[-1],))."""
        self._rank_local_flush("evaluate_positions")
        users = np.ascontiguousarray(np.asarray(users, dtype=np.int32).reshape(-1))
        n, m = len(users), int(min_history)
        off, cap = np.asarray(dataset.offsets, dtype=np.int64), 0      # the dataset's host offsets size the result
        if n and m >= 1 and users.min() >= 0 and users.max() < len(off) - 1:      # (otherwise the library rejects the call: nothing is written)
            cap = int(position_counts(off[1:][users] - off[:-1][users], self.max_length, m).sum())
        out = {"pos_off": np.zeros(n + 1, dtype=np.int64), "ranks": np.empty(cap, dtype=np.int32), "n_rankable": np.empty(cap, dtype=np.int32)}
        self.evaluate_calls += 1
        with self.torch.cuda.device(self.device):
            self._check(self.lib.sbr_evaluate_positions(self.h, dataset.d, _ptr(users) if n else None, n, m, int(exclude_mode),
                                                        _ptr(out["pos_off"]), _ptr(out["ranks"]), _ptr(out["n_rankable"]), cap))
        return out

    def evaluate_logprob(self, dataset, users, exclude_mode, want_ranks=False):
        """The log-probability of every goal item under the softmax over the rankable items of its user's score row
        (sbr_evaluate_logprob) -- the validation loss: users are split, fed, chunked and excluded as by evaluate_ranks();
        exclude_mode: EVAL_EXCL_NONE, _VIEWED or _WINDOW (an excluded item leaves the softmax; _WINDOW_ZERO is refused).  Returns a
        dict: "goal_off" (evaluate_ranks' layout), "logp" (float32 (goal_off[-1],): log p of the goal item, -inf where it is not
        rankable), "log_z" (float32 (n,): the row's log partition sum, -inf for a row without a rankable item) and, with
        want_ranks, "ranks" and "n_rankable" exactly as evaluate_ranks() returns them, from the same call."""
        self._rank_local_flush("evaluate_logprob")
        users = np.ascontiguousarray(np.asarray(users, dtype=np.int32).reshape(-1))
        n = len(users)
        off, cap = np.asarray(dataset.offsets, dtype=np.int64), 0      # the dataset's host offsets size the result
        if n and users.min() >= 0 and users.max() < len(off) - 1:      # (otherwise the library rejects the users: nothing is written)
            lens = off[1:][users] - off[:-1][users]
            cap = int((lens - lens // 2).sum())
        out = {"goal_off": np.zeros(n + 1, dtype=np.int64), "logp": np.empty(cap, dtype=np.float32), "log_z": np.empty(n, dtype=np.float32)}
        if want_ranks:
            out["ranks"], out["n_rankable"] = np.empty(cap, dtype=np.int32), np.empty(n, dtype=np.int32)
        self.evaluate_calls += 1
        with self.torch.cuda.device(self.device):
            self._check(self.lib.sbr_evaluate_logprob(self.h, dataset.d, _ptr(users) if n else None, n, int(exclude_mode), _ptr(out["goal_off"]),
                                                      _ptr(out["logp"]), cap, _ptr(out["log_z"]), _ptr(out.get("ranks")),
                                                      _ptr(out.get("n_rankable"))))
        return out

    def evaluate_positions_logprob(self, dataset, users, exclude_mode, min_history=1, want_ranks=False):
        """The log-probability of the NEXT item at every position of every user's sequence (sbr_evaluate_positions_logprob):
        evaluate_positions()' users, prefix, positions and layout.  exclude_mode: EVAL_EXCL_NONE, or EVAL_EXCL_PREFIX (the items in
        front of p leave the softmax at p).  Returns a dict: "pos_off", "logp" and "log_z" (float32 (pos_off[-1],)) and, with
        want_ranks, "ranks" and "n_rankable" exactly as evaluate_positions() returns them, from the same call."""
        self._rank_local_flush("evaluate_positions_logprob")
        users = np.ascontiguousarray(np.asarray(users, dtype=np.int32).reshape(-1))
        n, m = len(users), int(min_history)
        off, cap = np.asarray(dataset.offsets, dtype=np.int64), 0      # the dataset's host offsets size the result
        if n and m >= 1 and users.min() >= 0 and users.max() < len(off) - 1:      # (otherwise the library rejects the call: nothing is written)
            cap = int(position_counts(off[1:][users] - off[:-1][users], self.max_length, m).sum())
        out = {"pos_off": np.zeros(n + 1, dtype=np.int64), "logp": np.empty(cap, dtype=np.float32), "log_z": np.empty(cap, dtype=np.float32)}
        if want_ranks:
            out["ranks"], out["n_rankable"] = np.empty(cap, dtype=np.int32), np.empty(cap, dtype=np.int32)
        self.evaluate_calls += 1
        with self.torch.cuda.device(self.device):
            self._check(self.lib.sbr_evaluate_positions_logprob(self.h, dataset.d, _ptr(users) if n else None, n, m, int(exclude_mode),
                                                                _ptr(out["pos_off"]), _ptr(out["logp"]), _ptr(out["log_z"]),
                                                                _ptr(out.get("ranks")), _ptr(out.get("n_rankable")), cap))
        return out

    def debug_row_logprob(self, scores, goal_ids, n_items=None):
        """The test hook of the log-probability reduction (sbr_debug_row_logprob): scores, a float32 device tensor [rows][ld], are
        reduced over their first n_items columns (default: all); goal_ids int32 [rows][G].  Returns (logp float32 [rows][G],
        log_z float32 [rows]) as host arrays."""
        torch = self.torch
        assert scores.dtype == torch.float32 and scores.dim() == 2 and scores.is_contiguous() and scores.is_cuda
        rows, ld = scores.shape
        N = ld if n_items is None else int(n_items)
        goals = torch.as_tensor(np.ascontiguousarray(np.asarray(goal_ids, dtype=np.int32).reshape(rows, -1)), device=scores.device)
        G = goals.shape[1]
        logp = torch.empty((rows, max(G, 1)), dtype=torch.float32, device=scores.device)
        log_z = torch.empty(rows, dtype=torch.float32, device=scores.device)
        with torch.cuda.device(self.device):
            torch.cuda.current_stream().synchronize()      # the tensors were written on torch's stream, the call runs on the engine's
            self._check(self.lib.sbr_debug_row_logprob(self.h, ctypes.c_void_p(scores.data_ptr()), ld, rows, N, ctypes.c_void_p(goals.data_ptr()), G,
                                                       ctypes.c_void_p(logp.data_ptr()), ctypes.c_void_p(log_z.data_ptr())))
        return logp.cpu().numpy()[:, :G], log_z.cpu().numpy()

    def evaluate_candidates(self, dataset, users, exclude_mode, candidates=None, n_negatives=None, seed=0, neg_cdf=None,
                            want_negatives=False):
        """Every goal item ranked among a candidate set of its user (sbr_evaluate_candidates) -- the sampled protocol of the
        sequential-recommendation papers, without scoring the whole catalogue.  Users are split, fed and excluded as by
        evaluate_ranks() (exclude_mode: EVAL_EXCL_NONE, _VIEWED or _WINDOW).  Exactly one source of candidates: `candidates`, one
        id list per user (any order, duplicates allowed: each is sorted and de-duplicated; None or empty: no candidates), or
        `n_negatives` items per user that occur nowhere in its sequence, drawn on the device from (seed, user id) -- uniformly, or
        by the cumulative weights neg_cdf (float64 (n_items,)); sampled_negatives() restates the draw on the host.  Returns a
        dict: "goal_off" (int64 (n + 1,)) and "ranks" (int32 (goal_off[-1],): the rankable candidates in front of the goal item,
        -1 when it is not rankable itself) as evaluate_ranks() lays them out, "n_cand" (int32 (n,): the rankable candidates) and,
        with want_negatives, "negatives" (int32 (n, n_negatives): the ids in draw order, -1 behind the last)."""
        self._rank_local_flush("evaluate_candidates")
        users = np.ascontiguousarray(np.asarray(users, dtype=np.int32).reshape(-1))
        n = len(users)
        if (candidates is None) == (n_negatives is None):
            raise ValueError("evaluate_candidates takes exactly one of candidates= and n_negatives=")
        cand_ids = cand_off = negatives = None
        if candidates is not None:
            if want_negatives or neg_cdf is not None:
                raise ValueError("want_negatives and neg_cdf belong to n_negatives=, not to candidates=")
            lists = list(candidates)
            if len(lists) != n:
                raise ValueError("candidates must hold one id list per user: %d lists for %d users" % (len(lists), n))
            cand_ids, cand_off, _ = _cand_csr(lists, n) if n else (np.zeros(1, np.int32), np.zeros(1, np.int64), False)
            s = 0
        else:
            s = int(n_negatives)
            if not 1 <= s <= min(self.n_items - 1, EVAL_MAX_NEGATIVES):       # (the library checks it too: here before `negatives` is sized by it)
                raise ValueError("n_negatives=%d outside [1,min(N - 1,%d)]" % (s, EVAL_MAX_NEGATIVES))
            neg_cdf = _neg_cdf_arg(neg_cdf, self.n_items)
            negatives = np.empty((n, s), dtype=np.int32) if want_negatives else None
        off, cap = np.asarray(dataset.offsets, dtype=np.int64), 0      # the dataset's host offsets size the result
        if n and users.min() >= 0 and users.max() < len(off) - 1:      # (otherwise the library rejects the users: nothing is written)
            lens = off[1:][users] - off[:-1][users]
            cap = int((lens - lens // 2).sum())
        out = {"ranks": np.empty(cap, dtype=np.int32), "goal_off": np.zeros(n + 1, dtype=np.int64), "n_cand": np.empty(n, dtype=np.int32)}
        self.evaluate_calls += 1
        with self.torch.cuda.device(self.device):
            self._check(self.lib.sbr_evaluate_candidates(self.h, dataset.d, _ptr(users) if n else None, n, int(exclude_mode), _ptr(cand_ids),
                                                         _ptr(cand_off), s, int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(neg_cdf),
                                                         _ptr(out["goal_off"]), _ptr(out["ranks"]), cap, _ptr(out["n_cand"]), _ptr(negatives)))
        if want_negatives:
            out["negatives"] = negatives
        return out

    def sessions(self, capacity, history=0):
        """A SessionPool of `capacity` kept states beside this engine (sbr_sessions_create), each with a ring of its last
        `history` fed ids."""
        return SessionPool(self, capacity, history)

    # ---------------------------------------------------------------- debug / timing
    def debug_buffer(self, name):
        ptr, n = ctypes.c_void_p(), ctypes.c_size_t()
        self._check(self.lib.sbr_debug_buffer(self.h, name.encode(), ctypes.byref(ptr), ctypes.byref(n)))
        out = np.empty(n.value, dtype=np.float32)
        self._check(self.lib.sbr_copy_to_host(self.h, ptr, ctypes.c_void_p(out.ctypes.data), n.value))
        return out

    # ---------------------------------------------------------------- row-sparse blocks (include/sbr_rnn.h)
    def flush_lazy(self):
        """Every lazily stepped row current through the last applied step (sbr_flush_lazy)."""
        self._rank_local_flush("flush_lazy")
        self._check(self.lib.sbr_flush_lazy(self.h))

    def sparse_blocks(self):
        """[(n_rows, row_floats, max_local_rows)] of the row-sparse parameter blocks of this configuration."""
        out = []
        for b in range(self.query("sparse_blocks")):
            v = [ctypes.c_int64() for _ in range(3)]
            self._check(self.lib.sbr_sparse_info(self.h, b, *[ctypes.byref(x) for x in v]))
            out.append(tuple(int(x.value) for x in v))
        return out

    def sparse_pack(self, b):
        """This rank's touched gradient rows of block b: (ids int32 [cap], rows float32 [cap, row_floats], count); the
        first `count` entries are valid.  The tensors are the engine's exchange buffers (reused every step)."""
        if not hasattr(self, "_sp_buf"):
            self._sp_buf = {}
        if b not in self._sp_buf:
            n_rows, w, cap = self.sparse_blocks()[b]
            with self.torch.cuda.device(self.device):
                self._sp_buf[b] = (self.torch.empty(cap, dtype=self.torch.int32, device=self.device),
                                   self.torch.empty((cap, w), dtype=self.torch.float32, device=self.device))
        ids, rows = self._sp_buf[b]
        n = ctypes.c_int32()
        self._check(self.lib.sbr_sparse_pack(self.h, b, ctypes.c_void_p(ids.data_ptr()), ctypes.c_void_p(rows.data_ptr()),
                                             ctypes.byref(n)))
        return ids, rows, int(n.value)

    def sparse_unpack_add(self, b, ids, rows, count):
        """Adds ONE rank's packed rows into the gradient block (call for every rank in rank order, own rows included)."""
        if count:
            assert ids.is_contiguous() and rows.is_contiguous()
        self._check(self.lib.sbr_sparse_unpack_add(self.h, b, ctypes.c_void_p(ids.data_ptr()), ctypes.c_void_p(rows.data_ptr()),
                                                   int(count)))

    def sparse_pack_device(self, b):
        """The touched rows of block b with their count IN BAND and nothing synchronised: (ids int32 [1 + cap] with ids[0] =
        the count, rows float32 [cap, row_floats]) -- the engine's exchange buffers, gathered at their fixed capacity."""
        if not hasattr(self, "_sp_dev"):
            self._sp_dev = {}
        if b not in self._sp_dev:
            n_rows, w, cap = self.sparse_blocks()[b]
            with self.torch.cuda.device(self.device):
                self._sp_dev[b] = (self.torch.empty(cap + 1, dtype=self.torch.int32, device=self.device),
                                   self.torch.empty((cap, w), dtype=self.torch.float32, device=self.device))
        ids, rows = self._sp_dev[b]
        self._check(self.lib.sbr_sparse_pack_device(self.h, b, ctypes.c_void_p(ids.data_ptr()), ctypes.c_void_p(rows.data_ptr())))
        return ids, rows

    def sparse_unpack_add_all(self, b, ids_all, rows_all, world):
        """Adds every rank's gathered rows (ids_all [world, 1 + cap], rows_all [world, cap, row_floats]) in rank order."""
        assert ids_all.is_contiguous() and rows_all.is_contiguous()
        self._check(self.lib.sbr_sparse_unpack_add_all(self.h, b, ctypes.c_void_p(ids_all.data_ptr()),
                                                       ctypes.c_void_p(rows_all.data_ptr()), int(world)))

    def dense_ranges(self):
        """[(lo, hi)] float ranges of the gradient section (trailing cost included) outside the sparse blocks."""
        lo, hi, n = (ctypes.c_int64 * 16)(), (ctypes.c_int64 * 16)(), ctypes.c_int()
        self._check(self.lib.sbr_dense_ranges(self.h, 16, lo, hi, ctypes.byref(n)))
        return [(int(lo[i]), int(hi[i])) for i in range(n.value)]

    def set_deferred_join(self, on=True):
        self._check(self.lib.sbr_set_deferred_join(self.h, 1 if on else 0))

    def join_side(self):
        self._check(self.lib.sbr_join_side(self.h))

    def side_stream(self):
        """torch view of the engine's internal side stream (data-parallel: collectives ordered behind it)."""
        return self.torch.cuda.ExternalStream(self.query("side_stream"), device=self.device)

    def side_stream2(self):
        """... and of the second one (overlapped step tail: the embedding scatter-add runs there)."""
        return self.torch.cuda.ExternalStream(self.query("side_stream2"), device=self.device)

    def tail_ranges(self):
        """Overlapped step tail (query('tail_chunks') >= 2), phase-by-phase step: the float ranges of the gradient section
        that the two consumer streams produce: ((W_in lo, hi) on side_stream2, (W_hid lo, hi) on side_stream)."""
        q = self.query
        return (q("tail_win_lo"), q("tail_win_hi")), (q("tail_whid_lo"), q("tail_whid_hi"))

    def debug_scatter(self, reps=10):
        """the stand-alone scatter-add of the embedding gradient over the current batch (sbr_debug_scatter): (us per launch,
        valid entries, distinct rows)"""
        us, n, r = ctypes.c_float(), ctypes.c_int64(), ctypes.c_int64()
        self._check(self.lib.sbr_debug_scatter(self.h, int(reps), ctypes.byref(us), ctypes.byref(n), ctypes.byref(r)))
        return float(us.value), int(n.value), int(r.value)

    def debug_occupy(self, workgroups, lds_kb, milliseconds):
        """a foreign kernel that holds `workgroups` x `lds_kb` KiB of the chip's LDS for `milliseconds` on a stream of the library's
        own (sbr_debug_occupy; asynchronous); debug_occupy(0, 0, 0) waits for it"""
        self._check(self.lib.sbr_debug_occupy(self.h, int(workgroups), int(lds_kb), int(milliseconds)))

    def query(self, what):
        v = ctypes.c_int64()
        self._check(self.lib.sbr_query(self.h, what.encode(), ctypes.byref(v)))
        return int(v.value)

    def synchronize(self):
        self._check(self.lib.sbr_synchronize(self.h))

    def enable_timing(self, on=True, only=None):
        """on: record the per-phase events of every train step; only="rec_bwd": just the two events around that phase
        (every event record costs the stream a few microseconds)."""
        mode = 0 if not on else 1 if only is None else 2 + PHASE_NAMES.index(only)
        self._check(self.lib.sbr_enable_timing(self.h, mode))

    def phase_times(self):
        us = (ctypes.c_float * SBR_N_PHASES)()
        self._check(self.lib.sbr_phase_times(self.h, us))
        return dict(zip(PHASE_NAMES, [float(v) for v in us]))

    def chain_timing(self, on=True):
        """on: bracket every launch of a recurrent chain kernel (any layer, either direction) with a HIP-event pair from now on;
        off: stop and return {"fwd_us", "bwd_us": device time summed over the launches, "fwd_launches", "bwd_launches"}."""
        if on:
            self._check(self.lib.sbr_chain_times(self.h, 1, None, None))
            return None
        us, n = (ctypes.c_float * 2)(), (ctypes.c_int * 2)()
        self._check(self.lib.sbr_chain_times(self.h, 0, us, n))
        return {"fwd_us": float(us[0]), "bwd_us": float(us[1]), "fwd_launches": int(n[0]), "bwd_launches": int(n[1])}


# ------------------------------------------------------------------------------------------------ stateful sessions
def pad_hidden(H):
    """sbr_pad_hidden (csrc/sbr_common.h): the stored width of a layer of H units"""
    for w in (16, 32, 64, 128, 256, 512):
        if H <= w:
            return w
    return (H + 63) // 64 * 64


def _slot_list(slots):
    return np.ascontiguousarray(np.asarray(slots, dtype=np.int32).reshape(-1))


# ---------------------------------------------------------------- parked sessions (include/sbr_rnn.h "The record of a parked session")
RECORD_VERSION = 1


class RecordLayout(object):
    """Where the fields of a parked session's record lie, from the rule of include/sbr_rnn.h: int64 events, int32 ids[ring_len]
    (ring_len = max(history, 1)), zeros up to a multiple of 16 bytes, then per layer h[Hp] and, LSTM, c[Hp].  at[l] = (byte offset
    of h, byte offset of c or None, Hp); fingerprint: FNV-1a 64 over the 32-bit words (1, cell, L, Hp_0 .., ring_len)."""

    def __init__(self, cell, layers, history):
        self.cell, self.layers, self.history = cell, [int(H) for H in layers], int(history)
        self.ring_len = max(self.history, 1)
        self.head = (8 + 4 * self.ring_len + 15) // 16 * 16
        self.at, off = [], self.head
        for H in self.layers:
            Hp = pad_hidden(H)
            h_at, off = off, off + 4 * Hp
            c_at = None
            if cell == "LSTM":
                c_at, off = off, off + 4 * Hp
            self.at.append((h_at, c_at, Hp))
        self.record_bytes = off
        f = 0xcbf29ce484222325
        for w in [RECORD_VERSION, CELLS[cell], len(self.layers)] + [a[2] for a in self.at] + [self.ring_len]:
            for b in int(w).to_bytes(4, "little"):
                f = ((f ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
        self.fingerprint = f

    def __str__(self):
        return "%s %s ring_len=%d record_bytes=%d fingerprint=%016x" % (self.cell, [a[2] for a in self.at], self.ring_len, self.record_bytes,
                                                                         self.fingerprint)


class SessionRecords(object):
    """n parked sessions: .raw uint8 [n][record_bytes] as sbr_sessions_export writes it, and numpy VIEWS into it -- .events int64 [n],
    .history int32 [n][ring_len] (oldest first, then -1), .h(layer) / .c(layer) float32 [n][Hp].  records[i] (an index, a slice,
    an index array) and SessionRecords.concatenate select and join rows."""

    def __init__(self, layout, raw=None, n=0):
        self.layout = layout
        if raw is None:
            raw = np.zeros((int(n), layout.record_bytes), dtype=np.uint8)
        raw = np.asarray(raw)
        if raw.dtype != np.uint8 or raw.ndim != 2 or raw.shape[1] != layout.record_bytes or not raw.flags["C_CONTIGUOUS"]:
            raise ValueError("SessionRecords: raw must be contiguous uint8 [n][%d], got %s %s" % (layout.record_bytes, raw.dtype, raw.shape))
        self.raw = raw

    @property
    def fingerprint(self):
        return self.layout.fingerprint

    def __len__(self):
        return self.raw.shape[0]

    def _view(self, dtype, at, count):
        return self.raw[:, at:at + count * np.dtype(dtype).itemsize].view(dtype)

    @property
    def events(self):
        return self._view(np.int64, 0, 1)[:, 0]

    @property
    def history(self):
        return self._view(np.int32, 8, self.layout.ring_len)

    def h(self, layer):
        h_at, _, Hp = self.layout.at[layer]
        return self._view(np.float32, h_at, Hp)

    def c(self, layer):
        _, c_at, Hp = self.layout.at[layer]
        if c_at is None:
            raise ValueError("SessionRecords.c: a %s layer has no cell state" % self.layout.cell)
        return self._view(np.float32, c_at, Hp)

    def __getitem__(self, i):
        if isinstance(i, (int, np.integer)):
            i = slice(i, i + 1) if i != -1 else slice(i, None)
        return SessionRecords(self.layout, np.ascontiguousarray(self.raw[i]))

    @staticmethod
    def concatenate(parts):
        parts = list(parts)
        for q in parts[1:]:
            if q.fingerprint != parts[0].fingerprint:
                raise ValueError("SessionRecords.concatenate: records of two layouts: %s and %s" % (parts[0].layout, q.layout))
        return SessionRecords(parts[0].layout, np.concatenate([q.raw for q in parts], axis=0))


# A file of parked sessions: this head, then the n ids the records belong to (slots of a pool: int32; users of a serving.SessionStore:
# int64), then the n records.  magic, version, ring_len, fingerprint, record_bytes, n
PARK_HEAD = "<8sIIQQQ"
PARK_MAGIC_POOL, PARK_MAGIC_STORE = b"SBRSESS1", b"SBRSTOR1"
PARK_FILE_VERSION = 1


def pack_park_file(magic, layout, ids, records):
    """the bytes of a file of parked sessions (PARK_HEAD)"""
    import struct
    ids = np.ascontiguousarray(ids, dtype=np.int32 if magic == PARK_MAGIC_POOL else np.int64).reshape(-1)
    if len(ids) != len(records):
        raise ValueError("pack_park_file: %d ids for %d records" % (len(ids), len(records)))
    head = struct.pack(PARK_HEAD, magic, PARK_FILE_VERSION, layout.ring_len, layout.fingerprint, layout.record_bytes, len(ids))
    return head + ids.tobytes() + records.raw.tobytes()


def parse_park_file(data, magic, layout):
    """(ids, SessionRecords) of a file of parked sessions; the WHOLE head and the length are checked against `magic` and `layout`
    before anything is returned: ValueError with the reason"""
    import struct
    size = struct.calcsize(PARK_HEAD)
    if len(data) < size:
        raise ValueError("parked sessions: the file is cut short: %d bytes, the head alone has %d" % (len(data), size))
    got_magic, version, ring_len, fingerprint, record_bytes, n = struct.unpack(PARK_HEAD, data[:size])
    if got_magic != magic:
        raise ValueError("parked sessions: magic %r, not %r" % (got_magic, magic))
    if version != PARK_FILE_VERSION:
        raise ValueError("parked sessions: file version %d, this code reads version %d" % (version, PARK_FILE_VERSION))
    if fingerprint != layout.fingerprint:
        raise ValueError("parked sessions: layout fingerprint %016x (ring_len=%d, record_bytes=%d) in the file, the pool has %s"
                         % (fingerprint, ring_len, record_bytes, layout))
    if record_bytes != layout.record_bytes or ring_len != layout.ring_len:
        raise ValueError("parked sessions: record_bytes=%d ring_len=%d in the file, the pool has %s" % (record_bytes, ring_len, layout))
    id_type = np.dtype(np.int32 if magic == PARK_MAGIC_POOL else np.int64)
    want = size + n * id_type.itemsize + n * record_bytes
    if len(data) != want:
        raise ValueError("parked sessions: the file is cut short or overlong: %d bytes, %d records need %d" % (len(data), n, want))
    ids = np.frombuffer(data, dtype=id_type, count=n, offset=size).copy()
    raw = np.frombuffer(data, dtype=np.uint8, count=n * record_bytes, offset=size + n * id_type.itemsize).reshape(n, record_bytes).copy()
    return ids, SessionRecords(layout, raw)


def write_replacing(path, data):
    """`data` to a temporary name beside `path`, then moved into place: a reader never sees half a file"""
    tmp = "%s.tmp.%d" % (path, os.getpid())
    with open(tmp, "wb") as f:
        f.write(data)
    os.replace(tmp, path)


class SessionPool(object):
    """Kept recurrent states beside an RNNEngine (include/sbr_rnn.h "Stateful sessions", csrc/sbr_session.hip): slot s holds the
    state of one user after all the events fed to it, so the user's next event costs one recurrent step (advance) and one projection
    (rank) where RNNEngine.rank feeds the whole history again.  A state is "after p items fed from the start of the sequence"
    (evaluate_positions' definition): no mask, no window of max_length.  Close the pool before the engine."""

    def __init__(self, engine, capacity, history=0):
        self.engine, self.lib = engine, engine.lib
        self.capacity, self.history = int(capacity), int(history)
        handle = ctypes.c_void_p()
        with engine.torch.cuda.device(engine.device):
            engine._check(self.lib.sbr_sessions_create(engine.h, self.capacity, self.history, ctypes.byref(handle)))
        self.s = handle
        # the record of a parked session: Python's offsets (the views of SessionRecords) against the library's record
        self.layout = RecordLayout(engine.cell, engine.layers, self.history)
        nbytes, fp = ctypes.c_size_t(), ctypes.c_uint64()
        self._check(self.lib.sbr_sessions_record_layout(ctypes.byref(engine.cfg), self.history, ctypes.byref(nbytes), ctypes.byref(fp)))
        if (nbytes.value, fp.value) != (self.layout.record_bytes, self.layout.fingerprint):
            self.close()
            raise SbrError("SessionPool: the library's record has %d bytes, fingerprint %016x; engine.RecordLayout says %s"
                           % (nbytes.value, fp.value, self.layout))

    def _check(self, rc):
        self.engine._check(rc)

    def close(self):
        if getattr(self, "s", None):
            if getattr(self.engine, "h", None):      # (an engine already destroyed took its stream along: nothing left to wait for)
                self.lib.sbr_sessions_destroy(self.s)
            self.s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, slots=None):
        """the named slots (None: all) take the current hid_init / cell_init, 0 events, an empty history"""
        if slots is None:
            self._check(self.lib.sbr_sessions_reset(self.s, None, 0))
            return
        slots = _slot_list(slots)
        self._check(self.lib.sbr_sessions_reset(self.s, _ptr(slots), len(slots)))

    def advance(self, slots, items, second=None):
        """one event per named slot: items[r] (and second[r], a model with n_feat == 2) is fed to slots[r]; slots distinct"""
        self.engine._rank_local_flush("SessionPool.advance")
        slots, items = _slot_list(slots), _slot_list(items)
        if len(items) != len(slots):
            raise ValueError("advance: %d items for %d slots" % (len(items), len(slots)))
        if second is not None:
            second = _slot_list(second)
            if len(second) != len(slots):
                raise ValueError("advance: %d second indices for %d slots" % (len(second), len(slots)))
        with self.engine.torch.cuda.device(self.engine.device):
            self._check(self.lib.sbr_sessions_advance(self.s, _ptr(slots), _ptr(items), _ptr(second), len(slots)))

    @staticmethod
    def _event_lists(what, slots, sequences, second):
        """ragged lists -> the CSR of replay / replay_ranks: (slots, items, off, second)"""
        slots = _slot_list(slots)
        sequences = [_slot_list(q) for q in sequences]
        if len(sequences) != len(slots):
            raise ValueError("%s: %d sequences for %d slots" % (what, len(sequences), len(slots)))
        off = np.zeros(len(slots) + 1, dtype=np.int64)
        np.cumsum([len(q) for q in sequences], out=off[1:])
        items = np.concatenate(sequences + [np.zeros(0, dtype=np.int32)]).astype(np.int32, copy=False)
        if second is not None:
            second = [_slot_list(q) for q in second]
            if len(second) != len(slots):
                raise ValueError("%s: %d second-index sequences for %d slots" % (what, len(second), len(slots)))
            for r, (a, b) in enumerate(zip(sequences, second)):
                if len(a) != len(b):
                    raise ValueError("%s: row %d has %d items and %d second indices" % (what, r, len(a), len(b)))
            second = np.concatenate(second + [np.zeros(0, dtype=np.int32)]).astype(np.int32, copy=False)
        return slots, items, off, second

    @staticmethod
    def _event_csr(what, slots, items, off, second):
        """the CSR as the C-ABI takes it: converted to its types, contiguous, the lengths checked"""
        slots, items = _slot_list(slots), _slot_list(items)
        off = np.ascontiguousarray(np.asarray(off, dtype=np.int64).reshape(-1))
        if len(off) != len(slots) + 1:
            raise ValueError("%s: off must have %d entries (slots + 1), got %d" % (what, len(slots) + 1, len(off)))
        if int(off.max()) > len(items):      # (the library reads items up to there; the order of off is its own check)
            raise ValueError("%s: off reaches %d, but there are %d items" % (what, int(off.max()), len(items)))
        if second is not None:
            second = _slot_list(second)
            if len(second) != len(items):
                raise ValueError("%s: %d second indices for %d items" % (what, len(second), len(items)))
        return slots, items, off, second

    def replay(self, slots, sequences, second=None):
        """a run of events per named slot in one launch (sbr_sessions_replay): sequences[r], a 1-D id array of any length (and
        second[r] of the same length, a model with n_feat == 2), is fed to slots[r] in order FROM THE SLOT'S KEPT STATE -- bit for
        bit what one advance per event leaves.  This, not adopt, is the road for histories longer than max_length and for continuing
        a kept state."""
        self.replay_csr(*self._event_lists("replay", slots, sequences, second))

    def replay_csr(self, slots, items, off, second=None):
        """sbr_sessions_replay with the lists as the C-ABI takes them: int32 ids, int64 offsets (len(slots) + 1, off[0] == 0,
        non-decreasing): items[off[r] : off[r + 1]] go to slots[r], oldest first"""
        self.engine._rank_local_flush("SessionPool.replay")
        slots, items, off, second = self._event_csr("replay", slots, items, off, second)
        with self.engine.torch.cuda.device(self.engine.device):
            self._check(self.lib.sbr_sessions_replay(self.s, _ptr(slots), len(slots), _ptr(items), _ptr(second), _ptr(off)))

    def replay_ranks(self, slots, sequences, second=None, exclude=SESSION_EXCL_HISTORY, group_rows=0):
        """replay() that also ranks every event before it is fed (sbr_sessions_replay_ranks): the pool is left exactly as replay
        leaves it, and for event t of row r -- at off[r] + t of the flat result -- `ranks` holds the place of the item fed among the
        scores rank(slots[r], exclude=exclude) would have ranked at that moment (-1: not rankable there), `n_rankable` the rankable
        items, `events_before` the events the slot had in front of it (int64).  Equal, integer for integer, to the loop
        "rank at k = n_items, find the item, advance"; group_rows bounds the scratch (0: the library's default) and changes nothing
        else.  Returns {"off", "ranks", "n_rankable", "events_before"}."""
        return self.replay_ranks_csr(*self._event_lists("replay_ranks", slots, sequences, second), exclude=exclude, group_rows=group_rows)

    def replay_ranks_csr(self, slots, items, off, second=None, exclude=SESSION_EXCL_HISTORY, group_rows=0):
        """sbr_sessions_replay_ranks with the lists as the C-ABI takes them (replay_csr's)"""
        self.engine._rank_local_flush("SessionPool.replay_ranks")
        slots, items, off, second = self._event_csr("replay_ranks", slots, items, off, second)
        n, total = len(slots), int(off[-1])
        ranks, nrk = np.empty(total, dtype=np.int32), np.empty(total, dtype=np.int32)
        before = np.zeros(n, dtype=np.int64)
        with self.engine.torch.cuda.device(self.engine.device):
            self._check(self.lib.sbr_sessions_replay_ranks(self.s, _ptr(slots), n, _ptr(items), _ptr(second), _ptr(off), int(exclude),
                                                           int(group_rows), _ptr(ranks), _ptr(nrk), _ptr(before)))
        lens = off[1:] - off[:-1]
        # event t of row r had e0[r] + t events in front of it
        events_before = np.repeat(before, lens) + np.arange(total, dtype=np.int64) - np.repeat(off[:-1], lens)
        return {"off": off, "ranks": ranks, "n_rankable": nrk, "events_before": events_before}

    def adopt(self, slots):
        """rows 0 .. len(slots) - 1 of the engine's current batch become the named sessions: their state at the row's length from
        the chain kernels' forward pass, the length as event count, the last `history` fed ids"""
        self.engine._rank_local_flush("SessionPool.adopt")
        slots = _slot_list(slots)
        with self.engine.torch.cuda.device(self.engine.device):
            self._check(self.lib.sbr_sessions_adopt(self.s, _ptr(slots), len(slots)))

    def rank(self, slots, k, exclude=SESSION_EXCL_HISTORY, excl_ids=None, excl_off=None, return_scores=False):
        """Ordered top-k of the next item for the named slots, exactly as RNNEngine.rank_csr returns it: ids (n, k) int32, with
        return_scores also their float32 scores.  exclude: SESSION_EXCL_NONE / _LAST / _HISTORY (only the last `history` ids of a
        longer session are excluded); excl_ids / excl_off: a CSR of further ids per row."""
        self.engine._rank_local_flush("SessionPool.rank")
        slots = _slot_list(slots)
        n, k = len(slots), _check_k(k, self.engine.n_items)
        ids = np.empty((n, k), dtype=np.int32)
        scores = np.empty((n, k), dtype=np.float32) if return_scores else None
        excl_ids, excl_off = _csr_args(excl_ids, excl_off, n)
        with self.engine.torch.cuda.device(self.engine.device):
            self._check(self.lib.sbr_sessions_rank(self.s, _ptr(slots), n, k, int(exclude), _ptr(excl_ids), _ptr(excl_off), _ptr(ids),
                                                   _ptr(scores)))
        return (ids, scores) if return_scores else ids

    def rank_candidates(self, slots, k, candidates, exclude=SESSION_EXCL_HISTORY, excl_ids=None, excl_off=None, return_scores=False):
        """rank() restricted to candidate lists (sbr_sessions_rank_candidates): candidates as RNNEngine.rank_candidates takes them --
        one id array per named slot (sorted and de-duplicated here), or a single 1-D array shared by all of them.  The result equals
        rank(k = n_items) filtered to each row's list."""
        slots = _slot_list(slots)
        cand_ids, cand_off, shared = _cand_csr(candidates, len(slots))
        return self.rank_candidates_csr(slots, k, cand_ids, cand_off, shared, exclude=exclude, excl_ids=excl_ids, excl_off=excl_off,
                                        return_scores=return_scores)

    def rank_candidates_csr(self, slots, k, cand_ids, cand_off, shared, exclude=SESSION_EXCL_HISTORY, excl_ids=None, excl_off=None,
                            return_scores=False):
        """sbr_sessions_rank_candidates with the lists as the C-ABI takes them: every candidate list strictly ascending, int32 ids
        and int64 offsets (len(slots) + 1 of them, or 2 with shared)"""
        self.engine._rank_local_flush("SessionPool.rank_candidates")
        slots = _slot_list(slots)
        n, k = len(slots), _check_k(k, self.engine.n_items)
        ids = np.empty((n, k), dtype=np.int32)
        scores = np.empty((n, k), dtype=np.float32) if return_scores else None
        cand_ids, cand_off = _cand_args(cand_ids, cand_off, shared, n)
        excl_ids, excl_off = _csr_args(excl_ids, excl_off, n)
        with self.engine.torch.cuda.device(self.engine.device):
            self._check(self.lib.sbr_sessions_rank_candidates(self.s, _ptr(slots), n, k, _ptr(cand_ids), _ptr(cand_off), int(bool(shared)),
                                                              int(exclude), _ptr(excl_ids), _ptr(excl_off), _ptr(ids), _ptr(scores)))
        return (ids, scores) if return_scores else ids

    def read(self, slot, layer, padded=False):
        """the state of `slot` in `layer`: {"h": (H,) float32, "c": the same for LSTM else None, "events": fed so far, "history":
        the last min(events, history) ids, oldest first}; padded: h and c at their stored width"""
        H = int(self.engine.layers[layer]) if 0 <= int(layer) < len(self.engine.layers) else 1
        Hp = pad_hidden(H)
        h = np.zeros(Hp, dtype=np.float32)
        c = np.zeros(Hp, dtype=np.float32) if self.engine.cell == "LSTM" else None
        ev = ctypes.c_int64()
        hist = np.full(max(self.history, 1), -1, dtype=np.int32)
        self._check(self.lib.sbr_sessions_read(self.s, int(slot), int(layer), _ptr(h), _ptr(c), ctypes.byref(ev), _ptr(hist)))
        w = Hp if padded else H
        hist = hist[:self.history]
        return {"h": h[:w], "c": None if c is None else c[:w], "events": int(ev.value), "history": hist[hist >= 0].copy()}

    def write(self, slot, layer, h, c=None):
        """puts a state read earlier back (H or stored-width values; padded units of the former are zero); events and history stay"""
        H = int(self.engine.layers[layer]) if 0 <= int(layer) < len(self.engine.layers) else 1
        Hp = pad_hidden(H)

        def stored(a):
            a = np.asarray(a, dtype=np.float32).reshape(-1)
            if len(a) not in (H, Hp):
                raise ValueError("write: %d values for a layer of %d units (stored width %d)" % (len(a), H, Hp))
            out = np.zeros(Hp, dtype=np.float32)
            out[:len(a)] = a
            return out
        h = stored(h)
        c = None if c is None else stored(c)
        self._check(self.lib.sbr_sessions_write(self.s, int(slot), int(layer), _ptr(h), _ptr(c)))

    def export_records(self, slots, chunk_slots=0):
        """the named sessions off the device (sbr_sessions_export; the slots may repeat): SessionRecords that import_records puts
        into any slot of any pool of the same layout.  One wait, however many slots; chunk_slots bounds the staging buffer on the
        device (0: the library's default) and changes nothing else."""
        slots = _slot_list(slots)
        out = SessionRecords(self.layout, n=len(slots))
        with self.engine.torch.cuda.device(self.engine.device):
            self._check(self.lib.sbr_sessions_export(self.s, _ptr(slots), len(slots), int(chunk_slots), _ptr(out.raw), out.raw.nbytes))
        return out

    def import_records(self, slots, records, chunk_slots=0):
        """records[r] becomes slot slots[r] (distinct; sbr_sessions_import): event count, the whole history ring and the state of
        every layer -- afterwards the slot is the session the record was exported from, through every call of the pool"""
        slots = _slot_list(slots)
        if records.fingerprint != self.layout.fingerprint:
            raise ValueError("import_records: records of another layout: %s; this pool has %s" % (records.layout, self.layout))
        if len(records) != len(slots):
            raise ValueError("import_records: %d records for %d slots" % (len(records), len(slots)))
        with self.engine.torch.cuda.device(self.engine.device):
            self._check(self.lib.sbr_sessions_import(self.s, _ptr(slots), len(slots), int(chunk_slots), _ptr(records.raw), records.raw.nbytes))

    def save(self, path, slots=None):
        """the named slots (None: every slot) to a file (PARK_HEAD), written beside `path` and moved into place"""
        slots = np.arange(self.capacity, dtype=np.int32) if slots is None else _slot_list(slots)
        write_replacing(path, pack_park_file(PARK_MAGIC_POOL, self.layout, slots, self.export_records(slots)))

    def load(self, path, slots=None):
        """the sessions of a file written by save into the slot numbers saved (slots: into these instead, one per record); the whole
        head and the file's length are checked before the pool is touched (ValueError with the reason).  Returns the slots."""
        with open(path, "rb") as f:
            saved, records = parse_park_file(f.read(), PARK_MAGIC_POOL, self.layout)
        slots = saved if slots is None else _slot_list(slots)
        if len(slots) != len(records):
            raise ValueError("load: %d slots for the %d records of %s" % (len(slots), len(records), path))
        self.import_records(slots, records)
        return slots


# ------------------------------------------------------------------------------------------------ RNNCluster's cluster head
CLUSTER_TYPES = {"mix": 0, "softmax": 1, "sigmoid": 2}            # --cluster_type (command_parser.py:77)


class SbrClusterConfig(ctypes.Structure):
    _fields_ = [("abi_version", ctypes.c_int32), ("n_items", ctypes.c_int32), ("n_hidden", ctypes.c_int32),
                ("hidden_split", ctypes.c_int32), ("n_clusters", ctypes.c_int32), ("cluster_type", ctypes.c_int32),
                ("loss", ctypes.c_int32), ("batch_size", ctypes.c_int32), ("max_samples", ctypes.c_int32), ("updater", ctypes.c_int32),
                ("learning_rate", ctypes.c_float), ("rho", ctypes.c_float), ("beta1", ctypes.c_float), ("beta2", ctypes.c_float),
                ("scale", ctypes.c_float), ("noise_std", ctypes.c_float), ("seed", ctypes.c_uint64)]


class ClusterHead(object):
    """The cluster head of RNNCluster beside an RNNEngine (include/sbr_rnn.h, csrc/sbr_cluster.hip): owns the repartition R (N, C)
    and the selection weights Wc (H, C), reads the engine's user representation on the device, trains with its own updater state
    (rnn_cluster.py:237-256, :282-285).  `loss` uses the engine's names (RNNCluster's "CCE" is "SCCE")."""

    def __init__(self, engine, n_clusters, cluster_type="mix", loss="SCCE", max_samples=32, updater="adam", learning_rate=0.01,
                 rho=0.9, beta1=0.9, beta2=0.999, scale=1.0, noise_std=0.0, seed=0):
        if cluster_type not in CLUSTER_TYPES:
            raise ValueError("Unknown cluster type")
        if loss not in SAMPLED_LOSSES:
            raise ValueError("Unknown cluster loss")                     # rnn_cluster.py:101
        self.engine, self.lib, self.torch = engine, engine.lib, engine.torch
        H = int(engine.cfg.layers[engine.cfg.n_layers - 1])
        self.bi = bool(engine.cfg.bidirectional)
        self.n_items, self.n_clusters, self.n_hidden = engine.n_items, int(n_clusters), H * (2 if self.bi else 1)
        self.batch_size, self.max_samples = engine.batch_size, int(max_samples)
        c = SbrClusterConfig()
        c.abi_version, c.n_items, c.n_hidden, c.hidden_split = SBR_ABI_VERSION, self.n_items, self.n_hidden, H
        c.n_clusters, c.cluster_type, c.loss = self.n_clusters, CLUSTER_TYPES[cluster_type], LOSSES[loss]
        c.batch_size, c.max_samples, c.updater = self.batch_size, self.max_samples, UPDATERS[updater]
        c.learning_rate, c.rho, c.beta1, c.beta2 = float(learning_rate), float(rho), float(beta1), float(beta2)
        c.scale, c.noise_std, c.seed = float(scale), float(noise_std), int(seed)
        self.h = self.lib.sbr_cluster_create(ctypes.byref(c), ctypes.c_void_p(engine.stream.cuda_stream))
        if not self.h:
            raise SbrError("sbr_cluster_create: %s" % self.lib.sbr_last_error().decode())
        dev = engine.device
        self._tgt = self.torch.empty(self.batch_size, dtype=self.torch.int32, device=dev)
        self._smp = self.torch.empty(self.max_samples, dtype=self.torch.int32, device=dev)
        self._csel = self.torch.empty(max(self.batch_size, 16), dtype=self.torch.int32, device=dev)
        self._hard = None
        self._lists = None
        self.evaluate_calls = 0      # calls of evaluate() so far (tests: which road an evaluation took)

    def _check(self, rc):
        if rc != 0:
            raise SbrError("libsbr_rnn error %d: %s" % (rc, self.lib.sbr_last_error().decode()))

    def _h_last(self):
        """(device pointer, row stride, offset of the backwards half) of the engine's user representation"""
        ptr, n = ctypes.c_void_p(), ctypes.c_size_t()
        self.engine._check(self.lib.sbr_debug_buffer(self.engine.h, b"h_last", ctypes.byref(ptr), ctypes.byref(n)))
        Bp = (self.engine.batch_size + 15) // 16 * 16
        ld = n.value // Bp
        return ptr, ld, (ld // 2 if self.bi else 0)

    def close(self):
        if self.h:
            self.lib.sbr_cluster_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_params(self, R, Wc):
        R = np.ascontiguousarray(R, dtype=np.float32); Wc = np.ascontiguousarray(Wc, dtype=np.float32)
        if R.shape != (self.n_items, self.n_clusters) or Wc.shape != (self.n_hidden, self.n_clusters):
            raise ValueError("mismatch: cluster arrays have shapes %r, %r" % (R.shape, Wc.shape))
        self._check(self.lib.sbr_cluster_set_params(self.h, ctypes.c_void_p(R.ctypes.data), ctypes.c_void_p(Wc.ctypes.data)))
        self._hard = None
        self._lists = None

    def _get(self, fn):
        R = np.empty((self.n_items, self.n_clusters), dtype=np.float32); Wc = np.empty((self.n_hidden, self.n_clusters), dtype=np.float32)
        self._check(fn(self.h, ctypes.c_void_p(R.ctypes.data), ctypes.c_void_p(Wc.ctypes.data)))
        return R, Wc

    def get_params(self):
        return self._get(self.lib.sbr_cluster_get_params)

    def get_grads(self):
        return self._get(self.lib.sbr_cluster_get_grads)

    def set_scale(self, scale):
        self._check(self.lib.sbr_cluster_set_scale(self.h, float(scale)))

    def get_state(self):
        """The head's training state as bytes (sbr_cluster_state_save): R, Wc, their optimizer state, the step count, the noise
        counter, the scale and the seed."""
        with self.torch.cuda.device(self.engine.device):
            return _state_get(self.engine._check, self.lib, "sbr_cluster_state", self.h)

    def set_state(self, blob):
        """sbr_cluster_state_load: ValueError (nothing changed) for a blob of another head; the hard clusters are dropped."""
        with self.torch.cuda.device(self.engine.device):
            _state_set(self.engine._check, self.lib, "sbr_cluster_state", self.h, blob)
        self._hard = None
        self._lists = None

    def forward_backward(self, targets, cluster_samples, read_cost=True):
        """cost_clusters and its gradients on the engine's CURRENT user representations (call after engine.forward / a step)."""
        t = np.ascontiguousarray(targets, dtype=np.int32); sm = np.ascontiguousarray(cluster_samples, dtype=np.int32)
        if t.shape[0] != self.batch_size or not 1 <= sm.shape[0] <= self.max_samples:
            raise ValueError("cluster head: %d targets, %d samples (batch %d, at most %d samples)" % (t.shape[0], sm.shape[0], self.batch_size, self.max_samples))
        self._tgt.copy_(self.torch.from_numpy(t)); self._smp[:sm.shape[0]].copy_(self.torch.from_numpy(sm))
        ptr, ld, off2 = self._h_last()
        cost = ctypes.c_float()
        self._check(self.lib.sbr_cluster_forward_backward(self.h, ptr, ld, off2, ctypes.c_void_p(self._tgt.data_ptr()),
                                                          ctypes.c_void_p(self._smp.data_ptr()), int(sm.shape[0]),
                                                          ctypes.byref(cost) if read_cost else None))
        self._last_j = self.batch_size + int(sm.shape[0])
        return float(cost.value) if read_cost else None

    def apply_update(self):
        self._check(self.lib.sbr_cluster_apply_update(self.h))
        self._hard = None
        self._lists = None

    def train_step_lagged(self, dataset, n_cluster_samples, seed):
        """One training iteration of both models on the engine's current, device-built batch (sbr_cluster_train_step_lagged): the
        network's lagged step, this head's forward/backward on the user representations of that step -- targets: the batch's;
        cluster samples: the batch's negatives (n_cluster_samples == 0) or that many ids drawn on the device by the law of
        `dataset` (a DeviceDataset) from `seed` -- and this head's update.  Nothing is waited for and nothing is copied from the host.
        Returns the network's cost of the PREVIOUS lagged call (None on the first); flush_lagged() returns the last one."""
        n = int(n_cluster_samples)
        cost, have = ctypes.c_float(), ctypes.c_int32()
        # (the engine's mapping of the status: SBR_EINVAL is a ValueError)
        self.engine._check(self.lib.sbr_cluster_train_step_lagged(self.h, self.engine.h, dataset.d, n, ctypes.c_uint64(int(seed) & (2 ** 64 - 1)),
                                                                  ctypes.byref(cost), ctypes.byref(have)))
        self._last_j = self.batch_size + (n if n > 0 else self.engine.n_samples)
        self._hard = None
        self._lists = None
        return float(cost.value) if have.value else None

    def flush_lagged(self):
        """the network's cost of the last lagged step (None if there is none to collect): RNNEngine.flush_lagged"""
        return self.engine.flush_lagged()

    def last_ids(self):
        """The id list of the last forward/backward (tests and tooling): targets ++ cluster samples, int32 (J,).  Waits for the stream."""
        j = getattr(self, "_last_j", 0)
        if j <= 0:
            raise SbrError("ClusterHead.last_ids: no forward/backward yet")
        ids = np.empty(j, dtype=np.int32)
        self.engine._check(self.lib.sbr_cluster_last_ids(self.h, _ptr(ids), j))
        return ids

    def select(self, rows, with_activations=False):
        """argmax cluster of the first `rows` user representations (rnn_cluster.py:334) [, the selection activations]"""
        ptr, ld, off2 = self._h_last()
        z = self.torch.empty((rows, self.n_clusters), dtype=self.torch.float32, device=self.engine.device) if with_activations else None
        self._check(self.lib.sbr_cluster_select(self.h, ptr, ld, off2, int(rows), ctypes.c_void_p(self._csel.data_ptr()),
                                                ctypes.c_void_p(z.data_ptr()) if z is not None else None))
        csel = self._csel[:rows].cpu().numpy().astype(np.int64)
        return (csel, z.cpu().numpy()) if with_activations else csel

    def hard_clusters(self):
        """_get_hard_clusters() (rnn_cluster.py:293-300) as a host array (N, C); cached until the arrays change"""
        if self._hard is None:
            out = np.empty((self.n_items, self.n_clusters), dtype=np.float32)
            self._check(self.lib.sbr_cluster_hard(self.h, ctypes.c_void_p(out.ctypes.data)))
            self._hard = out
        return self._hard

    def mask_scores(self, scores_dev, csel, want_used=True):
        """device form: scores_dev (rows, >= N) float32 tensor *= hard[:, csel[row]]; returns the items per selected cluster"""
        rows = int(scores_dev.shape[0])
        self._csel[:rows].copy_(self.torch.from_numpy(np.ascontiguousarray(csel, dtype=np.int32)))
        used = self.torch.empty(rows, dtype=self.torch.float32, device=self.engine.device) if want_used else None
        self._check(self.lib.sbr_cluster_mask_scores(self.h, ctypes.c_void_p(scores_dev.data_ptr()), int(scores_dev.stride(0)), rows,
                                                     ctypes.c_void_p(self._csel.data_ptr()),
                                                     ctypes.c_void_p(used.data_ptr()) if used is not None else None))
        return used.cpu().numpy() if used is not None else None

    def cluster_lists(self):
        """The hard clusters of prepare_tests (rnn_cluster.py:440-466) as a list of C ascending int32 id arrays, built on the device
        (sbr_cluster_lists): cluster j holds every item whose membership R[i][j] is positive, and every item without a positive
        membership whose largest one -- the first of them -- is R[i][j].  Cached until the arrays change."""
        if self._lists is None:
            sizes = np.empty(self.n_clusters, dtype=np.int32)
            self._check(self.lib.sbr_cluster_lists(self.h, ctypes.c_void_p(sizes.ctypes.data), None))
            members = np.empty(max(int(sizes.sum()), 1), dtype=np.int32)
            self._check(self.lib.sbr_cluster_lists(self.h, ctypes.c_void_p(sizes.ctypes.data), ctypes.c_void_p(members.ctypes.data)))
            bounds = np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)])
            self._lists = [members[bounds[j]:bounds[j + 1]].copy() for j in range(self.n_clusters)]
        return self._lists

    def rank(self, X, mask, k, exclude=None, exclude_input=True, return_scores=False):
        """RNNEngine.rank inside each row's cluster (sbr_cluster_rank): the row's cluster is the arg-max of its selection activations,
        only that cluster's items (cluster_lists) are scored and ranked.  Returns (ids (rows, k) int32, [scores (rows, k) float32,]
        clusters (rows,) int32, sizes (rows,) int32): ids score descending, ties to the lowest id, -1 (-inf) where the row runs out
        of rankable members -- k may exceed the cluster's size; sizes = items in the row's cluster before any exclusion.  `exclude`,
        `exclude_input` as in RNNEngine.rank; an excluded id outside the row's cluster changes nothing."""
        eng = self.engine
        eng._rank_local_flush("rank")
        n = eng.set_batch(X, mask)
        ids_arr, off_arr = _excl_csr(exclude, n)
        return self.rank_csr(n, k, ids_arr, off_arr, exclude_input=exclude_input, return_scores=return_scores)

    def rank_csr(self, rows, k, excl_ids=None, excl_off=None, exclude_input=True, return_scores=False):
        """sbr_cluster_rank on the batch already set on the engine (`rows` rows); the lists as the C-ABI takes them"""
        self.engine._rank_local_flush("rank")
        k = _check_k(k, self.n_items)
        ids = np.empty((rows, k), dtype=np.int32)
        scores = np.empty((rows, k), dtype=np.float32) if return_scores else None
        clusters, sizes = np.empty(rows, dtype=np.int32), np.empty(rows, dtype=np.int32)
        excl_ids, excl_off = _csr_args(excl_ids, excl_off, rows)
        # (the engine's mapping of the status: SBR_EINVAL is a ValueError, as RNNEngine.rank raises it)
        self.engine._check(self.lib.sbr_cluster_rank(self.h, self.engine.h, k, int(bool(exclude_input)), _ptr(excl_ids), _ptr(excl_off),
                                                     _ptr(ids), _ptr(scores), _ptr(clusters), _ptr(sizes)))
        return (ids, scores, clusters, sizes) if return_scores else (ids, clusters, sizes)

    def evaluate(self, dataset, users, k, road, exclude_mode, want_ids=False, want_mask=True, want_whole=False):
        """Whole users of a DeviceDataset evaluated inside their item clusters on the device (sbr_cluster_evaluate), split and fed
        as by RNNEngine.evaluate.  road: CEVAL_LISTS (only the members of the user's cluster are ranked: top_k_recommendations)
        or CEVAL_PRODUCT (softmax probability times hard membership over the catalogue: the compiled test function);
        exclude_mode: EVAL_EXCL_* (LISTS: NONE, VIEWED, WINDOW; PRODUCT: NONE, WINDOW -- the items fed score 0.0).  Returns
        {"inside": rec, "whole": rec or None, "cluster": (n,) int32, "size": (n,) int32 items in the user's cluster (None on the
        PRODUCT road), "cluster_use": (C,) int32 users per cluster}; rec is RNNEngine.evaluate's dict, "whole" (want_whole) the
        whole-catalogue ranking of the same forward pass."""
        eng = self.engine
        eng._rank_local_flush("evaluate")
        users = np.ascontiguousarray(np.asarray(users, dtype=np.int32).reshape(-1))
        n, k = len(users), _check_k(k, self.n_items)
        inside = _eval_record(n, k, self.n_items, want_mask, want_ids)
        whole = _eval_record(n, k, self.n_items, want_mask, want_ids) if want_whole else None
        out = {"inside": inside, "whole": whole, "cluster": np.empty(n, np.int32),
               "size": np.empty(n, np.int32) if int(road) == CEVAL_LISTS else None, "cluster_use": np.empty(self.n_clusters, np.int32)}
        self.evaluate_calls += 1
        with self.torch.cuda.device(eng.device):
            # (the engine's mapping of the status: SBR_EINVAL is a ValueError, as RNNEngine.evaluate raises it)
            eng._check(self.lib.sbr_cluster_evaluate(self.h, eng.h, dataset.d, _ptr(users) if n else None, n, k, int(road), int(exclude_mode),
                                                     ctypes.byref(SbrEvalOut.of(whole)) if want_whole else None, ctypes.byref(SbrEvalOut.of(inside)),
                                                     _ptr(out["cluster"]), _ptr(out["size"]), _ptr(out["cluster_use"])))
        return out
