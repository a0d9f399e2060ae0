"""ctypes binding of the C ABI in ``include/hgnn_hip.h`` (libhgnn_hip.so).

The library is built in-tree by ``hierarchicalgnn_amd.build`` (hipcc,
``--offload-arch=gfx950``).  There is deliberately NO fallback: if the shared
object is missing, or a call returns a non-zero status, a ``RuntimeError`` is
raised.  PyTorch is only used for device memory and the stream handle.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, Structure, byref, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# HGNN_LIB: A/B measurements of two builds of the SAME sources with different tuning constants (tools/); never a fallback
LIB_PATH = os.environ.get("HGNN_LIB") or os.path.join(_HERE, "csrc", "libhgnn_hip.so")

HGNN_OK = 0
CNT_WORK, CNT_SPLIT, CNT_PARTIAL, CNT_ERR, CNT_VALID, CNT_UNSORTED = 0, 1, 2, 3, 4, 5
ABI_VERSION = 26
MLP_BWD_BLOCKS = 512   # HGNN_MLP_BWD_BLOCKS
MLP_BWD_TILE_ROWS_N1024 = 32   # HGNN_MLP_BWD_TILE_ROWS_N1024: rows per tile of the N = 1024 backward layer
GMM_STATE, GMM_BLOCKS = 16, 1024   # HGNN_GMM_STATE, HGNN_GMM_BLOCKS
LN_ACT_BLOCKS = 1024   # HGNN_LN_ACT_BLOCKS
MLP_BWD_F32_BLOCKS = 512   # HGNN_MLP_BWD_F32_BLOCKS: grid of the fp32 backward layer (device independent)
RED_SUM, RED_MIN, RED_MAX = 0, 1, 2   # HGNN_RED_*
DT_F32, DT_BF16, DT_I32, DT_I64, DT_F64 = 0, 1, 2, 3, 4   # HGNN_DT_*
# HGNN_TE_*: entries of hgnn_track_eval's result vector
(TE_TRACK_EFF, TE_TRACK_PUR, TE_HIT_EFF, TE_HIT_PUR, TE_N_KEPT, TE_N_MASK, TE_N_TRUTH, TE_N_CAND, TE_N_PART,
 TE_NO_MATCH, TE_STATUS, TE_N_MATCH, TE_RESULT) = range(13)
# HGNN_TR_*: hgnn_track_records' limits and histogram columns
TR_MAX_VARS, TR_MAX_BINS, TR_COLUMNS = 4, 64, 6
# HGNN_TS_*: hgnn_track_scan's modes, limit, the three item counts after the HGNN_TE_* entries of a row, and the
# reserved candidate label
TS_EDGE, TS_PAIR = 0, 1
TS_MAX_CUTS = 64
TS_N_PASS, TS_N_TRUE_PASS, TS_N_TRUE, TS_ROW = 12, 13, 14, 15
TS_RESERVED_LABEL = 2 ** 63 - 1

# HGNN_AM_*: hgnn_assign_match's constants, status bits and the entries of its info vector
AM_SCALE_BITS, AM_FALLBACK_WEIGHT = 30, 1e-12
AM_ST_BAD_ID, AM_ST_BAD_WEIGHT, AM_ST_OVERFLOW, AM_ST_BUDGET = 1, 2, 4, 8
AM_N_PAIRS, AM_STATUS, AM_PHASES, AM_GRID_ROUNDS, AM_TAIL_ROUNDS, AM_HOST_READS = range(6)
AM_INFO = 8
# HGNN_HDB_*: entries of hgnn_hdbscan_f32's info vector; HGNN_HDBSCAN_LAMBDA_DUP
(HDB_ROUNDS, HDB_HOST_READS, HDB_N_CLUSTERS, HDB_STAGE_SYNC, HDB_T_CORE_NS, HDB_T_SORT_NS, HDB_T_TREE_NS) = range(7)
HDB_T_ROUND0_NS, HDB_INFO = 8, 32
HDBSCAN_LAMBDA_DUP = 2.0 ** 100
# HGNN_PH_*: hgnn_pair_hinge_*'s host hparams vector and device state vector
PH_MAX_DIM = 16
(PH_WEIGHT_MIN, PH_WEIGHT_LEAK, PH_PTCUT, PH_PT_INTERVAL, PH_LOG_WEIGHT_RATIO, PH_MARGIN, PH_SCALE) = range(7)
PH_HPARAMS = 8
PH_KT, PH_KF, PH_ST, PH_SF, PH_LOSS = range(5)
PH_STATE = 8
# HGNN_WB_*: hgnn_weighted_bce_*'s combine modes, status bits and device state vector (hparams: PH_* entries 0-4)
WB_COMBINE_SUM, WB_COMBINE_MAX = 0, 1
WB_ST_BAD_ID, WB_ST_BAD_SCORE = 1, 2
WB_KT, WB_KF, WB_ST, WB_SF, WB_LOSS = range(5)
WB_STATE = 8
# HGNN_OPT_*: hgnn_optim_*'s chunk size, flag bits, status bit and device state vector
OPT_CHUNK = 4096
OPT_AMSGRAD, OPT_CLIP, OPT_ZERO_GRADS, OPT_WRITE_GRADS, OPT_SCALAR = 1, 2, 4, 8, 16
OPT_ST_NONFINITE = 1
OPT_NORM, OPT_COEF, OPT_SUMSQ = range(3)
OPT_STATE = 4
# HGNN_GC_* / HGNN_GA_*: hgnn_knn_edges' status bit; hgnn_graph_attention_*'s limits, function codes, flag bits and
# device state vector
GC_ST_BAD_ID = 1
GA_MAX_DIM = 16
GA_FN_SIGMOID, GA_FN_EXP = 0, 1
GA_TRAINING, GA_NORM = 1, 2
GA_MEAN, GA_VAR, GA_RSTD, GA_SUMF, GA_E, GA_DBETA, GA_DGAMMA, GA_SGF = range(8)
GA_STATE = 8
# HGNN_EP_*: hgnn_event_*'s status bit, flag bits and device info vector
EP_ST_BAD_ID = 1
EP_NOISE, EP_REMOVE_ISOLATED, EP_USE_PRIMARY = 1, 2, 4
EP_N_NODES, EP_E_EDGE_INDEX, EP_E_MODULEWISE, EP_E_SIGNAL, EP_STATUS = range(5)
EP_INFO = 8
# HGNN_TP_*: hgnn_training_pairs_*'s limit, modes, status bits and device info vector
TP_MAX_K = 128
TP_MODE_MODULEWISE, TP_MODE_PID = 0, 1
TP_ST_BAD_IDX, TP_ST_BAD_MTE = 1, 2
TP_P, TP_N_ROW, TP_N_TRUTH, TP_STATUS = range(4)
TP_INFO = 4

class HgnnPlan(Structure):
    """mirror of ``struct hgnn_plan``"""
    _fields_ = [
        ("n_rows", c_int64), ("n_dst", c_int64), ("n_src", c_int64),
        ("chunk", c_int32), ("has_gather", c_int32),
        ("max_work", c_int64), ("max_split", c_int64), ("max_partial", c_int64),
        ("perm", c_void_p), ("src_row", c_void_p), ("dst32", c_void_p), ("rowptr", c_void_p),
        ("wi_begin", c_void_p), ("wi_end", c_void_p), ("wi_target", c_void_p), ("wi_dst", c_void_p),
        ("split_dst", c_void_p), ("split_pbegin", c_void_p), ("counts", c_void_p),
    ]


class HgnnMlpDesc(Structure):
    """mirror of ``struct hgnn_mlp_desc``"""
    _fields_ = [
        ("n_seg", c_int32),
        ("seg_table", c_void_p * 3), ("seg_index", c_void_p * 3), ("seg_width", c_int32 * 3),
        ("n_layers", c_int32),
        ("W", c_void_p * 3), ("b", c_void_p * 3), ("ln_w", c_void_p * 3), ("ln_b", c_void_p * 3),
        ("width", c_int32 * 4), ("act", c_int32 * 3),
        ("ln_eps", c_float),
        ("skip", c_void_p),
        ("M", c_int64),
        ("w0_cols", c_int32),
        ("w_last_rows", c_int32),
        ("save_pre", c_void_p * 3),
        ("n_pre", c_int32),
        ("pre_table", c_void_p * 2), ("pre_index", c_void_p * 2),
    ]


class HgnnOptEntry(Structure):
    """mirror of ``struct hgnn_opt_entry``"""
    _fields_ = [
        ("p", c_void_p), ("g", c_void_p), ("offset", c_int64), ("numel", c_int64), ("first_chunk", c_int64),
        ("decay", c_float), ("step_size", c_float), ("inv_sqrt_bc2", c_float), ("one_minus_b1", c_float),
        ("b2", c_float), ("one_minus_b2", c_float), ("eps", c_float), ("reserved", c_int32),
    ]


class HgnnTrParticles(Structure):
    """mirror of ``struct hgnn_tr_particles``"""
    _fields_ = [(k, c_void_p) for k in ("pid", "nhits", "pt", "primary", "reconstructable", "n_match", "n_kept",
                                        "n_mask", "cand_index", "shared", "values")]


class HgnnTrCandidates(Structure):
    """mirror of ``struct hgnn_tr_candidates``"""
    _fields_ = [(k, c_void_p) for k in ("label", "size", "n_kept", "n_mask", "particle", "shared")]


_SIGNATURES = {
    "hgnn_abi_version": (c_int, []),
    "hgnn_last_error": (c_char_p, []),
    "hgnn_set_option": (c_int, [c_char_p, c_int]),
    "hgnn_get_option": (c_int, [c_char_p, POINTER(c_int)]),
    "hgnn_sizeof_plan": (c_int, []),
    "hgnn_sizeof_mlp_desc": (c_int, []),
    "hgnn_plan_dims": (c_int, [c_int64, c_int64, c_int64, c_int32, POINTER(HgnnPlan)]),
    "hgnn_plan_workspace_bytes": (c_int, [c_int64, c_int64, POINTER(c_size_t)]),
    "hgnn_plan_build": (c_int, [c_void_p, c_void_p, POINTER(HgnnPlan), c_void_p, c_size_t, c_void_p]),
    "hgnn_segment_reduce_f32": (c_int, [POINTER(HgnnPlan), c_void_p, c_int32, c_void_p, c_void_p,
                                        c_void_p, c_void_p, c_void_p]),
    "hgnn_segment_reduce_f32_ex": (c_int, [POINTER(HgnnPlan), c_void_p, c_int32, c_void_p, c_void_p,
                                           c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "hgnn_plan_item_order_workspace_bytes": (c_int, [POINTER(HgnnPlan), POINTER(c_size_t)]),
    "hgnn_plan_item_order": (c_int, [POINTER(HgnnPlan), c_void_p, c_void_p, c_size_t, c_void_p]),
    "hgnn_segment_reduce_ex": (c_int, [POINTER(HgnnPlan), c_int32, c_int32, c_void_p, c_int32, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_void_p]),
    "hgnn_segment_arg_backward": (c_int, [c_void_p, c_int64, c_int32, c_int64, c_int32, c_void_p, c_void_p, c_void_p]),
    "hgnn_gather_rows_f32": (c_int, [c_void_p, c_int64, c_int32, c_void_p, c_int64, c_void_p, c_void_p,
                                     c_void_p, c_void_p]),
    "hgnn_spread_rows_f32": (c_int, [POINTER(HgnnPlan), c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "hgnn_segment_reduce_bf16": (c_int, [POINTER(HgnnPlan), c_void_p, c_int32, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p]),
    "hgnn_spread_rows_bf16": (c_int, [POINTER(HgnnPlan), c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "hgnn_gather_rows_bf16": (c_int, [c_void_p, c_int64, c_int32, c_void_p, c_int64, c_void_p, c_void_p,
                                      c_void_p]),
    "hgnn_edge_dot_f32": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int32,
                                  c_int64, c_void_p, c_void_p]),
    "hgnn_index_to_i32": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "hgnn_knn_radius_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int32, c_int32, c_float, c_void_p,
                                    c_void_p, c_void_p]),
    "hgnn_knn_workspace_bytes": (c_int, [c_int64, c_int64, c_int32, POINTER(c_size_t)]),
    "hgnn_knn_radius_ws_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int32, c_int32, c_float, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "hgnn_knn_sorted_workspace_bytes": (c_int, [c_int64, c_int64, c_int32, c_int32, POINTER(c_size_t)]),
    "hgnn_knn_radius_sorted_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int32, c_int32, c_float, c_void_p,
                                           c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    "hgnn_gmm2_fit_f32": (c_int, [c_void_p, c_int64, c_int32, c_float, c_float, c_void_p, c_void_p, c_void_p,
                                  c_void_p]),
    "hgnn_gmm2_cut_f32": (c_int, [c_void_p, c_float, c_int32, c_float, c_void_p, c_void_p]),
    "hgnn_cc_labels": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_void_p]),
    "hgnn_ln_act_forward_bf16": (c_int, [c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_int32, c_float,
                                         c_void_p, c_void_p]),
    "hgnn_ln_act_backward_bf16": (c_int, [c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_int32,
                                          c_float, c_void_p, c_void_p, c_void_p]),
    "hgnn_wgrad_workspace_bytes": (c_int, [c_int64, c_int32, c_int32, POINTER(c_size_t)]),
    "hgnn_wgrad_bf16": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int32, c_int32, c_void_p, c_int64,
                                c_void_p, c_void_p, c_size_t, c_void_p]),
    "hgnn_wgrad_f32_split3": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int32, c_int32, c_void_p, c_int64,
                                c_void_p, c_void_p, c_size_t, c_void_p]),
    "hgnn_wgrad_f32_workspace_bytes": (c_int, [c_int64, c_int32, c_int32, POINTER(c_size_t)]),
    "hgnn_wgrad_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int32, c_int32, c_void_p, c_int64,
                               c_void_p, c_size_t, c_void_p]),
    "hgnn_project_f32": (c_int, [c_void_p, c_int64, c_int64, c_int32, c_void_p, c_void_p, c_int64, c_int32, c_void_p,
                                 c_void_p, c_int64, c_void_p]),
    "hgnn_linear_narrow_f32": (c_int, [c_void_p, c_int64, c_int64, c_int32, c_void_p, c_int64, c_void_p, c_int32,
                                       c_void_p, c_int64, c_void_p]),
    "hgnn_outer_narrow_f32": (c_int, [c_void_p, c_int64, c_int64, c_int32, c_void_p, c_int64, c_int32, c_void_p,
                                      c_void_p, c_int64, c_void_p]),
    "hgnn_wgrad_narrow_f32_workspace_bytes": (c_int, [c_int64, c_int32, c_int32, POINTER(c_size_t)]),
    "hgnn_wgrad_narrow_f32": (c_int, [c_void_p, c_int64, c_int32, c_void_p, c_int64, c_int32, c_int64, c_void_p, c_int64,
                                      c_void_p, c_void_p, c_size_t, c_void_p]),
    "hgnn_mlp_backward_layer_supported_bf16": (c_int, [c_int32, c_int32]),
    "hgnn_mlp_backward_layer_bf16": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                             c_int32, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "hgnn_mlp_backward_layer_supported_f32": (c_int, [c_int32, c_int32]),
    "hgnn_mlp_backward_layer_f32": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_int32, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "hgnn_mlp_supported": (c_int, [POINTER(HgnnMlpDesc)]),
    "hgnn_mlp_forward_f32": (c_int, [POINTER(HgnnMlpDesc), c_void_p, c_void_p]),
    "hgnn_mlp_supported_f32_padded": (c_int, [POINTER(HgnnMlpDesc)]),
    "hgnn_mlp_forward_f32_padded": (c_int, [POINTER(HgnnMlpDesc), c_void_p, c_void_p]),
    "hgnn_mlp_supported_f32_plain": (c_int, [POINTER(HgnnMlpDesc)]),
    "hgnn_mlp_forward_f32_plain": (c_int, [POINTER(HgnnMlpDesc), c_void_p, c_void_p]),
    "hgnn_mlp_supported_f32_square": (c_int, [POINTER(HgnnMlpDesc)]),
    "hgnn_mlp_forward_f32_square": (c_int, [POINTER(HgnnMlpDesc), c_void_p, c_void_p]),
    "hgnn_act_rows_forward_f32": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p]),
    "hgnn_act_rows_backward_f32": (c_int, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p,
                                           c_void_p]),
    "hgnn_mlp_supported_bf16": (c_int, [POINTER(HgnnMlpDesc)]),
    "hgnn_mlp_forward_bf16": (c_int, [POINTER(HgnnMlpDesc), c_void_p, c_void_p]),
    "hgnn_mlp_supported_bf16_split": (c_int, [POINTER(HgnnMlpDesc)]),
    "hgnn_mlp_forward_bf16_split": (c_int, [POINTER(HgnnMlpDesc), c_void_p, c_void_p]),
    "hgnn_mlp_supported_f32_split3": (c_int, [POINTER(HgnnMlpDesc)]),
    "hgnn_mlp_forward_f32_split3": (c_int, [POINTER(HgnnMlpDesc), c_void_p, c_void_p]),
    "hgnn_mlp_supported_f32_split3_padded": (c_int, [POINTER(HgnnMlpDesc)]),
    "hgnn_mlp_forward_f32_split3_padded": (c_int, [POINTER(HgnnMlpDesc), c_void_p, c_void_p]),
    "hgnn_linear_f32_split3": (c_int, [c_void_p, c_int64, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "hgnn_project_f32_split3": (c_int, [c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p,
                                        c_void_p]),
    "hgnn_ln_act_forward_f32": (c_int, [c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_int32, c_float,
                                        c_void_p, c_void_p]),
    "hgnn_ln_act_backward_f32": (c_int, [c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_int32,
                                         c_float, c_void_p, c_void_p, c_void_p]),
    "hgnn_track_eval_workspace_bytes": (c_int, [c_int64, c_int64, POINTER(c_size_t)]),
    "hgnn_track_eval": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_double,
                                c_double, c_double, c_void_p, c_void_p, c_size_t, c_void_p]),
    "hgnn_track_records_workspace_bytes": (c_int, [c_int64, c_int64, c_int32, POINTER(c_size_t)]),
    "hgnn_track_records": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p,
                                   c_int32, POINTER(c_float), POINTER(c_int32), c_double, c_double, c_double,
                                   c_void_p, POINTER(HgnnTrParticles), POINTER(HgnnTrCandidates), c_void_p, c_void_p,
                                   c_size_t, c_void_p]),
    "hgnn_track_scan_workspace_bytes": (c_int, [c_int32, c_int64, c_int64, c_int64, c_int32, POINTER(c_size_t)]),
    "hgnn_track_scan": (c_int, [c_int32, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_void_p, c_int64,
                                c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_double, c_double,
                                c_double, c_void_p, c_void_p, c_size_t, c_void_p]),
    "hgnn_graph_intersection_workspace_bytes": (c_int, [c_int64, c_int64, c_int32, POINTER(c_size_t)]),
    "hgnn_graph_intersection": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int32, c_void_p, c_void_p,
                                        c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "hgnn_assign_match_workspace_bytes": (c_int, [c_int64, c_int64, c_int64, POINTER(c_size_t)]),
    "hgnn_assign_match": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p,
                                  c_void_p, c_void_p, POINTER(c_int64), c_void_p, c_size_t, c_void_p]),
    "hgnn_hdbscan_workspace_bytes": (c_int, [c_int64, c_int32, c_int32, c_int32, POINTER(c_size_t)]),
    "hgnn_hdbscan_f32": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                 POINTER(c_int64), c_void_p, c_size_t, c_void_p]),
    "hgnn_hdbscan_tree_host": (c_int, [c_void_p, c_void_p, c_int64, c_int32, c_void_p, POINTER(c_int64)]),
    "hgnn_pair_hinge_workspace_bytes": (c_int, [c_int64, c_int64, c_int32, c_int32, POINTER(c_size_t)]),
    "hgnn_pair_hinge_forward": (c_int, [c_void_p, c_int64, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_int64,
                                        POINTER(c_double), c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                        c_void_p]),
    "hgnn_pair_hinge_backward": (c_int, [POINTER(HgnnPlan), c_void_p, c_int64, c_int32, c_void_p, c_int32, c_void_p,
                                         c_void_p, c_int64, POINTER(c_double), c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_size_t, c_void_p]),
    "hgnn_weighted_bce_workspace_bytes": (c_int, [c_int64, c_int32, POINTER(c_size_t)]),
    "hgnn_weighted_bce_forward": (c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int64, c_void_p,
                                          c_int64, c_int64, c_int32, POINTER(c_double), c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_size_t, c_void_p]),
    "hgnn_weighted_bce_backward": (c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int64, c_void_p,
                                           c_int64, c_int64, c_int32, POINTER(c_double), c_void_p, c_void_p, c_void_p,
                                           c_void_p]),
    "hgnn_sizeof_opt_entry": (c_int, []),
    "hgnn_optim_workspace_bytes": (c_int, [c_int64, POINTER(c_size_t)]),
    "hgnn_optim_grad_norm": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_double, c_int32, c_void_p, c_void_p,
                                     c_void_p, c_size_t, c_void_p]),
    "hgnn_optim_adamw_step": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int64,
                                      c_int32, c_void_p, c_void_p]),
    "hgnn_knn_edges_workspace_bytes": (c_int, [c_int64, c_int32, c_int64, c_int32, POINTER(c_size_t)]),
    "hgnn_knn_edges": (c_int, [c_void_p, c_int64, c_int32, c_int64, c_int32, c_void_p, c_int64, c_void_p, c_void_p,
                               c_size_t, c_void_p]),
    "hgnn_graph_attention_workspace_bytes": (c_int, [c_int64, c_int32, POINTER(c_size_t)]),
    "hgnn_graph_attention_forward": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int32, c_void_p, c_int32, c_int64,
                                             c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_double,
                                             c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                             c_size_t, c_void_p]),
    "hgnn_graph_attention_backward": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_int32, c_void_p,
                                              c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "hgnn_event_hit_counts_workspace_bytes": (c_int, [c_int64, POINTER(c_size_t)]),
    "hgnn_event_hit_counts": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_size_t,
                                      c_void_p]),
    "hgnn_event_nodes_workspace_bytes": (c_int, [c_int64, c_int64, POINTER(c_size_t)]),
    "hgnn_event_nodes": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_double, c_int64, c_int32,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "hgnn_event_inverse_mask": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p]),
    "hgnn_event_edges_workspace_bytes": (c_int, [c_int64, POINTER(c_size_t)]),
    "hgnn_event_edges_count": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                       c_size_t, c_void_p]),
    "hgnn_event_edges_fill": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                      c_int64, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "hgnn_event_gather_rows": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_int64, c_void_p, c_void_p]),
    "hgnn_training_pairs_workspace_bytes": (c_int, [c_int64, c_int32, c_int64, c_int32, POINTER(c_size_t)]),
    "hgnn_training_pairs_count": (c_int, [c_void_p, c_int64, c_int32, c_void_p, c_int64, c_void_p, c_void_p, c_int32,
                                          c_void_p, c_void_p, c_size_t, c_void_p]),
    "hgnn_training_pairs_fill": (c_int, [c_void_p, c_int64, c_int32, c_void_p, c_int64, c_void_p, c_void_p, c_int32,
                                         c_void_p, c_void_p, c_int64, c_void_p, c_size_t, c_void_p]),
}

_lib = None


def load() -> ctypes.CDLL:
    """Load libhgnn_hip.so (once).  Raises RuntimeError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"hierarchicalgnn_amd: {LIB_PATH} is missing. Build it with "
            "`python -m hierarchicalgnn_amd.build` (needs hipcc; gfx950). "
            "There is no CPU / eager fallback for the HIP kernels.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so is stale
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def declared_symbols():
    """names the binding expects (kept in sync with include/hgnn_hip.h by a test)"""
    return sorted(_SIGNATURES)


def register(name, restype, argtypes):
    _SIGNATURES[name] = (restype, argtypes)
    if _lib is not None:
        fn = getattr(_lib, name)
        fn.restype = restype
        fn.argtypes = argtypes


def check(rc: int, what: str = "") -> None:
    if rc != HGNN_OK:
        msg = load().hgnn_last_error()
        raise RuntimeError(f"libhgnn_hip {what} failed (status {rc}): {msg.decode() if msg else ''}")


def get_option(name: str) -> int:
    v = c_int(0)
    check(load().hgnn_get_option(name.encode(), byref(v)), "hgnn_get_option")
    return v.value


def ptr(t):
    """device pointer of a tensor (or NULL)"""
    return c_void_p(t.data_ptr()) if t is not None and t.numel() > 0 else c_void_p(0)


def current_stream(device):
    import torch
    return c_void_p(torch.cuda.current_stream(device).cuda_stream)


def workspace(symbol: str, device, *args):
    """(uint8 scratch tensor on ``device``, its size in bytes as the library counts it) for the size query ``symbol``
    called with ``args`` and the byte count's address.  The tensor has at least one byte, so its pointer is never NULL."""
    import torch
    nb = c_size_t(0)
    check(getattr(load(), symbol)(*args, byref(nb)), symbol)
    return torch.empty(max(int(nb.value), 1), dtype=torch.uint8, device=device), int(nb.value)


def index_dtype(t) -> int:
    """HGNN_DT_* of an int64 or int32 index tensor"""
    import torch
    return DT_I64 if t.dtype == torch.int64 else DT_I32


def pt_scalars(hparams):
    """the host hparams vector of the pT-weighted losses with the five PH_* entries they share filled in"""
    h = (c_double * PH_HPARAMS)()
    h[PH_WEIGHT_MIN] = float(hparams["weight_min"])
    h[PH_WEIGHT_LEAK] = float(hparams["weight_leak"])
    h[PH_PTCUT] = float(hparams["ptcut"])
    h[PH_PT_INTERVAL] = float(hparams["pt_interval"])
    h[PH_LOG_WEIGHT_RATIO] = float(hparams["log_weight_ratio"])
    return h


class PendingStatus:
    """The status words of the calls nobody has read yet: device -> int32[1], OR-ed on the device, so a call makes no
    host read.  ``stats``: the owning module's counters; ``stats["host_reads"]`` counts one per device word read."""

    def __init__(self, stats):
        self.stats = stats
        self.words = {}

    def add(self, device, status):
        word = self.words.get(device)
        self.words[device] = status if word is None else word | status

    def take(self, device=None) -> int:
        """reads and clears the word of ``device`` (None: of every device); 0 if nothing is pending"""
        import torch
        if device is None:
            devs = list(self.words)
        else:
            dev = torch.device(device)
            devs = [dev if dev.index is not None else torch.device(dev.type, torch.cuda.current_device())]
        out = 0
        for dev in devs:
            word = self.words.pop(dev, None)
            if word is not None:
                self.stats["host_reads"] += 1
                out |= int(word.item())
        return out
