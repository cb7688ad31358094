"""ctypes binding of libclip_ops_hip.so (C ABI in include/clip_ops_hip.h).

Like the operator library there is no substitute: a CUDA tensor reaching one of these chains without the library
raises.  (CPU tensors -- the golden-vector tests -- take the element-wise torch formulation the kernels restate.)
"""
from __future__ import annotations

import ctypes

from . import _cabi

LIB_PATH = _cabi.lib_path("libclip_ops_hip.so")

ABI_VERSION = 12

c_int, c_long, c_float, c_void_p = ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_void_p

_PAIR = [c_void_p, c_void_p, c_void_p, c_long, c_long, c_void_p, c_void_p, c_void_p, c_int]
_FOCAL = [c_void_p, c_long, c_long, c_void_p, c_int, c_int, c_int, c_float, c_float]

SYMBOLS = {
    "clipops_abi_version": ([], c_int),
    "clipops_last_error": ([], ctypes.c_char_p),
    "clipops_match_cost_f32": ([c_void_p, c_long, c_long, c_void_p, c_long, c_long, c_void_p, c_void_p] + [c_int] * 4 +
                               [c_float] * 3 + [c_void_p, c_void_p], c_int),
    "clipops_pair_box_loss_fwd_f32": (_PAIR + [c_void_p, c_void_p, c_void_p], c_int),
    "clipops_pair_box_loss_bwd_f32": (_PAIR + [c_void_p, c_void_p, c_void_p, c_void_p], c_int),
    "clipops_pair_iou_f32": ([c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p], c_int),
    "clipops_track_ownership_i64": ([c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p], c_int),
    "clipops_focal_labels_i64": ([c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int,
                                  c_int, c_int, c_void_p, c_void_p], c_int),
    "clipops_focal_fwd_f32": (_FOCAL + [c_void_p, c_void_p], c_int),
    "clipops_focal_bwd_f32": (_FOCAL + [c_void_p, c_void_p, c_void_p], c_int),
    "clipops_colsum_f32": ([c_void_p, c_long, c_int, c_void_p, c_void_p], c_int),
    "clipops_colsum_partial_f32": ([c_void_p, c_long, c_int, c_int, c_void_p, c_void_p], c_int),
    "clipops_colsum_partial_bf16": ([c_void_p, c_long, c_int, c_int, c_void_p, c_void_p], c_int),
    "clipops_assign_f32": ([c_void_p, c_long, c_long, c_long, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                            c_void_p], c_int),
    "clipops_mha_fwd_f32": ([c_void_p] * 3 + [c_long] * 6 + [c_void_p] + [c_int] * 3 + [c_float, c_void_p, c_void_p,
                                                                                          c_void_p], c_int),
    "clipops_mha_bwd_f32": ([c_void_p] * 3 + [c_long] * 6 + [c_void_p] * 4 + [c_int] * 3 + [c_float] +
                            [c_void_p, c_long, c_long] * 3 + [c_void_p], c_int),
    "clipops_add_layer_norm_fwd_f32": ([c_void_p] * 4 + [c_long, c_float] + [c_void_p] * 4, c_int),
    "clipops_add_layer_norm_bwd_f32": ([c_void_p] * 4 + [c_long, c_int] + [c_void_p] * 3, c_int),
    "clipops_add_layer_norm_pos_fwd_f32": ([c_void_p] * 5 + [c_long, c_float] + [c_void_p] * 5, c_int),
    "clipops_add_layer_norm_fanin_bwd_f32": ([c_void_p] * 6 + [c_long, c_int] + [c_void_p] * 4, c_int),
    "clipops_sine_embed_fwd_f32": ([c_void_p, c_void_p, c_long, c_int, c_int, c_float, c_void_p, c_void_p], c_int),
    "clipops_sine_embed_bwd_f32": ([c_void_p, c_void_p, c_long, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p],
                                   c_int),
    "clipops_inverse_sigmoid_fwd_f32": ([c_void_p, c_long, c_float, c_void_p, c_void_p], c_int),
    "clipops_inverse_sigmoid_bwd_f32": ([c_void_p, c_void_p, c_long, c_float, c_void_p, c_void_p], c_int),
    "clipops_refine_boxes_fwd_f32": ([c_void_p, c_void_p, c_long, c_float, c_void_p, c_void_p], c_int),
    "clipops_linear_bwd_f32": ([c_void_p] * 4 + [c_int] * 3 + [c_void_p] * 4, c_int),
    "clipops_linear_fwd_f32": ([c_void_p] * 3 + [c_int] * 4 + [c_void_p, c_void_p], c_int),
    "clipops_relu_bwd_colsum_partial_f32": ([c_void_p, c_void_p, c_long, c_int, c_int, c_void_p, c_void_p, c_void_p], c_int),
    "clipops_shift_relu_f32": ([c_void_p, c_void_p, c_void_p, c_long, c_int, c_long, c_void_p], c_int),
    "clipops_shift_relu_bf16": ([c_void_p, c_void_p, c_void_p, c_long, c_int, c_long, c_void_p], c_int),
    "clipops_refine_boxes_bwd_f32": ([c_void_p, c_void_p, c_void_p, c_long, c_float, c_void_p, c_void_p, c_void_p],
                                     c_int),
    "clipops_refine_boxes_split_fwd_f32": ([c_void_p, c_void_p, c_long, c_float, c_void_p, c_void_p, c_void_p], c_int),
    "clipops_result_rows_f32": ([c_void_p] * 4 + [c_int, c_int, ctypes.c_int64] + [c_float] * 4 + [c_void_p] * 3 +
                                [c_int, c_void_p], c_int),
    "clipops_handover_fwd_f32": ([c_void_p] * 6 + [c_int] * 7 + [c_void_p] * 4, c_int),
    "clipops_handover_bwd_f32": ([c_void_p] * 4 + [c_int] * 8 + [c_void_p, c_void_p], c_int),
    "clipops_bank_update_f32": ([c_void_p, c_void_p] + [c_int] * 6 + [c_float, c_float, ctypes.c_int64, c_void_p], c_int),
    "clipops_bank_result_rows_f32": ([c_void_p] * 4 + [c_int] * 3 + [c_void_p, c_void_p, c_float, c_float] +
                                     [c_void_p] * 3 + [c_int, c_void_p], c_int),
    "clipops_bank_update_streams_f32": ([c_void_p, c_void_p] + [c_int] * 6 + [c_void_p] * 4, c_int),
    "clipops_bank_result_rows_streams_f32": ([c_void_p] * 4 + [c_int] * 3 + [c_void_p] * 7 + [c_int, c_void_p], c_int),
    "clipops_draw_table_f32": ([c_void_p] * 3 + [c_int] * 3 + [c_void_p, c_float, c_float, c_int, c_int, c_void_p,
                                                                 c_void_p], c_int),
    "clipops_clear_events_f64": ([c_void_p] * 7 + [c_int, c_void_p] + [c_int] * 3 + [c_void_p] * 6, c_int),
    "clipops_error_table_f64": ([c_void_p] * 8 + [c_int] * 6 + [c_void_p, c_void_p], c_int),
    "clipops_bdd_cross_class_f64": ([c_void_p] * 8 + [c_int] * 3 + [c_void_p] * 8, c_int),
    "clipops_hota_events_f64": ([c_void_p] * 7 + [c_int] + [c_void_p] * 4 + [c_int, c_int] + [c_void_p] * 7, c_int),
    "clipops_identity_pairs_i32": ([c_int] + [c_void_p] * 8 + [c_int] + [c_void_p] * 6, c_int),
    "clipops_assoc_reduce_f64": ([c_int] + [c_void_p] * 8 + [c_int, c_int] + [c_void_p] * 7, c_int),
    "clipops_timeline_u8": ([c_void_p] * 4 + [c_int] * 6 + [c_void_p, c_void_p], c_int),
    "clipops_fill_gaps_workspace": ([c_int] * 3, c_long),
    "clipops_fill_gaps_f32": ([c_void_p] * 3 + [c_int] * 7 + [c_void_p] * 5 + [c_int, c_void_p], c_int),
}

# status bits of clipops_fill_gaps_f32 (CLIPOPS_FG_* in include/clip_ops_hip.h)
FG_DUPLICATE, FG_ID, FG_FRAME, FG_SEQUENCE = 1, 2, 4, 8

# clipops_handover_sources / clipops_handover_grads (include/clip_ops_hip.h); the index of a source is its position here
HANDOVER_SOURCES = ("logits", "boxes", "outputs", "queries", "last_ref", "init_ref", "det_embed", "prev_ref",
                    "prev_long", "prev_last", "prev_query", "prev_iou")


class HandoverSources(ctypes.Structure):
    _fields_ = [("ptr", c_void_p * len(HANDOVER_SOURCES)), ("row_stride", c_long * len(HANDOVER_SOURCES))]


class HandoverGrads(ctypes.Structure):
    _fields_ = [("ptr", c_void_p * len(HANDOVER_SOURCES))]


# clipops_bank / clipops_bank_model (include/clip_ops_hip.h): the fields of a models/track_bank.TrackBank, in order
BANK_FIELDS = ("ids", "labels", "disappear_time", "boxes", "ref_pts", "logits", "scores", "output_embed", "long_memory",
               "last_output", "query_embed", "next_id", "counters", "free_list")
BANK_MODEL = ("pred_logits", "pred_bboxes", "outputs", "last_ref_pts", "queries")


class Bank(ctypes.Structure):
    _fields_ = [(name, c_void_p) for name in BANK_FIELDS]


class BankModel(ctypes.Structure):
    _fields_ = [("ptr", c_void_p * len(BANK_MODEL)), ("batch_stride", c_long * len(BANK_MODEL)),
                ("row_stride", c_long * len(BANK_MODEL)), ("det_embed", c_void_p), ("det_row_stride", c_long)]


lib, check = _cabi.bind("libclip_ops_hip.so", "clipops", SYMBOLS, ABI_VERSION)
