"""ctypes binding of libtrack_eval_hip.so (C ABI in include/track_eval_hip.h).

Like the other libraries there is no substitute: ``evaluation.evaluate_packed`` with a CUDA ``device`` raises without
the library.  (Without a CUDA ``device`` it is the numpy / scipy statement of the same definition that runs.)
"""
from __future__ import annotations

import ctypes

from . import _cabi

LIB_PATH = _cabi.lib_path("libtrack_eval_hip.so")

ABI_VERSION = 1
MAX_DIM = 2048          # TRACKEVAL_MAX_DIM
N_ALPHA = 19            # TRACKEVAL_N_ALPHA
CLEAR_INTS = ("CLR_TP", "CLR_FN", "CLR_FP", "IDSW", "MT", "PT", "ML", "Frag")      # TRACKEVAL_CLEAR_INTS order

c_int, c_void_p = ctypes.c_int, ctypes.c_void_p

SYMBOLS = {
    "trackeval_abi_version": ([], c_int),
    "trackeval_last_error": ([], ctypes.c_char_p),
    # gt_boxes, tr_boxes, gt_off, tr_off, sim_off | n_frames | sim | stream
    "trackeval_similarity": ([c_void_p] * 5 + [c_int] + [c_void_p] * 2, c_int),
    # sim, sim_off, gt_off, tr_off, gt_classes | n_frames, max_gt, max_tr | tr_remove, status | stream
    "trackeval_preproc_match": ([c_void_p] * 5 + [c_int] * 3 + [c_void_p] * 3, c_int),
    # sim, sim_off, gt_off, tr_off, gt_ids, tr_ids, seq_off | n_seqs | n_gt_ids, n_tr_ids, cell_off, gid_off, tid_off |
    # max_gt, max_tr | potential, id_matches, gt_count, tr_count, alignment | stream
    "trackeval_accumulate": ([c_void_p] * 7 + [c_int] + [c_void_p] * 5 + [c_int] * 2 + [c_void_p] * 6, c_int),
    # sim, sim_off, gt_off, tr_off, gt_ids, tr_ids, frame_seq | n_frames | n_tr_ids, cell_off, alignment, alphas (host) |
    # max_gt, max_tr | matches, tp, loc, status | stream
    "trackeval_hota_match": ([c_void_p] * 7 + [c_int] + [c_void_p] * 4 + [c_int] * 2 + [c_void_p] * 5, c_int),
    # seq_off | n_seqs | n_gt_ids, n_tr_ids, cell_off, gid_off, tid_off, gt_count, tr_count, matches, tp, loc |
    # out_tp, out_sums | stream
    "trackeval_hota_reduce": ([c_void_p] + [c_int] + [c_void_p] * 13, c_int),
    # sim, sim_off, gt_off, tr_off, gt_ids, tr_ids, seq_off | n_seqs | n_gt_ids | max_gt, max_tr, max_gt_ids |
    # out_ints, motp_sum, status | stream
    "trackeval_clear": ([c_void_p] * 7 + [c_int] + [c_void_p] + [c_int] * 3 + [c_void_p] * 4, c_int),
    # n_seqs | n_gt_ids, n_tr_ids, cell_off, gid_off, tid_off, gt_count, tr_count, id_matches | max_ids | out, status |
    # stream
    "trackeval_identity": ([c_int] + [c_void_p] * 8 + [c_int] + [c_void_p] * 3, c_int),
}


lib, check = _cabi.bind("libtrack_eval_hip.so", "trackeval", SYMBOLS, ABI_VERSION)
