"""ctypes binding of libtrack_eval_bdd_hip.so (C ABI in include/track_eval_bdd_hip.h).

Like the other libraries there is no substitute: ``evaluation_bdd100k.evaluate_packed_bdd`` with a CUDA ``device``
raises without the library.  (Without a CUDA ``device`` it is the numpy / scipy statement of the same definition that
runs.)
"""
from __future__ import annotations

import ctypes

from . import _cabi

LIB_PATH = _cabi.lib_path("libtrack_eval_bdd_hip.so")

ABI_VERSION = 1
N_CLASSES = 8           # BDDEVAL_N_CLASSES
MAX_DIM = 2048          # BDDEVAL_MAX_DIM = TRACKEVAL_MAX_DIM

c_int, c_void_p = ctypes.c_int, ctypes.c_void_p

SYMBOLS = {
    "bddeval_abi_version": ([], c_int),
    "bddeval_last_error": ([], ctypes.c_char_p),
    # gt_classes, tr_classes, gt_off, tr_off, seq_off, frame_seq | n_frames | gt_count, tr_count | stream
    "bddeval_class_count": ([c_void_p] * 6 + [c_int] + [c_void_p] * 3, c_int),
    # gt_boxes, tr_boxes, gt_ids, tr_ids, gt_classes, tr_classes, gt_off, tr_off, seq_off, frame_seq | n_frames |
    # split_gt_off, split_tr_off, out_gt_boxes, out_tr_boxes, out_gt_ids, out_tr_ids | stream
    "bddeval_class_split": ([c_void_p] * 10 + [c_int] + [c_void_p] * 7, c_int),
    # gt_boxes, tr_boxes, gt_off, tr_off, sim_off | n_frames | sim | stream
    "bddeval_similarity": ([c_void_p] * 5 + [c_int] + [c_void_p] * 2, c_int),
    # sim, sim_off, gt_off, tr_off, tr_boxes, ig_off, ig_boxes, frame_src | n_frames, max_gt, max_tr |
    # tr_remove, status | stream
    "bddeval_preproc": ([c_void_p] * 8 + [c_int] * 3 + [c_void_p] * 3, c_int),
}


lib, check = _cabi.bind("libtrack_eval_bdd_hip.so", "bddeval", SYMBOLS, ABI_VERSION)
