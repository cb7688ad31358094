"""ctypes binding of libtrack_motion_hip.so (C ABI in include/track_motion_hip.h).

Like the other libraries there is no substitute: ``models.motion.MotionState`` on CUDA tensors raises without the
library.  (On CPU tensors it is the torch statement of the same definition that runs.)
"""
from __future__ import annotations

import ctypes

from . import _cabi

LIB_PATH = _cabi.lib_path("libtrack_motion_hip.so")

ABI_VERSION = 1
MAX_LENGTH = 16                 # TRACKMOTION_MAX_LENGTH
STATUS_NEGATIVE_ID = 1          # TRACKMOTION_STATUS_*
STATUS_ID_PAST_CAPACITY = 2
STATUS_BAD_LABEL = 4

c_int, c_int64, c_float, c_void_p = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p

SYMBOLS = {
    "trackmotion_abi_version": ([], c_int),
    "trackmotion_last_error": ([], ctypes.c_char_p),
    # scores, labels, boxes, ids, disappear_time, last_appear_boxes | n, K | thresh, miss_tolerance |
    # table_boxes, table_count | capacity, L | ids_out, disappear_time_out, last_appear_boxes_out, status | stream
    "trackmotion_observe": ([c_void_p] * 6 + [c_int, c_int, c_float, c_int64] + [c_void_p] * 2 + [c_int, c_int]
                            + [c_void_p] * 5, c_int),
    # new_boxes | n, first_id | table_boxes, table_count | capacity, L | stream
    "trackmotion_register": ([c_void_p, c_int, c_int64, c_void_p, c_void_p, c_int, c_int, c_void_p], c_int),
    # ids, disappear_time, last_appear_boxes, ref_pts | n, motion_lambda, min_length | table_boxes, table_count |
    # capacity, L | ref_pts_out, delta_out | stream
    "trackmotion_extrapolate": ([c_void_p] * 4 + [c_int, c_float, c_int] + [c_void_p] * 2 + [c_int, c_int]
                                + [c_void_p] * 3, c_int),
}


lib, check = _cabi.bind("libtrack_motion_hip.so", "trackmotion", SYMBOLS, ABI_VERSION)
