"""ctypes binding of libtrack_motion_hip.so (C ABI in include/track_motion_hip.h).

Like the other libraries there is no substitute: ``models.motion.MotionState`` on CUDA tensors raises without the
library.  (On CPU tensors it is the torch statement of the same definition that runs.)
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libtrack_motion_hip.so")

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


def _load() -> ctypes.CDLL:
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -m memotr_amd.build` "
                          "(hipcc --offload-arch=gfx950).")
    import torch  # noqa: F401  (binds the HIP runtime torch's streams live in; see _lib.py)

    lib = ctypes.CDLL(LIB_PATH)
    for name, (argtypes, restype) in SYMBOLS.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = restype
    got = lib.trackmotion_abi_version()
    if got != ABI_VERSION:
        raise ImportError(f"libtrack_motion_hip.so ABI {got} != binding ABI {ABI_VERSION}; rebuild the library")
    return lib


lib = _load()


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc}): {lib.trackmotion_last_error().decode()}")
