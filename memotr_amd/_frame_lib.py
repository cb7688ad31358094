"""ctypes binding of libframe_ops_hip.so (C ABI in include/frame_ops_hip.h).

Like the other two libraries there is no substitute: a CUDA frame reaching ``data.frames.preprocess_frames`` without
the library raises.  (CPU frames take the torch integer restatement of the same definition.)
"""
from __future__ import annotations

import ctypes

from . import _cabi

LIB_PATH = _cabi.lib_path("libframe_ops_hip.so")

ABI_VERSION = 1

c_int, c_long, c_void_p = ctypes.c_int, ctypes.c_long, ctypes.c_void_p

SYMBOLS = {
    "frameops_abi_version": ([], c_int),
    "frameops_last_error": ([], ctypes.c_char_p),
    # src, row_pitch, frame_pitch, B, h, w, s0x, s1x, a1x, s0y, s1y, b1y, th, tw, Hp, Wp, lut, swap_rb, out, stream
    "frameops_resize_normalize_u8": ([c_void_p, c_long, c_long, c_int, c_int, c_int] + [c_void_p] * 6 + [c_int] * 4 +
                                     [c_void_p, c_int, c_void_p, c_void_p], c_int),
}


lib, check = _cabi.bind("libframe_ops_hip.so", "frameops", SYMBOLS, ABI_VERSION)
