"""ctypes binding of libaugment_ops_hip.so (C ABI in include/augment_ops_hip.h).

Like the other libraries there is no substitute: CUDA frames reaching ``data.augment.augment_clip`` without the
library raise.  (CPU frames take the torch integer restatement of the same definition.)
"""
from __future__ import annotations

import ctypes

from . import _cabi

LIB_PATH = _cabi.lib_path("libaugment_ops_hip.so")

ABI_VERSION = 1
STAGE_U8, STAGE_F32 = 0, 1

c_int, c_long, c_void_p = ctypes.c_int, ctypes.c_long, ctypes.c_void_p

SYMBOLS = {
    "augops_abi_version": ([], c_int),
    "augops_last_error": ([], ctypes.c_char_p),
    # src, row_pitch, frame_pitch, T, h, w, flip, swap_rb | xmin_x, cnt_x, kk_x, ksize_x | xmin_y, cnt_y, kk_y, ksize_y |
    # oh, ow, stage | out_u8, out_row_pitch, out_frame_pitch | out_f32, Hp, Wp, lut, hsv_div, use_hsv, dh, ds, dv,
    # reverse | stream
    "augops_resample_u8": ([c_void_p, c_long, c_long] + [c_int] * 5 + ([c_void_p] * 3 + [c_int]) * 2 + [c_int] * 3 +
                           [c_void_p, c_long, c_long] + [c_void_p, c_int, c_int, c_void_p, c_void_p] + [c_int] * 5 +
                           [c_void_p], c_int),
}


lib, check = _cabi.bind("libaugment_ops_hip.so", "augops", SYMBOLS, ABI_VERSION)
