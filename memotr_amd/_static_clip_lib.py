"""ctypes binding of libstatic_clip_ops_hip.so (C ABI in include/static_clip_ops_hip.h).

Like the other libraries there is no substitute: a CUDA image reaching ``data.static_clip.shift_chain`` without the
library raises.  (A CPU image takes the torch integer restatement of the same definition.)
"""
from __future__ import annotations

import ctypes

from . import _cabi

LIB_PATH = _cabi.lib_path("libstatic_clip_ops_hip.so")

ABI_VERSION = 1

c_int, c_long, c_void_p = ctypes.c_int, ctypes.c_long, ctypes.c_void_p

SYMBOLS = {
    "staticclip_abi_version": ([], c_int),
    "staticclip_last_error": ([], ctypes.c_char_p),
    # h, w | strip, lds_bytes
    "staticclip_plan": ([c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int)], c_int),
    # src, row_pitch, h, w, T, flip, swap_rb | s, y0, hc | xmin, cnt, kk, ksize | out, out_row_pitch, out_frame_pitch |
    # stream
    "staticclip_shift_chain": ([c_void_p, c_long] + [c_int] * 5 + [c_int] * 3 + [c_void_p] * 3 + [c_int] +
                               [c_void_p, c_long, c_long] + [c_void_p], c_int),
}


lib, check = _cabi.bind("libstatic_clip_ops_hip.so", "staticclip", SYMBOLS, ABI_VERSION)


def launch_plan(h: int, w: int):
    """(strip, lds_bytes) the library chooses for an ``h`` x ``w`` image; ``lds_bytes == 0``: the global-memory path."""
    strip, lds = c_int(0), c_int(0)
    check(lib.staticclip_plan(int(h), int(w), ctypes.byref(strip), ctypes.byref(lds)), "staticclip_plan")
    return strip.value, lds.value
