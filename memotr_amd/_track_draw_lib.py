"""ctypes binding of libtrack_draw_hip.so (C ABI in include/track_draw_hip.h).  The kernel has no substitute: drawing
into a CUDA frame without the library raises."""
from __future__ import annotations

import ctypes

from . import _cabi

LIB_PATH = _cabi.lib_path("libtrack_draw_hip.so")

ABI_VERSION = 1
ERR_LEN = 256
ROW_WORDS = 16
MAX_GLYPHS = 10
TILE_X, TILE_Y = 64, 16     # pixels per workgroup
CHUNK = 64                  # table rows culled against a tile at a time

c_int, c_int64, c_void_p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p

SYMBOLS = {
    "trackdraw_abi_version": ([], c_int),
    "trackdraw_last_error": ([], ctypes.c_char_p),
    "trackdraw_font": ([c_void_p], None),
    # in, in_pitch, out, out_pitch, width, height, table, n, thickness, font_scale, fill_alpha, stream
    "trackdraw_draw_u8": ([c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int,
                           c_void_p], c_int),
}


lib, check = _cabi.bind("libtrack_draw_hip.so", "trackdraw", SYMBOLS, ABI_VERSION)
