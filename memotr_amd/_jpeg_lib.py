"""ctypes binding of libjpeg_ops_hip.so (C ABI in include/jpeg_ops_hip.h).

The host stage (header parsing, Huffman decoding) needs no device and ctypes releases the interpreter lock for the
duration of a call; the device stage has no substitute: a CUDA decode without the library raises.
"""
from __future__ import annotations

import ctypes

from . import _cabi

LIB_PATH = _cabi.lib_path("libjpeg_ops_hip.so")

ABI_VERSION = 1
UNSUPPORTED = 16            # status codes from here on: a valid stream of a kind the decoder does not read
ERR_LEN = 256
MAX_THREADS = 16
QT_WORDS = 192
TILE_X, TILE_Y = 64, 16     # output pixels per workgroup of the colour launch

c_int, c_int64, c_size_t, c_void_p = ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_void_p


class Info(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ("width", "height", "ncomp", "hmax", "vmax", "restart_interval",
                                              "mcus_x", "mcus_y")] + \
               [(k, ctypes.c_int32 * 3) for k in ("h", "v", "blocks_w", "blocks_h")] + \
               [("coef_offset", ctypes.c_int64 * 3), ("coef_count", ctypes.c_int64)]


SYMBOLS = {
    "jpegops_abi_version": ([], c_int),
    "jpegops_last_error": ([], ctypes.c_char_p),
    # bytes, n, info*
    "jpegops_parse_header": ([c_void_p, c_size_t, c_void_p], c_int),
    # bytes, n, info*, coef_out, coef_bytes, qt_out
    "jpegops_entropy_decode": ([c_void_p, c_size_t, c_void_p, c_void_p, c_size_t, c_void_p], c_int),
    # streams, sizes, n_frames, infos, coef_outs, coef_bytes, qt_outs, status, errors, n_threads
    "jpegops_entropy_decode_batch": ([c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_int], c_int),
    "jpegops_planes_bytes": ([c_void_p], c_int64),
    # coef_dev, coef_pitch, qt_dev, qt_pitch, info*, planes, planes_bytes, out, row_pitch, frame_pitch, B, swap_rb, stream
    "jpegops_decode_pixels_u8": ([c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64,
                                  c_int64, c_int, c_int, c_void_p], c_int),
}


lib, check = _cabi.bind("libjpeg_ops_hip.so", "jpegops", SYMBOLS, ABI_VERSION)
