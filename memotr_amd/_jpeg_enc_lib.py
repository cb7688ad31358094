"""ctypes binding of libjpeg_enc_hip.so (C ABI in include/jpeg_enc_hip.h).

The host stage (marker segments, Huffman coding) needs no device and ctypes releases the interpreter lock for the
duration of a call; the device stage has no substitute: a CUDA encode without the library raises.
"""
from __future__ import annotations

import ctypes

from . import _cabi

LIB_PATH = _cabi.lib_path("libjpeg_enc_hip.so")

ABI_VERSION = 1
ERR_LEN = 256
MAX_THREADS = 16
QT_WORDS = 192
TILE_X, TILE_Y = 64, 16     # luma pixels per workgroup of the colour launch

c_int, c_int64, c_size_t, c_void_p = ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_void_p


class Info(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ("width", "height", "ncomp", "hmax", "vmax", "restart_interval",
                                              "mcus_x", "mcus_y")] + \
               [(k, ctypes.c_int32 * 3) for k in ("h", "v", "blocks_w", "blocks_h")] + \
               [("coef_offset", ctypes.c_int64 * 3), ("coef_count", ctypes.c_int64)]


SYMBOLS = {
    "jpegenc_abi_version": ([], c_int),
    "jpegenc_last_error": ([], ctypes.c_char_p),
    # width, height, hmax, info*
    "jpegenc_geometry": ([c_int, c_int, c_int, c_void_p], c_int),
    # quality, qt_out
    "jpegenc_quant_tables": ([c_int, c_void_p], c_int),
    # coef, qt, info*, out, cap
    "jpegenc_huffman_encode": ([c_void_p, c_void_p, c_void_p, c_void_p, c_size_t], c_int64),
    # coefs, qts, info*, n_frames, outs, caps, sizes, n_threads
    "jpegenc_huffman_encode_batch": ([c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int], c_int),
    "jpegenc_planes_bytes": ([c_void_p], c_int64),
    # frame, row_pitch, frame_pitch, info*, qt, planes, planes_bytes, coef_dev, coef_pitch, B, swap_rb, stream
    "jpegenc_forward_u8": ([c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64,
                            c_int, c_int, c_void_p], c_int),
}


lib, check = _cabi.bind("libjpeg_enc_hip.so", "jpegenc", SYMBOLS, ABI_VERSION)
