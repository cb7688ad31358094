"""ctypes binding of libtrack_draw_hip.so (C ABI in include/track_draw_hip.h).  The kernel has no substitute: drawing
into a CUDA frame without the library raises."""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libtrack_draw_hip.so")

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
    got = lib.trackdraw_abi_version()
    if got != ABI_VERSION:
        raise ImportError(f"libtrack_draw_hip.so ABI {got} != binding ABI {ABI_VERSION}; rebuild the library")
    return lib


lib = _load()


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc}): {lib.trackdraw_last_error().decode()}")
