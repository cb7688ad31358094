"""ctypes binding of libstatic_clip_ops_hip.so (C ABI in include/static_clip_ops_hip.h).

Like the other libraries there is no substitute: a CUDA image reaching ``data.static_clip.shift_chain`` without the
library raises.  (A CPU image takes the torch integer restatement of the same definition.)
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libstatic_clip_ops_hip.so")

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
    got = lib.staticclip_abi_version()
    if got != ABI_VERSION:
        raise ImportError(f"libstatic_clip_ops_hip.so ABI {got} != binding ABI {ABI_VERSION}; rebuild the library")
    return lib


lib = _load()


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc}): {lib.staticclip_last_error().decode()}")


def launch_plan(h: int, w: int):
    """(strip, lds_bytes) the library chooses for an ``h`` x ``w`` image; ``lds_bytes == 0``: the global-memory path."""
    strip, lds = c_int(0), c_int(0)
    check(lib.staticclip_plan(int(h), int(w), ctypes.byref(strip), ctypes.byref(lds)), "staticclip_plan")
    return strip.value, lds.value
