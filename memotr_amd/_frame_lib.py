"""ctypes binding of libframe_ops_hip.so (C ABI in include/frame_ops_hip.h).

Like the other two libraries there is no substitute: a CUDA frame reaching ``data.frames.preprocess_frames`` without
the library raises.  (CPU frames take the torch integer restatement of the same definition.)
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libframe_ops_hip.so")

ABI_VERSION = 1

c_int, c_long, c_void_p = ctypes.c_int, ctypes.c_long, ctypes.c_void_p

SYMBOLS = {
    "frameops_abi_version": ([], c_int),
    "frameops_last_error": ([], ctypes.c_char_p),
    # src, row_pitch, frame_pitch, B, h, w, s0x, s1x, a1x, s0y, s1y, b1y, th, tw, Hp, Wp, lut, swap_rb, out, stream
    "frameops_resize_normalize_u8": ([c_void_p, c_long, c_long, c_int, c_int, c_int] + [c_void_p] * 6 + [c_int] * 4 +
                                     [c_void_p, c_int, c_void_p, c_void_p], c_int),
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
    got = lib.frameops_abi_version()
    if got != ABI_VERSION:
        raise ImportError(f"libframe_ops_hip.so ABI {got} != binding ABI {ABI_VERSION}; rebuild the library")
    return lib


lib = _load()


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc}): {lib.frameops_last_error().decode()}")
