"""ctypes binding of libopt_ops_hip.so (C ABI in include/opt_ops_hip.h).

Like the other libraries there is no substitute: ``optim.ClipAdamW`` on CUDA parameters raises without the library.
(On CPU parameters it is the torch statement of the same definition that runs.)
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _cabi

LIB_PATH = _cabi.lib_path("libopt_ops_hip.so")

ABI_VERSION = 1
CHUNK = 16384                   # OPTSTEP_CHUNK
MAX_GROUPS = 8                  # OPTSTEP_MAX_GROUPS
MAX_CHUNKS = 1 << 20            # OPTSTEP_MAX_CHUNKS

# optstep_tensor / optstep_chunk as numpy record types: the tables are assembled on the host in these layouts
TENSOR_DTYPE = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("numel", "<i8"), ("group", "<i4"),
                         ("reserved", "<i4")])
CHUNK_DTYPE = np.dtype([("tensor", "<i4"), ("index", "<i4")])
assert TENSOR_DTYPE.itemsize == 48 and CHUNK_DTYPE.itemsize == 8


class Group(ctypes.Structure):          # optstep_group
    _fields_ = [(n, ctypes.c_double) for n in ("lr", "weight_decay", "beta1", "beta2", "eps")]


class Hyper(ctypes.Structure):          # optstep_hyper
    _fields_ = [("group", Group * MAX_GROUPS)]


c_int, c_double, c_void_p = ctypes.c_int, ctypes.c_double, ctypes.c_void_p

SYMBOLS = {
    "optstep_abi_version": ([], c_int),
    "optstep_last_error": ([], ctypes.c_char_p),
    # tensors, chunks | n_tensors, n_chunks | partials, steps, steps_prev | stream
    "optstep_sumsq": ([c_void_p] * 2 + [c_int] * 2 + [c_void_p] * 4, c_int),
    # tensors, chunks | n_tensors, n_chunks | partials, steps, steps_prev | hyper | n_groups, max_norm |
    # total_norm_out | stream
    "optstep_adamw": ([c_void_p] * 2 + [c_int] * 2 + [c_void_p] * 3 + [ctypes.POINTER(Hyper), c_int, c_double]
                      + [c_void_p] * 2, c_int),
}


lib, check = _cabi.bind("libopt_ops_hip.so", "optstep", SYMBOLS, ABI_VERSION)
