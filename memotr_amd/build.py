"""Build the package's HIP libraries into memotr_amd/lib/ with hipcc for gfx950 (cross-compiles without a GPU).

One row of ``LIBS`` per library; ``python -m memotr_amd.build`` rebuilds all of them:

    msda            libmsda_hip.so              the deformable-attention operator
    clip            libclip_ops_hip.so          fused small-tensor chains of the train step
    frame           libframe_ops_hip.so         raw-frame resize / normalise
    augment         libaugment_ops_hip.so       training-clip augmentation
    static_clip     libstatic_clip_ops_hip.so   clips made from one still image
    track_eval      libtrack_eval_hip.so        HOTA / CLEAR / Identity evaluation
    track_eval_bdd  libtrack_eval_bdd_hip.so    BDD100K's class split and preprocessing in front of it
    track_motion    libtrack_motion_hip.so      the online tracker's motion post-process
    jpeg            libjpeg_ops_hip.so          JPEG decode: host entropy stage and device pixels
    jpeg_enc        libjpeg_enc_hip.so          JPEG encode: device coefficients and host Huffman stage
    track_draw      libtrack_draw_hip.so        track overlay
    opt             libopt_ops_hip.so           gradient clipping + AdamW step
"""
from __future__ import annotations

import os
import re
import shutil
import subprocess
from functools import partial
from typing import NamedTuple

_HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(_HERE, "csrc", "msda_hip.hip")
HDR = os.path.join(os.path.dirname(_HERE), "include", "msda_hip.h")
# the operator's kernels, one header per family, and its host-side dispatch, all included by msda_hip.hip
KERNEL_HEADERS = tuple(os.path.join(_HERE, "csrc", n) for n in (
    "msda_common.h", "msda_select.h", "msda_generic.h", "msda_fwd_gather.h", "msda_fwd_win.h", "msda_tile.h",
    "msda_bwd_tile_lv.h", "msda_bwd_bins.h", "msda_bwd_rows.h", "msda_bwd_sorted.h", "msda_fused_side.h",
    "msda_dispatch_fwd.h", "msda_dispatch_bwd.h", "msda_attn_map.h"))
LIB_DIR = os.path.join(_HERE, "lib")
LIB = os.path.join(LIB_DIR, "libmsda_hip.so")


class Lib(NamedTuple):
    src: str                # the .hip file
    out: str                # the shared library
    extra: tuple = ()       # flags after HIPCC_FLAGS


def _lib(src: str, out: str, *extra: str) -> Lib:
    return Lib(os.path.join(_HERE, "csrc", src), os.path.join(LIB_DIR, out), extra)


LIBS = {
    "msda": _lib("msda_hip.hip", "libmsda_hip.so"),
    "clip": _lib("clip_ops.hip", "libclip_ops_hip.so"),
    "frame": _lib("frame_ops.hip", "libframe_ops_hip.so"),
    "augment": _lib("augment_ops.hip", "libaugment_ops_hip.so"),
    "static_clip": _lib("static_clip_ops.hip", "libstatic_clip_ops_hip.so"),
    # float64 results are held to TrackEval's bit for bit where the definition allows it: no fused multiply-add
    "track_eval": _lib("track_eval.hip", "libtrack_eval_hip.so", "-ffp-contract=off"),
    # the same arithmetic rules as libtrack_eval_hip.so: similarities are TrackEval's bit for bit
    "track_eval_bdd": _lib("track_eval_bdd.hip", "libtrack_eval_bdd_hip.so", "-ffp-contract=off"),
    # float32 add, mul and div are the host statement's bit for bit (models/motion.py): no fused multiply-add
    "track_motion": _lib("track_motion.hip", "libtrack_motion_hip.so", "-ffp-contract=off"),
    # int32 products of hostile coefficients wrap, as the numpy statement's do; the batch entry point starts threads
    "jpeg": _lib("jpeg_ops.hip", "libjpeg_ops_hip.so", "-fwrapv", "-pthread"),
    "jpeg_enc": _lib("jpeg_enc.hip", "libjpeg_enc_hip.so", "-pthread"),     # the batch entry point starts threads
    "track_draw": _lib("track_draw.hip", "libtrack_draw_hip.so"),
    # every float32 operation of the update is rounded once, as include/opt_ops_hip.h states it: no fused multiply-add
    "opt": _lib("opt_ops.hip", "libopt_ops_hip.so", "-ffp-contract=off"),
}

HIPCC_FLAGS = [
    "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
    "-munsafe-fp-atomics",      # float/double atomicAdd -> global_atomic_add_f32/_f64
]


def hipcc_path() -> str:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (ROCm toolchain required to build libmsda_hip.so)")


def source_hash() -> str:
    """sha256 (first 16 hex digits) of the kernel sources: stamps measurements (profiles/traffic.json) so that a
    number taken on other kernels is recognised as stale."""
    import hashlib
    h = hashlib.sha256()
    for p in (SRC,) + KERNEL_HEADERS:
        with open(p, "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


_INCLUDE = re.compile(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', re.M)


def sources(name: str) -> list:
    """The library's .hip file and every file it reaches through ``#include "..."`` lines, each resolved relative to
    the file that includes it.  (No include here is conditional or spelled by a macro.)"""
    seen, todo = [], [LIBS[name].src]
    while todo:
        path = todo.pop()
        if path in seen:
            continue
        seen.append(path)
        with open(path) as f:
            todo += [os.path.normpath(os.path.join(os.path.dirname(path), inc)) for inc in _INCLUDE.findall(f.read())]
    return seen


def stale(name: str) -> bool:
    """The library is missing, or older than one of its ``sources``."""
    out = LIBS[name].out
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(p) > t for p in sources(name))


def needs_build() -> bool:
    return stale("msda")


def build(name: str, force: bool = False, verbose: bool = False) -> str:
    src, out, extra = LIBS[name]
    if not force and not stale(name):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = [hipcc_path(), *HIPCC_FLAGS, *extra, src, "-o", out]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return out


def build_all(force: bool = False, verbose: bool = False) -> list:
    return [build(name, force, verbose) for name in LIBS]


# the public names of the single libraries (test fixtures, the driver hooks)
build_lib = partial(build, "msda")
build_clip_lib = partial(build, "clip")
build_frame_lib = partial(build, "frame")
build_augment_lib = partial(build, "augment")
build_static_clip_lib = partial(build, "static_clip")
build_track_eval_lib = partial(build, "track_eval")
build_track_eval_bdd_lib = partial(build, "track_eval_bdd")
build_track_motion_lib = partial(build, "track_motion")
build_jpeg_lib = partial(build, "jpeg")
build_jpeg_enc_lib = partial(build, "jpeg_enc")
build_track_draw_lib = partial(build, "track_draw")
build_opt_lib = partial(build, "opt")


if __name__ == "__main__":
    for lib_path in build_all(force=True, verbose=True):
        print(lib_path)
