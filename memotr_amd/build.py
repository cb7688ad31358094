"""Build memotr_amd/lib/libmsda_hip.so (the operator), libclip_ops_hip.so (fused small-tensor chains of the train
step), libframe_ops_hip.so (raw-frame resize / normalise), libaugment_ops_hip.so (training-clip augmentation),
libstatic_clip_ops_hip.so (clips made from one still image), libtrack_eval_hip.so (HOTA / CLEAR / Identity
evaluation), libtrack_eval_bdd_hip.so (BDD100K's class split and preprocessing in front of it) and
libtrack_motion_hip.so (the online tracker's motion post-process) and libjpeg_ops_hip.so (JPEG decode: host entropy
stage and device pixels), libjpeg_enc_hip.so (JPEG encode: device coefficients and host Huffman stage) and
libtrack_draw_hip.so (track overlay) and libopt_ops_hip.so (gradient clipping + AdamW step) with hipcc for gfx950 (cross-compiles without a GPU)."""
from __future__ import annotations

import os
import shutil
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(_HERE, "csrc", "msda_hip.hip")
HDR = os.path.join(os.path.dirname(_HERE), "include", "msda_hip.h")
# the operator's kernels, one header per family, and its host-side dispatch, all included by msda_hip.hip
KERNEL_HEADERS = tuple(os.path.join(_HERE, "csrc", n) for n in (
    "msda_common.h", "msda_select.h", "msda_generic.h", "msda_fwd_gather.h", "msda_fwd_win.h", "msda_tile.h",
    "msda_bwd_tile_lv.h", "msda_bwd_bins.h", "msda_bwd_rows.h", "msda_bwd_sorted.h", "msda_fused_side.h",
    "msda_dispatch_fwd.h", "msda_dispatch_bwd.h"))
LIB_DIR = os.path.join(_HERE, "lib")
LIB = os.path.join(LIB_DIR, "libmsda_hip.so")
CLIP_SRC = os.path.join(_HERE, "csrc", "clip_ops.hip")
CLIP_HDR = os.path.join(os.path.dirname(_HERE), "include", "clip_ops_hip.h")
CLIP_LIB = os.path.join(LIB_DIR, "libclip_ops_hip.so")
ASSIGN_CORE = os.path.join(_HERE, "csrc", "assign_core.h")
FRAME_SRC = os.path.join(_HERE, "csrc", "frame_ops.hip")
FRAME_HDR = os.path.join(os.path.dirname(_HERE), "include", "frame_ops_hip.h")
FRAME_LIB = os.path.join(LIB_DIR, "libframe_ops_hip.so")
AUGMENT_SRC = os.path.join(_HERE, "csrc", "augment_ops.hip")
AUGMENT_HDR = os.path.join(os.path.dirname(_HERE), "include", "augment_ops_hip.h")
AUGMENT_LIB = os.path.join(LIB_DIR, "libaugment_ops_hip.so")
STATIC_CLIP_SRC = os.path.join(_HERE, "csrc", "static_clip_ops.hip")
STATIC_CLIP_HDR = os.path.join(os.path.dirname(_HERE), "include", "static_clip_ops_hip.h")
STATIC_CLIP_LIB = os.path.join(LIB_DIR, "libstatic_clip_ops_hip.so")
TRACK_EVAL_SRC = os.path.join(_HERE, "csrc", "track_eval.hip")
TRACK_EVAL_HDR = os.path.join(os.path.dirname(_HERE), "include", "track_eval_hip.h")
TRACK_EVAL_LIB = os.path.join(LIB_DIR, "libtrack_eval_hip.so")
TRACK_EVAL_BDD_SRC = os.path.join(_HERE, "csrc", "track_eval_bdd.hip")
TRACK_EVAL_BDD_HDR = os.path.join(os.path.dirname(_HERE), "include", "track_eval_bdd_hip.h")
TRACK_EVAL_BDD_LIB = os.path.join(LIB_DIR, "libtrack_eval_bdd_hip.so")
TRACK_MOTION_SRC = os.path.join(_HERE, "csrc", "track_motion.hip")
TRACK_MOTION_HDR = os.path.join(os.path.dirname(_HERE), "include", "track_motion_hip.h")
TRACK_MOTION_LIB = os.path.join(LIB_DIR, "libtrack_motion_hip.so")
JPEG_SRC = os.path.join(_HERE, "csrc", "jpeg_ops.hip")
JPEG_HDR = os.path.join(os.path.dirname(_HERE), "include", "jpeg_ops_hip.h")
JPEG_CORE = os.path.join(_HERE, "csrc", "jpeg_entropy_core.h")
JPEG_LIB = os.path.join(LIB_DIR, "libjpeg_ops_hip.so")
JPEG_ENC_SRC = os.path.join(_HERE, "csrc", "jpeg_enc.hip")
JPEG_ENC_HDR = os.path.join(os.path.dirname(_HERE), "include", "jpeg_enc_hip.h")
JPEG_ENC_CORE = os.path.join(_HERE, "csrc", "jpeg_encode_core.h")
JPEG_ENC_LIB = os.path.join(LIB_DIR, "libjpeg_enc_hip.so")
TRACK_DRAW_SRC = os.path.join(_HERE, "csrc", "track_draw.hip")
TRACK_DRAW_HDR = os.path.join(os.path.dirname(_HERE), "include", "track_draw_hip.h")
TRACK_DRAW_LIB = os.path.join(LIB_DIR, "libtrack_draw_hip.so")
OPT_SRC = os.path.join(_HERE, "csrc", "opt_ops.hip")
OPT_HDR = os.path.join(os.path.dirname(_HERE), "include", "opt_ops_hip.h")
OPT_LIB = os.path.join(LIB_DIR, "libopt_ops_hip.so")

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


def _stale(lib: str, deps) -> bool:
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    return any(os.path.getmtime(p) > t for p in deps)


def needs_build() -> bool:
    return _stale(LIB, (SRC, HDR) + KERNEL_HEADERS)


def _compile(src: str, lib: str, verbose: bool, extra=()) -> str:
    os.makedirs(LIB_DIR, exist_ok=True)
    cmd = [hipcc_path(), *HIPCC_FLAGS, *extra, src, "-o", lib]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return lib


def build_lib(force: bool = False, verbose: bool = False) -> str:
    if not force and not needs_build():
        return LIB
    return _compile(SRC, LIB, verbose)


def build_clip_lib(force: bool = False, verbose: bool = False) -> str:
    if not force and not _stale(CLIP_LIB, (CLIP_SRC, CLIP_HDR, ASSIGN_CORE)):
        return CLIP_LIB
    return _compile(CLIP_SRC, CLIP_LIB, verbose)


def build_frame_lib(force: bool = False, verbose: bool = False) -> str:
    if not force and not _stale(FRAME_LIB, (FRAME_SRC, FRAME_HDR)):
        return FRAME_LIB
    return _compile(FRAME_SRC, FRAME_LIB, verbose)


def build_augment_lib(force: bool = False, verbose: bool = False) -> str:
    if not force and not _stale(AUGMENT_LIB, (AUGMENT_SRC, AUGMENT_HDR)):
        return AUGMENT_LIB
    return _compile(AUGMENT_SRC, AUGMENT_LIB, verbose)


def build_static_clip_lib(force: bool = False, verbose: bool = False) -> str:
    if not force and not _stale(STATIC_CLIP_LIB, (STATIC_CLIP_SRC, STATIC_CLIP_HDR)):
        return STATIC_CLIP_LIB
    return _compile(STATIC_CLIP_SRC, STATIC_CLIP_LIB, verbose)


def build_track_eval_lib(force: bool = False, verbose: bool = False) -> str:
    if not force and not _stale(TRACK_EVAL_LIB, (TRACK_EVAL_SRC, TRACK_EVAL_HDR, ASSIGN_CORE)):
        return TRACK_EVAL_LIB
    # float64 results are held to TrackEval's bit for bit where the definition allows it: no fused multiply-add
    return _compile(TRACK_EVAL_SRC, TRACK_EVAL_LIB, verbose, extra=("-ffp-contract=off",))


def build_track_eval_bdd_lib(force: bool = False, verbose: bool = False) -> str:
    deps = (TRACK_EVAL_BDD_SRC, TRACK_EVAL_BDD_HDR, TRACK_EVAL_HDR, ASSIGN_CORE)
    if not force and not _stale(TRACK_EVAL_BDD_LIB, deps):
        return TRACK_EVAL_BDD_LIB
    # the same arithmetic rules as libtrack_eval_hip.so: similarities are TrackEval's bit for bit
    return _compile(TRACK_EVAL_BDD_SRC, TRACK_EVAL_BDD_LIB, verbose, extra=("-ffp-contract=off",))


def build_track_motion_lib(force: bool = False, verbose: bool = False) -> str:
    if not force and not _stale(TRACK_MOTION_LIB, (TRACK_MOTION_SRC, TRACK_MOTION_HDR)):
        return TRACK_MOTION_LIB
    # float32 add, mul and div are the host statement's bit for bit (models/motion.py): no fused multiply-add
    return _compile(TRACK_MOTION_SRC, TRACK_MOTION_LIB, verbose, extra=("-ffp-contract=off",))


def build_jpeg_lib(force: bool = False, verbose: bool = False) -> str:
    if not force and not _stale(JPEG_LIB, (JPEG_SRC, JPEG_HDR, JPEG_CORE)):
        return JPEG_LIB
    # int32 products of hostile coefficients wrap, as the numpy statement's do; the batch entry point starts threads
    return _compile(JPEG_SRC, JPEG_LIB, verbose, extra=("-fwrapv", "-pthread"))


def build_jpeg_enc_lib(force: bool = False, verbose: bool = False) -> str:
    if not force and not _stale(JPEG_ENC_LIB, (JPEG_ENC_SRC, JPEG_ENC_HDR, JPEG_ENC_CORE)):
        return JPEG_ENC_LIB
    return _compile(JPEG_ENC_SRC, JPEG_ENC_LIB, verbose, extra=("-pthread",))     # the batch entry point starts threads


def build_track_draw_lib(force: bool = False, verbose: bool = False) -> str:
    if not force and not _stale(TRACK_DRAW_LIB, (TRACK_DRAW_SRC, TRACK_DRAW_HDR)):
        return TRACK_DRAW_LIB
    return _compile(TRACK_DRAW_SRC, TRACK_DRAW_LIB, verbose)


def build_opt_lib(force: bool = False, verbose: bool = False) -> str:
    if not force and not _stale(OPT_LIB, (OPT_SRC, OPT_HDR)):
        return OPT_LIB
    # every float32 operation of the update is rounded once, as include/opt_ops_hip.h states it: no fused multiply-add
    return _compile(OPT_SRC, OPT_LIB, verbose, extra=("-ffp-contract=off",))


if __name__ == "__main__":
    print(build_lib(force=True, verbose=True))
    print(build_clip_lib(force=True, verbose=True))
    print(build_frame_lib(force=True, verbose=True))
    print(build_augment_lib(force=True, verbose=True))
    print(build_static_clip_lib(force=True, verbose=True))
    print(build_track_eval_lib(force=True, verbose=True))
    print(build_track_eval_bdd_lib(force=True, verbose=True))
    print(build_track_motion_lib(force=True, verbose=True))
    print(build_jpeg_lib(force=True, verbose=True))
    print(build_jpeg_enc_lib(force=True, verbose=True))
    print(build_track_draw_lib(force=True, verbose=True))
    print(build_opt_lib(force=True, verbose=True))
