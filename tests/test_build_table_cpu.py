"""CPU: the build table (memotr_amd/build.py LIBS): one row per .hip file and per binding module, staleness
dependencies scanned from the ``#include "..."`` lines, and one build function.
Nothing is compiled here but libframe_ops_hip.so, where it is missing."""
import glob
import os
import re
import shutil

import pytest

from conftest import ROOT

from memotr_amd import build as B

CSRC = os.path.join(ROOT, "memotr_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
# what each library was declared to depend on when the lists were written by hand: csrc/ names, include/ names
HAND_WRITTEN = {
    "clip": (["clip_ops.hip", "assign_core.h", "clip_common.h", "clip_criterion.h", "clip_handover.h", "clip_boxes.h",
              "clip_rows.h", "clip_attention.h", "clip_linear.h", "clip_tracks.h", "clip_fill_gaps.h"], ["clip_ops_hip.h"]),
    "frame": (["frame_ops.hip"], ["frame_ops_hip.h"]),
    "augment": (["augment_ops.hip"], ["augment_ops_hip.h"]),
    "static_clip": (["static_clip_ops.hip"], ["static_clip_ops_hip.h"]),
    "track_eval": (["track_eval.hip", "assign_core.h"], ["track_eval_hip.h"]),
    "track_eval_bdd": (["track_eval_bdd.hip", "assign_core.h"], ["track_eval_bdd_hip.h", "track_eval_hip.h"]),
    "track_motion": (["track_motion.hip"], ["track_motion_hip.h"]),
    "jpeg": (["jpeg_ops.hip", "jpeg_entropy_core.h"], ["jpeg_ops_hip.h"]),
    "jpeg_enc": (["jpeg_enc.hip", "jpeg_encode_core.h"], ["jpeg_enc_hip.h"]),
    "track_draw": (["track_draw.hip"], ["track_draw_hip.h"]),
    "opt": (["opt_ops.hip"], ["opt_ops_hip.h"]),
}


def test_every_hip_file_is_the_source_of_exactly_one_row():
    assert sorted(lib.src for lib in B.LIBS.values()) == sorted(glob.glob(os.path.join(CSRC, "*.hip")))
    assert len({lib.out for lib in B.LIBS.values()}) == len(B.LIBS) == 12
    assert B.LIBS["msda"][:2] == (B.SRC, B.LIB) and all(os.path.dirname(lib.out) == B.LIB_DIR for lib in B.LIBS.values())


def test_every_binding_module_loads_some_rows_output_and_the_docstring_lists_the_rows():
    outputs = {os.path.basename(lib.out) for lib in B.LIBS.values()}
    modules = sorted(glob.glob(os.path.join(ROOT, "memotr_amd", "_*lib.py")))
    assert len(modules) == 12
    bound = set()
    for path in modules:
        with open(path) as f:
            text = f.read()
        (loaded,) = re.findall(r'_cabi\.bind\("([^"]+)"', text)
        assert re.findall(r'_cabi\.lib_path\("([^"]+)"\)', text) == [loaded], path        # LIB_PATH is what is loaded
        bound.add(loaded)
    assert bound == outputs
    rows = re.findall(r"^    (\w+) +(lib\w+\.so) ", B.__doc__, flags=re.M)
    assert rows == [(name, os.path.basename(lib.out)) for name, lib in B.LIBS.items()]


def test_the_include_scan_finds_what_the_hand_written_lists_named():
    assert set(B.sources("msda")) == {B.SRC, B.HDR} | set(B.KERNEL_HEADERS)
    assert len(B.sources("msda")) == 2 + len(B.KERNEL_HEADERS)
    assert set(HAND_WRITTEN) == set(B.LIBS) - {"msda"}
    for name, (csrc, include) in HAND_WRITTEN.items():
        want = [os.path.join(CSRC, n) for n in csrc] + [os.path.join(INCLUDE, n) for n in include]
        assert sorted(B.sources(name)) == sorted(want), name
        assert B.sources(name)[0] == B.LIBS[name].src


@pytest.fixture()
def redirected(tmp_path, monkeypatch):
    """The ``jpeg`` row on a copy of its sources (same relative layout) and an output under ``tmp_path``; hipcc replaced
    by a function that records its command line and touches the output."""
    files = {}
    for rel in ("memotr_amd/csrc/jpeg_ops.hip", "memotr_amd/csrc/jpeg_entropy_core.h", "include/jpeg_ops_hip.h"):
        files[os.path.basename(rel)] = dst = str(tmp_path / rel)
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        shutil.copy(os.path.join(ROOT, rel), dst)
    row = B.LIBS["jpeg"]._replace(src=files["jpeg_ops.hip"], out=str(tmp_path / "out" / "libjpeg_ops_hip.so"))
    monkeypatch.setitem(B.LIBS, "jpeg", row)
    commands = []

    def hipcc(cmd):
        commands.append(cmd)
        with open(cmd[-1], "wb"):
            pass
        newest = max(os.path.getmtime(p) for p in files.values())
        os.utime(cmd[-1], (newest + 1, newest + 1))

    monkeypatch.setattr(B.subprocess, "check_call", hipcc)
    return row, files, commands


def test_build_compiles_when_stale_and_only_then(redirected):
    row, files, commands = redirected
    assert sorted(B.sources("jpeg")) == sorted(files.values())
    assert B.stale("jpeg") and B.build("jpeg") == row.out and len(commands) == 1
    assert commands[0] == [B.hipcc_path(), *B.HIPCC_FLAGS, "-fwrapv", "-pthread", row.src, "-o", row.out]
    assert not B.stale("jpeg") and B.build("jpeg") == row.out and B.build_jpeg_lib() == row.out and len(commands) == 1
    for n, header in enumerate(("jpeg_ops_hip.h", "jpeg_entropy_core.h", "jpeg_ops.hip"), start=2):
        t = os.path.getmtime(row.out) + 1
        os.utime(files[header], (t, t))
        assert B.stale("jpeg") and B.build("jpeg") == row.out and len(commands) == n, header
        assert not B.stale("jpeg")
    assert B.build("jpeg", force=True) == row.out and len(commands) == 5 and commands[4] == commands[0]


def test_the_public_names_are_the_rows():
    assert B.build_frame_lib.func is B.build and B.build_frame_lib.args == ("frame",)
    names = {"build_lib": "msda", "build_jpeg_lib": "jpeg"}
    names.update({f"build_{n}_lib": n for n in B.LIBS if n not in ("msda", "jpeg")})
    for public, name in names.items():
        assert getattr(B, public).args == (name,), public
    assert B.build_frame_lib() == B.build("frame") == B.LIBS["frame"].out       # (compiles it, if nothing has yet)
    assert B.needs_build() == B.stale("msda")
