"""CPU: the one loader of the HIP libraries (memotr_amd/_cabi.py), on the smallest of them, libframe_ops_hip.so:
what it raises for a missing file, another ABI version and a name the library lacks, and what its ``check`` does."""
import ctypes
import os
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT

from memotr_amd import _cabi

FILE, PREFIX = "libframe_ops_hip.so", "frameops"


@pytest.fixture(scope="module")
def frame_lib():
    from memotr_amd.build import build_frame_lib
    build_frame_lib()
    from memotr_amd import _frame_lib
    return _frame_lib


def test_a_missing_file_names_the_path_and_the_build_command(frame_lib, tmp_path):
    missing = str(tmp_path / "nowhere" / FILE)
    with pytest.raises(ImportError) as e:
        _cabi.bind(FILE, PREFIX, frame_lib.SYMBOLS, frame_lib.ABI_VERSION, path=missing)
    assert missing in str(e.value) and "memotr_amd.build" in str(e.value)
    with pytest.raises(ImportError, match="has no CPU fallback"):
        _cabi.bind(FILE, PREFIX, frame_lib.SYMBOLS, frame_lib.ABI_VERSION, path=missing,
                   missing_note=" memotr_amd has no CPU fallback.")


def test_another_abi_version_is_refused(frame_lib):
    want = frame_lib.ABI_VERSION + 1
    with pytest.raises(ImportError) as e:
        _cabi.bind(FILE, PREFIX, frame_lib.SYMBOLS, want)
    assert f"ABI {frame_lib.ABI_VERSION} != binding ABI {want}" in str(e.value) and "rebuild" in str(e.value)


def test_a_name_the_library_does_not_export_is_an_attribute_error(frame_lib):
    symbols = dict(frame_lib.SYMBOLS, frameops_no_such_entry=([], ctypes.c_int))
    with pytest.raises(AttributeError, match="frameops_no_such_entry"):
        _cabi.bind(FILE, PREFIX, symbols, frame_lib.ABI_VERSION)


def test_bind_returns_the_declared_library_and_its_check(frame_lib):
    lib, check = _cabi.bind(FILE, PREFIX, frame_lib.SYMBOLS, frame_lib.ABI_VERSION)
    assert type(lib) is ctypes.CDLL and type(frame_lib.lib) is ctypes.CDLL        # no proxy in front of the calls
    fn = lib.frameops_resize_normalize_u8
    assert list(fn.argtypes) == frame_lib.SYMBOLS["frameops_resize_normalize_u8"][0] and fn.restype is ctypes.c_int
    assert check(0, "x") is None
    p = ctypes.c_void_p(4096)               # never dereferenced: the null source is refused first, nothing is launched
    rc = fn(None, 192, 9216, 1, 48, 64, p, p, p, p, p, p, 60, 80, 64, 96, p, 0, p, None)
    assert rc != 0
    message = lib.frameops_last_error().decode()
    assert "null" in message
    with pytest.raises(RuntimeError) as e:
        check(rc, "x")
    assert str(e.value) == f"x failed ({rc}): {message}"
    with pytest.raises(RuntimeError, match="x failed"):
        frame_lib.check(rc, "x")


def test_the_operator_library_can_be_replaced_for_an_a_b_build(hip_lib, tmp_path):
    copy = str(tmp_path / "libmsda_other.so")
    shutil.copy(hip_lib.LIB_PATH, copy)
    out = subprocess.run([sys.executable, "-c", "from memotr_amd import _lib; print(_lib.LIB_PATH)"], cwd=ROOT,
                         env=dict(os.environ, MEMOTR_MSDA_LIB=copy), capture_output=True, text=True, timeout=300,
                         check=True)                                        # the child imports, it opens no device
    assert out.stdout.strip().splitlines()[-1] == copy
