"""CPU: libtrack_motion_hip.so loads and exports exactly what include/track_motion_hip.h declares; argument
validation is host-side and works without a device (nothing is launched here)."""
import ctypes

import pytest

from cabi_helpers import assert_binding_matches_header, assert_parameter_counts, define


@pytest.fixture(scope="module")
def motion_lib():
    from memotr_amd.build import build_track_motion_lib
    build_track_motion_lib()
    from memotr_amd import _track_motion_lib
    return _track_motion_lib


HEADER = "track_motion_hip.h"


def test_library_exports_every_declared_symbol(motion_lib):
    syms = assert_binding_matches_header(motion_lib, HEADER, "trackmotion", "TRACKMOTION_ABI_VERSION")
    assert syms == ["trackmotion_abi_version", "trackmotion_extrapolate", "trackmotion_last_error",
                    "trackmotion_observe", "trackmotion_register"]
    from memotr_amd.models import motion
    assert define(HEADER, "TRACKMOTION_MAX_LENGTH") == motion_lib.MAX_LENGTH == motion.MAX_LENGTH == 16
    assert define(HEADER, "TRACKMOTION_STATUS_NEGATIVE_ID") == motion_lib.STATUS_NEGATIVE_ID
    assert define(HEADER, "TRACKMOTION_STATUS_ID_PAST_CAPACITY") == motion_lib.STATUS_ID_PAST_CAPACITY
    assert define(HEADER, "TRACKMOTION_STATUS_BAD_LABEL") == motion_lib.STATUS_BAD_LABEL


def test_declared_parameter_counts_match_the_binding(motion_lib):
    assert_parameter_counts(motion_lib, HEADER)


def test_argument_errors_are_reported_without_a_device(motion_lib):
    lib = motion_lib.lib
    p = ctypes.c_void_p(4096)             # never dereferenced: validation is host-side and comes before any launch
    err = lib.trackmotion_last_error
    calls = {
        "trackmotion_observe": lambda n=3, a=p, L=5, cap=8, K=1: lib.trackmotion_observe(
            a, p, p, p, p, p, n, K, 0.5, 4, p, p, cap, L, p, p, p, p, None),
        "trackmotion_register": lambda n=3, a=p, L=5, cap=8, first=0: lib.trackmotion_register(
            a, n, first, p, p, cap, L, None),
        "trackmotion_extrapolate": lambda n=3, a=p, L=5, cap=8, m=3: lib.trackmotion_extrapolate(
            a, p, p, p, n, 0.5, m, p, p, cap, L, p, None, None),
    }
    for name, call in calls.items():
        assert call(a=None) == 1 and b"null pointer" in err() and name.encode() in err(), name
        assert call(n=-1) == 1 and b"negative" in err() and name.encode() in err(), name
        assert call(cap=-1) == 1 and b"negative" in err(), name
        for L in (1, 17, -3):
            assert call(L=L) == 1 and b"outside 2 .. 16" in err() and name.encode() in err(), (name, L)
        assert call(n=2 ** 31 // 4 + 1) == 2 and b"exceed" in err(), name
        assert call(n=0) == 0 and err() == b"", name             # an empty call launches nothing and clears the text
        assert call(n=0, a=None) == 0, name
    assert calls["trackmotion_extrapolate"](m=1) == 1 and b"min_length < 2" in err()
    assert calls["trackmotion_observe"](K=0) == 1 and b"K < 1" in err()
    assert calls["trackmotion_observe"](K=-1) == 1 and b"negative" in err()
    assert calls["trackmotion_register"](first=6) == 1 and b"outside the table" in err() and b"6 .. 8" in err()
    assert calls["trackmotion_register"](first=-1) == 1 and b"outside the table" in err()
    with pytest.raises(RuntimeError, match="null pointer"):
        motion_lib.check(calls["trackmotion_register"](a=None), "trackmotion_register")


def test_cuda_tensors_without_a_kernel_are_an_error_not_a_fallback():
    """The device path calls the library and nothing else: the source of MotionState has no torch fallback in it."""
    import inspect
    from memotr_amd.models.motion import MotionState
    for op in (MotionState.observe, MotionState.register, MotionState.extrapolate):
        src = inspect.getsource(op)
        assert "L.check(L.lib.trackmotion_" in src and "except" not in src
    module = inspect.getsource(inspect.getmodule(MotionState))
    body = module.split('"""', 2)[2]              # (the docstring names the calls the code must not make)
    for banned in (".item()", ".tolist()", ".cpu()", ".nonzero("):
        assert banned not in body, banned
