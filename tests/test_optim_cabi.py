"""CPU: libopt_ops_hip.so loads and exports exactly what include/opt_ops_hip.h declares; argument validation is
host-side and works without a device (nothing is launched here)."""
import ctypes
import re

import pytest

from cabi_helpers import assert_binding_matches_header, assert_parameter_counts, define, header_text


@pytest.fixture(scope="module")
def opt_lib():
    from memotr_amd.build import build_opt_lib
    build_opt_lib()
    from memotr_amd import _opt_lib
    return _opt_lib


HEADER = "opt_ops_hip.h"


def test_library_exports_every_declared_symbol(opt_lib):
    syms = assert_binding_matches_header(opt_lib, HEADER, "optstep", "OPTSTEP_ABI_VERSION")
    assert syms == ["optstep_abi_version", "optstep_adamw", "optstep_last_error", "optstep_sumsq"]
    assert define(HEADER, "OPTSTEP_CHUNK") == opt_lib.CHUNK
    assert define(HEADER, "OPTSTEP_MAX_GROUPS") == opt_lib.MAX_GROUPS == 8
    assert define(HEADER, "OPTSTEP_MAX_CHUNKS") == opt_lib.MAX_CHUNKS


def test_declared_parameter_counts_and_record_layouts_match_the_binding(opt_lib):
    assert_parameter_counts(opt_lib, HEADER)
    text = header_text(HEADER)
    # the records the tables are assembled in: field order and sizes as the header's structs
    fields = lambda struct: re.findall(r"(\w+)\s*[;,]", re.search(   # noqa: E731
        rf"typedef struct \{{([^}}]*)\}} {struct};", text).group(1))
    assert fields("optstep_tensor") == list(opt_lib.TENSOR_DTYPE.names) and opt_lib.TENSOR_DTYPE.itemsize == 48
    assert fields("optstep_chunk") == list(opt_lib.CHUNK_DTYPE.names) and opt_lib.CHUNK_DTYPE.itemsize == 8
    assert fields("optstep_group") == [n for n, _ in opt_lib.Group._fields_]
    assert ctypes.sizeof(opt_lib.Hyper) == 8 * 5 * 8


def test_argument_errors_are_reported_without_a_device(opt_lib):
    lib = opt_lib.lib
    p = ctypes.c_void_p(4096)             # never dereferenced: validation is host-side and comes before any launch
    err = lib.optstep_last_error

    def hyper(**over):
        h = opt_lib.Hyper()
        for i in range(opt_lib.MAX_GROUPS):
            g = h.group[i]
            g.lr, g.weight_decay, g.beta1, g.beta2, g.eps = 1e-3, 1e-2, 0.9, 0.999, 1e-8
        for k, v in over.items():
            setattr(h.group[1], k, v)
        return h

    calls = {
        "optstep_sumsq": lambda a=p, nt=3, nc=5: lib.optstep_sumsq(a, p, nt, nc, p, p, p, None),
        "optstep_adamw": lambda a=p, nt=3, nc=5, h=None, ng=2, out=p: lib.optstep_adamw(
            a, p, nt, nc, p, p, p, h if h is not None else hyper(), ng, 0.1, out, None),
    }
    for name, call in calls.items():
        assert call(a=None) == 1 and b"null pointer" in err() and name.encode() in err(), name
        assert call(nc=-1) == 1 and b"negative" in err() and name.encode() in err(), name
        assert call(nt=-1) == 1 and b"negative" in err(), name
        assert call(nc=opt_lib.MAX_CHUNKS + 1) == 2 and b"exceed" in err(), name
        assert call(nt=0) == 1 and b"chunks without tensors" in err(), name
        assert call(nc=0) == 0 and err() == b"", name            # an empty call launches nothing and clears the text
        assert call(nc=0, a=None) == 0, name
    adamw = calls["optstep_adamw"]
    assert adamw(out=None) == 1 and b"null pointer" in err()
    for ng in (0, 9, -1):
        assert adamw(ng=ng) == 1 and b"outside 1 .. 8" in err(), ng
    for bad in (dict(lr=-1.0), dict(lr=float("nan")), dict(lr=float("inf")), dict(beta1=1.0), dict(beta2=-0.5),
                dict(eps=-1e-8), dict(weight_decay=-0.1)):
        assert adamw(h=hyper(**bad)) == 1 and b"invalid hyper-parameter in group 1" in err(), bad
    assert lib.optstep_adamw(p, p, 3, 5, p, p, p, None, 2, 0.1, p, None) == 1 and b"hyper" in err()
    with pytest.raises(RuntimeError, match="null pointer"):
        opt_lib.check(calls["optstep_sumsq"](a=None), "optstep_sumsq")


def test_cuda_parameters_without_a_kernel_are_an_error_not_a_fallback():
    """The device path calls the library and nothing else: ``step`` has no torch substitute behind the launches."""
    import inspect
    from memotr_amd.optim import ClipAdamW
    src = inspect.getsource(ClipAdamW.step)
    assert "L.check(L.lib.optstep_sumsq(" in src and "L.check(L.lib.optstep_adamw(" in src and "except" not in src
    device_part = src.split('if plan.device.type != "cuda":')[1]
    for banned in (".item()", ".tolist()", ".cpu()", "synchronize()\n", "clip_grad_norm_", "torch.optim"):
        assert banned not in device_part.replace("plan.events[k].synchronize()", ""), banned
