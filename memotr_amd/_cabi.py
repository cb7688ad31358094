"""The one loader of the package's HIP libraries: every ``_*lib.py`` binds its library through ``bind``.

``lib`` is the raw ``ctypes.CDLL`` with ``argtypes`` / ``restype`` set, so a call costs no Python frame of ours.
"""
from __future__ import annotations

import ctypes
import os


def lib_path(file_name: str) -> str:
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", file_name)


def declare(lib: ctypes.CDLL, symbols) -> ctypes.CDLL:
    """Set ``argtypes`` / ``restype`` of every name in ``symbols`` (name -> (argtypes, restype))."""
    for name, (argtypes, restype) in symbols.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export it
        fn.argtypes = argtypes
        fn.restype = restype
    return lib


def bind(file_name: str, prefix: str, symbols, abi_version: int, path: str | None = None, missing_note: str = ""):
    """Load ``lib/<file_name>`` (or ``path``), declare ``symbols``, compare ``<prefix>_abi_version()`` with
    ``abi_version``.  Returns ``(lib, check)``; ``check(rc, what)`` raises ``<prefix>_last_error()`` for ``rc != 0``."""
    path = path or lib_path(file_name)
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: build it with `python -m memotr_amd.build` "
                          f"(hipcc --offload-arch=gfx950).{missing_note}")
    # torch ships its own libamdhip64 (same SONAME); importing it first makes the HIP
    # library bind to the runtime torch's streams/allocations live in.
    import torch  # noqa: F401

    lib = declare(ctypes.CDLL(path), symbols)
    got = getattr(lib, prefix + "_abi_version")()
    if got != abi_version:
        raise ImportError(f"{file_name} ABI {got} != binding ABI {abi_version}; rebuild the library")
    last_error = getattr(lib, prefix + "_last_error")

    def check(rc: int, what: str) -> None:
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): {last_error().decode()}")

    return lib, check
