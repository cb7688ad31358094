"""Shared by the C-ABI tests of the HIP libraries: what a header under include/ declares, against what the library
exports and what the ctypes binding (a ``memotr_amd._*lib`` module) states."""
import ctypes
import os
import re

from conftest import ROOT


def header_text(header_file):
    """include/<header_file> without its ``/* */`` and ``//`` comments."""
    with open(os.path.join(ROOT, "include", header_file)) as f:
        text = f.read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def define(header_file, name):
    return int(re.search(rf"#define {name} (\d+)", header_text(header_file)).group(1))


def declared_symbols(header_file, prefix):
    return sorted(set(re.findall(rf"\b({prefix}_\w+)\s*\(", header_text(header_file))))


def assert_parameter_counts(mod, header_file):
    text = header_text(header_file)
    for name, (argtypes, _) in mod.SYMBOLS.items():
        params = re.search(rf"\b{name}\s*\(([^)]*)\)", text).group(1).strip()
        assert (0 if params == "void" else params.count(",") + 1) == len(argtypes), name


def assert_binding_matches_header(mod, header_file, prefix, abi_macro=None):
    """The library exports every declared name, ``mod.SYMBOLS`` names exactly those with the declared parameter
    counts, and the ABI versions of library, binding and header agree.  Returns the declared names."""
    declared = declared_symbols(header_file, prefix)
    raw = ctypes.CDLL(mod.LIB_PATH)
    for s in declared:
        assert hasattr(raw, s), f"{os.path.basename(mod.LIB_PATH)} does not export {s}"
    assert sorted(mod.SYMBOLS) == declared
    assert_parameter_counts(mod, header_file)
    assert getattr(mod.lib, prefix + "_abi_version")() == mod.ABI_VERSION
    if abi_macro is not None:
        assert define(header_file, abi_macro) == mod.ABI_VERSION
    return declared
