"""The convolution C-ABI (include/tnn_conv.h): header, ctypes table and libtnn_hip.so agree, and none of it leaks into
include/tnn_hip.h (whose every symbol the CPU test twin must export)."""

import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT, TWIN_SO

HEADER = os.path.join(ROOT, "include", "tnn_conv.h")
MAIN_HEADER = os.path.join(ROOT, "include", "tnn_hip.h")
LIB = os.path.join(ROOT, "tinynn-autograd_amd", "lib", "libtnn_hip.so")


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"TNN_API\s+[\w\s\*]+?\b(tnn_\w+)\s*\(", text)))


def exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_header_table_and_library_agree():
    from tinynn_autograd_amd import _lib
    syms = declared(HEADER)
    assert syms == sorted(_lib._CONV_SIGNATURES) == _lib.CONV_SYMBOLS
    assert {"tnn_conv2d_fwd", "tnn_conv2d_bwd_data", "tnn_conv2d_bwd_filter", "tnn_maxpool2d_fwd", "tnn_maxpool2d_bwd"} <= set(syms)
    assert os.path.exists(LIB), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    exp = exported(LIB)
    assert set(syms) <= exp
    assert {s for s in exp if s.startswith(("tnn_conv", "tnn_maxpool"))} == set(syms)


def test_signatures_match_the_declarations():
    """Argument count and the order of pointer / 64-bit / int arguments of the ctypes table follow the header."""
    from tinynn_autograd_amd import _conv_signatures as S, conv
    text = header_text()
    table = {ctypes.c_void_p: "p", ctypes.c_int64: "i64", ctypes.c_int: "int", S._i64p: "i64p"}
    for name, argtypes in S._CONV_SIGNATURES.items():
        args = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        kinds = []
        for arg in args.split(","):
            arg = arg.strip()
            kinds.append("i64p" if "int64_t*" in arg else "p" if "*" in arg else "i64" if "int64_t" in arg else "int")
        assert kinds == [table[t] for t in argtypes], name
    for name, value in (("AUTO", S.FORM_AUTO), ("TILE", S.FORM_TILE), ("SMALL", S.FORM_SMALL)):
        assert re.search(r"#define TNN_CONV_FORM_%s %d\b" % (name, value), text)
        assert getattr(conv, "FORM_" + name) == value
    assert re.search(r"#define TNN_CONV_TILE_ELEMS %d\b" % S.TILE_ELEMS, text) and conv.TILE_ELEMS == S.TILE_ELEMS


def test_not_declared_in_the_main_header():
    from tinynn_autograd_amd import _lib
    assert not set(declared(HEADER)) & set(declared(MAIN_HEADER))
    for other in (_lib.EXPORTED_SYMBOLS, _lib._INDEX_SIGNATURES, _lib._BMM_SIGNATURES):
        assert not set(_lib._CONV_SIGNATURES) & set(other)


def test_the_test_twin_takes_the_composed_route():
    """The twin exports none of it: `has_conv` is False, a raw call says so, and conv2d runs the tap loop instead."""
    import numpy as np
    import tinynn_autograd_amd as tn
    from tinynn_autograd_amd import _lib, device_array as da
    if tn.backend_name() == "hip-gfx950":
        pytest.skip("the product library is loaded (GPU machine)")
    assert not exported(TWIN_SO) & set(_lib.CONV_SYMBOLS)
    lib = _lib.get()
    assert not lib.has_conv
    with pytest.raises(_lib.TnnError, match="needs libtnn_hip.so"):
        lib.conv2d_fwd()
    x = np.arange(32.0, dtype=np.float32).reshape(1, 2, 4, 4)
    w = np.ones((1, 2, 2, 2), dtype=np.float32)
    y = np.asarray(da.conv2d(tn.asarray(x), tn.asarray(w)))
    np.testing.assert_array_equal(y[0, 0, 0], [84.0, 92.0, 100.0])
    with pytest.raises(ValueError, match="native"):
        da.conv2d(tn.asarray(x), tn.asarray(w), route="native")
