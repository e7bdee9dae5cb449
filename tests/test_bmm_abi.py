"""The batched-GEMM C-ABI (include/tnn_bmm.h): header, ctypes table and libtnn_hip.so agree, and none of it leaks into
include/tnn_hip.h (whose every symbol the CPU test twin must export)."""

import os
import re
import subprocess

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "tnn_bmm.h")
MAIN_HEADER = os.path.join(ROOT, "include", "tnn_hip.h")
LIB = os.path.join(ROOT, "tinynn-autograd_amd", "lib", "libtnn_hip.so")


def declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"TNN_API\s+[\w\s\*]+?\b(tnn_\w+)\s*\(", text)))


def exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_header_table_and_library_agree():
    from tinynn_autograd_amd import _lib
    syms = declared(HEADER)
    assert syms == sorted(_lib._BMM_SIGNATURES) == _lib.BMM_SYMBOLS
    assert "tnn_gemm_batched" in syms
    assert os.path.exists(LIB), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    exp = exported(LIB)
    assert set(syms) <= exp
    assert {s for s in exp if s.startswith("tnn_gemm_batched")} == set(syms)


def test_signature_matches_the_declaration():
    """Argument count and the order of pointer / 64-bit / int arguments of the ctypes table follow the header."""
    import ctypes
    from tinynn_autograd_amd import _bmm_signatures as S
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    args = re.search(r"tnn_gemm_batched\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
    kinds = []
    for arg in args.split(","):
        arg = arg.strip()
        kinds.append("i64p" if "int64_t*" in arg else "p" if "*" in arg else "i64" if "int64_t" in arg else "int")
    table = {ctypes.c_void_p: "p", ctypes.c_int64: "i64", ctypes.c_int: "int", S._i64p: "i64p"}
    assert kinds == [table[t] for t in S._BMM_SIGNATURES["tnn_gemm_batched"]]
    assert "TNN_BMM_MAX_BATCH_DIMS %d" % S.MAX_BATCH_DIMS in text
    for name, value in (("AUTO", S.FORM_AUTO), ("TILE", S.FORM_TILE), ("SMALL", S.FORM_SMALL)):
        assert re.search(r"#define TNN_BMM_FORM_%s %d\b" % (name, value), text)
    from tinynn_autograd_amd import batching
    assert batching.MAX_BATCH_DIMS == S.MAX_BATCH_DIMS


def test_not_declared_in_the_main_header():
    from tinynn_autograd_amd import _lib
    assert not set(declared(HEADER)) & set(declared(MAIN_HEADER))
    assert not set(_lib._BMM_SIGNATURES) & set(_lib.EXPORTED_SYMBOLS)
    assert not set(_lib._BMM_SIGNATURES) & set(_lib._INDEX_SIGNATURES)


def test_the_test_twin_takes_the_loop_route():
    """Under the CPU test twin the batched entry point is absent: calling it says so, and `@` loops over tnn_gemm instead."""
    import numpy as np
    import tinynn_autograd_amd as tn
    from tinynn_autograd_amd import _lib
    if tn.backend_name() == "hip-gfx950":
        pytest.skip("the product library is loaded (GPU machine)")
    lib = _lib.get()
    assert not lib.has_bmm
    with pytest.raises(_lib.TnnError, match="needs libtnn_hip.so"):
        lib.gemm_batched()
    a = np.arange(24.0).reshape(2, 3, 4)
    b = np.arange(40.0).reshape(2, 4, 5)
    np.testing.assert_array_equal(np.asarray(tn.asarray(a) @ tn.asarray(b)), a @ b)
