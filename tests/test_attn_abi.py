"""The attention C-ABI (include/tnn_attn.h): header, ctypes table, planner constants and libtnn_hip.so agree, and none of it
leaks into include/tnn_hip.h (whose every symbol the CPU test twin must export)."""

import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT, TWIN_SO

HEADER = os.path.join(ROOT, "include", "tnn_attn.h")
MAIN_HEADER = os.path.join(ROOT, "include", "tnn_hip.h")
LIB = os.path.join(ROOT, "tinynn-autograd_amd", "lib", "libtnn_hip.so")


def stripped(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def declared(path):
    return sorted(set(re.findall(r"TNN_API\s+[\w\s\*]+?\b(tnn_\w+)\s*\(", stripped(path))))


def exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_header_table_and_library_agree():
    from tinynn_autograd_amd import _lib
    syms = declared(HEADER)
    assert syms == sorted(_lib._ATTN_SIGNATURES) == _lib.ATTN_SYMBOLS
    assert syms == ["tnn_attn_bwd_kv", "tnn_attn_bwd_q", "tnn_attn_fwd"]
    assert os.path.exists(LIB), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    exp = exported(LIB)
    assert set(syms) <= exp
    assert {s for s in exp if s.startswith("tnn_attn")} == set(syms)


def test_signatures_match_the_declarations():
    """Argument count and the order of pointer / 64-bit / double / int arguments of the ctypes table follow the header."""
    from tinynn_autograd_amd import _attn_signatures as S
    text = stripped(HEADER)
    table = {ctypes.c_void_p: "p", ctypes.c_int64: "i64", ctypes.c_int: "int", ctypes.c_double: "double", S._i64p: "i64p"}
    for name, argtypes in S._ATTN_SIGNATURES.items():
        args = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        kinds = []
        for arg in args.split(","):
            arg = arg.strip()
            kinds.append("i64p" if "int64_t*" in arg else "p" if "*" in arg else "i64" if "int64_t" in arg
                         else "double" if "double" in arg else "int")
        assert kinds == [table[t] for t in argtypes], name


def test_block_constants_agree_between_header_and_planner():
    from tinynn_autograd_amd import attention as at
    text = stripped(HEADER)
    for macro, name in (("MAX_HEAD_DIM", "MAX_HEAD_DIM"), ("BLOCK_Q", "BLOCK_Q"), ("WAVE_ROWS", "WAVE_ROWS"),
                        ("BLOCK_K", "BLOCK_K"), ("MFMA_K", "MFMA_K")):
        found = re.search(r"#define TNN_ATTN_%s (\d+)\b" % macro, text)
        assert found, macro
        assert int(found.group(1)) == getattr(at, name), macro
    assert at.BLOCK_Q == 4 * at.WAVE_ROWS


def test_not_declared_in_the_main_header():
    from tinynn_autograd_amd import _lib
    assert not set(declared(HEADER)) & set(declared(MAIN_HEADER))
    for other in (_lib.EXPORTED_SYMBOLS, _lib._INDEX_SIGNATURES, _lib._BMM_SIGNATURES, _lib._CONV_SIGNATURES):
        assert not set(_lib._ATTN_SIGNATURES) & set(other)


def test_the_test_twin_takes_the_composed_route():
    """The twin exports none of it: `has_attn` is False, a raw call says so, and attention runs the composed chain instead."""
    import numpy as np
    import tinynn_autograd_amd as tn
    from tinynn_autograd_amd import _lib, device_array as da
    if tn.backend_name() == "hip-gfx950":
        pytest.skip("the product library is loaded (GPU machine)")
    assert not exported(TWIN_SO) & set(_lib.ATTN_SYMBOLS)
    lib = _lib.get()
    assert not lib.has_attn
    with pytest.raises(_lib.TnnError, match="needs libtnn_hip.so"):
        lib.attn_fwd()
    q = np.zeros((1, 2, 3), dtype=np.float32)
    v = np.arange(8.0, dtype=np.float32).reshape(1, 4, 2)
    o, lse = da.attention(tn.asarray(q), tn.asarray(np.ones((1, 4, 3), dtype=np.float32)), tn.asarray(v))
    np.testing.assert_allclose(np.asarray(o), np.broadcast_to(v.mean(axis=1, keepdims=True), (1, 2, 2)), rtol=1e-6)
    np.testing.assert_allclose(np.asarray(lse), np.full((1, 2), np.log(4.0)), rtol=1e-6)
    with pytest.raises(ValueError, match="native"):
        da.attention(tn.asarray(q), tn.asarray(q), tn.asarray(q), route="native")
