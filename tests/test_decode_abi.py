"""The decode C-ABI (include/tnn_decode.h): header, ctypes table, planner constants and libtnn_hip.so agree, the symbols are
its own, and none of it leaks into include/tnn_hip.h (whose every symbol the CPU test twin must export)."""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, TWIN_SO

HEADER = os.path.join(ROOT, "include", "tnn_decode.h")
MAIN_HEADER = os.path.join(ROOT, "include", "tnn_hip.h")
ATTN_HEADER = os.path.join(ROOT, "include", "tnn_attn.h")
LIB = os.path.join(ROOT, "tinynn-autograd_amd", "lib", "libtnn_hip.so")
SYMBOLS = ["tnn_decode_attn", "tnn_decode_attn_workspace", "tnn_sample_rows"]
PREFIXES = ("tnn_decode_", "tnn_sample_")


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
    assert syms == sorted(_lib._DECODE_SIGNATURES) == _lib.DECODE_SYMBOLS == SYMBOLS
    assert all(s.startswith(PREFIXES) for s in syms)
    assert os.path.exists(LIB), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    exp = exported(LIB)
    assert set(syms) <= exp
    assert {s for s in exp if s.startswith(PREFIXES)} == set(syms)                        # the prefixes are exclusive


def test_signatures_match_the_declarations():
    """Argument count and the order of pointer / 64-bit / double / int arguments of the ctypes table follow the header."""
    from tinynn_autograd_amd import _decode_signatures as S
    text = stripped(HEADER)
    table = {ctypes.c_void_p: "p", ctypes.c_int64: "i64", ctypes.c_int: "int", S._i64p: "i64p", ctypes.c_double: "double"}
    for name, argtypes in S._DECODE_SIGNATURES.items():
        args = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        kinds = []
        for arg in args.split(","):
            arg = arg.strip()
            kinds.append("i64p" if "int64_t*" in arg else "p" if "*" in arg else "i64" if "int64_t" in arg
                         else "double" if "double" in arg else "int")
        assert kinds == [table[t] for t in argtypes], name


def test_constants_agree_between_header_planner_and_oracle():
    import decode_oracle as do
    from tinynn_autograd_amd import attention as at, decoding as dc
    text = stripped(HEADER)
    for macro, name in (("DECODE_VEC", "VEC"), ("DECODE_CHUNK", "CHUNK"), ("DECODE_MAX_SPLITS", "MAX_SPLITS"),
                        ("DECODE_UNROLL", "UNROLL"), ("SAMPLE_RADIX_BITS", "RADIX_BITS"), ("SAMPLE_ITEMS", "SAMPLE_ITEMS")):
        found = re.search(r"#define TNN_%s (\d+)\b" % macro, text)
        assert found, macro
        assert int(found.group(1)) == getattr(dc, name), macro
    assert (do.CHUNK, do.UNROLL, do.MAX_SPLITS) == (dc.CHUNK, dc.UNROLL, dc.MAX_SPLITS)
    head = int(re.search(r"#define TNN_ATTN_MAX_HEAD_DIM (\d+)\b", stripped(ATTN_HEADER)).group(1))
    assert head == dc.MAX_HEAD_DIM == at.MAX_HEAD_DIM
    assert 32 % dc.RADIX_BITS == 0 and dc.CHUNK == 64 and 1 <= dc.TARGET


def test_not_declared_in_the_main_header_nor_in_another_table():
    from tinynn_autograd_amd import _lib
    assert not set(declared(HEADER)) & (set(declared(MAIN_HEADER)) | set(declared(ATTN_HEADER)))
    for other in (_lib.EXPORTED_SYMBOLS, _lib._INDEX_SIGNATURES, _lib._BMM_SIGNATURES, _lib._CONV_SIGNATURES,
                  _lib._ATTN_SIGNATURES, _lib._NORM_SIGNATURES, _lib._TOKEN_SIGNATURES):
        assert not set(_lib._DECODE_SIGNATURES) & set(other)
        assert not [s for s in other if s.startswith(PREFIXES)]


def test_the_test_twin_takes_the_composed_route():
    """The twin exports none of it: `has_decode` is False, a raw call says so, and both operations run their composed form."""
    import tinynn_autograd_amd as tn
    from tinynn_autograd_amd import _lib, device_array as da
    lib = _lib.get()
    if tn.backend_name() == "hip-gfx950":
        assert lib.has_decode
        return
    assert not exported(TWIN_SO) & set(_lib.DECODE_SYMBOLS)
    assert not lib.has_decode
    for call in (lib.decode_attn, lib.decode_attn_workspace, lib.sample_rows):
        with pytest.raises(_lib.TnnError, match="needs libtnn_hip.so"):
            call()
    k = tn.asarray(np.zeros((1, 4, 1, 2), dtype=np.float32))
    v = tn.asarray(np.arange(8, dtype=np.float32).reshape(1, 4, 1, 2))
    q = tn.asarray(np.zeros((1, 1, 2), dtype=np.float32))
    o = da.attention_decode(q, k, v, 4)                        # equal scores: the mean of the four value rows
    np.testing.assert_allclose(np.asarray(o), [[[3.0, 4.0]]], rtol=1e-6)
    ids = da.sample_rows(tn.asarray(np.array([[0.0, 2.0, 1.0]], dtype=np.float32)), None, temperature=0.0)
    assert ids.dtype == np.int64 and np.asarray(ids).tolist() == [1]
    with pytest.raises(ValueError, match="native decode attention route"):
        da.attention_decode(q, k, v, 4, route="native")
    with pytest.raises(ValueError, match="native sampling route"):
        da.sample_rows(tn.asarray(np.zeros((1, 3), dtype=np.float32)), None, temperature=0.0, route="native")
