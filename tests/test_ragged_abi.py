"""The ragged-step C-ABI (include/tnn_ragged.h): header, ctypes table and libtnn_hip.so agree, the prefix tnn_ragged_ is its
own, and none of it leaks into another header or table (include/tnn_hip.h least of all: the CPU test twin must export every
symbol of that one)."""

import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, TWIN_SO

HEADER = os.path.join(ROOT, "include", "tnn_ragged.h")
LIB = os.path.join(ROOT, "tinynn-autograd_amd", "lib", "libtnn_hip.so")
SYMBOLS = ["tnn_ragged_advance", "tnn_ragged_decode_attn", "tnn_ragged_embed_fwd"]
PREFIX = "tnn_ragged_"


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
    assert syms == sorted(_lib._RAGGED_SIGNATURES) == _lib.RAGGED_SYMBOLS == SYMBOLS
    assert all(s.startswith(PREFIX) for s in syms)
    assert os.path.exists(LIB), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    exp = exported(LIB)
    assert set(syms) <= exp
    assert {s for s in exp if s.startswith(PREFIX)} == set(syms)                           # the prefix is exclusive


def test_signatures_match_the_declarations():
    """Argument count and the order of pointer / 64-bit / double / int arguments of the ctypes table follow the header."""
    from tinynn_autograd_amd import _ragged_signatures as S
    text = stripped(HEADER)
    table = {ctypes.c_void_p: "p", ctypes.c_int64: "i64", ctypes.c_int: "int", S._i64p: "i64p", ctypes.c_double: "double"}
    for name, argtypes in S._RAGGED_SIGNATURES.items():
        args = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        kinds = []
        for arg in args.split(","):
            arg = arg.strip()
            kinds.append("i64p" if "int64_t*" in arg else "p" if "*" in arg else "i64" if "int64_t" in arg
                         else "double" if "double" in arg else "int")
        assert kinds == [table[t] for t in argtypes], name


def test_the_prefix_lies_in_no_other_header_or_table():
    from tinynn_autograd_amd import _lib
    for path in glob.glob(os.path.join(ROOT, "include", "*.h")):
        if os.path.abspath(path) != os.path.abspath(HEADER):
            assert not [s for s in declared(path) if s.startswith(PREFIX) or s in SYMBOLS], path
    others = (_lib.EXPORTED_SYMBOLS, _lib._INDEX_SIGNATURES, _lib._BMM_SIGNATURES, _lib._CONV_SIGNATURES, _lib._ATTN_SIGNATURES,
              _lib._NORM_SIGNATURES, _lib._TOKEN_SIGNATURES, _lib._DECODE_SIGNATURES, _lib._DROPOUT_SIGNATURES,
              _lib._OSTEP_SIGNATURES)
    for other in others:
        assert not set(_lib._RAGGED_SIGNATURES) & set(other)
        assert not [s for s in other if s.startswith(PREFIX)]
    # ... and the new symbols start with no prefix that another ABI test holds closed
    closed = ("tnn_decode_", "tnn_sample_", "tnn_attn", "tnn_embed_", "tnn_xent_", "tnn_norm_", "tnn_conv", "tnn_gemm_batched",
              "tnn_dropout_", "tnn_ostep_", "tnn_index_")
    assert not [s for s in SYMBOLS if s.startswith(closed)]


def test_the_test_twin_takes_the_composed_route():
    """The twin exports none of it: `has_ragged` is False, a raw call says so, and the three operations run their composed form."""
    import tinynn_autograd_amd as tn
    from tinynn_autograd_amd import _lib, device_array as da
    lib = _lib.get()
    if tn.backend_name() == "hip-gfx950":
        assert lib.has_ragged
        return
    assert not exported(TWIN_SO) & set(_lib.RAGGED_SYMBOLS)
    assert not lib.has_ragged
    for call in (lib.ragged_decode_attn, lib.ragged_advance, lib.ragged_embed_fwd):
        with pytest.raises(_lib.TnnError, match="needs libtnn_hip.so"):
            call()
    k = tn.asarray(np.zeros((2, 4, 1, 2), dtype=np.float32))
    v = tn.asarray(np.arange(16, dtype=np.float32).reshape(2, 4, 1, 2))
    q = tn.asarray(np.zeros((2, 1, 2), dtype=np.float32))
    new = tn.asarray(np.array([[[6.0, 7.0]], [[20.0, 21.0]]], dtype=np.float32))
    o = da.attention_decode_ragged(q, k, v, da.lengths([3, 1]), tn.asarray(np.zeros((2, 1, 2), dtype=np.float32)), new)
    # equal scores: the mean of rows 0..3 (row 3 replaced by 6, 7) and of rows 0..1 (row 1 replaced by 20, 21)
    np.testing.assert_allclose(np.asarray(o), [[[3.0, 4.0]], [[14.0, 15.0]]], rtol=1e-6)
    table, pos = tn.asarray(np.arange(6, dtype=np.float32).reshape(3, 2)), tn.asarray(10 * np.arange(8, dtype=np.float32).reshape(4, 2))
    e = da.embedding_at(table, tn.asarray(np.array([2, 0])), da.lengths([1, 3]), pos)
    assert np.asarray(e).tolist() == [[24.0, 35.0], [60.0, 71.0]]
    with pytest.raises(ValueError, match="native ragged decode attention route"):
        da.attention_decode_ragged(q, k, v, da.lengths([3, 1]), q, new, route="native")
    with pytest.raises(ValueError, match="native embedding_at route"):
        da.embedding_at(table, tn.asarray(np.array([2, 0])), da.lengths([1, 3]), pos, route="native")
