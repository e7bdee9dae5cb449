"""The cache-extending attention C-ABI (include/tnn_extend.h): header, ctypes table and libtnn_hip.so agree, the prefix
tnn_extend_ is its own, none of it leaks into another header or table, the constants of extend.py are the header's, and the
CPU test twin takes the composed route."""

import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, TWIN_SO

HEADER = os.path.join(ROOT, "include", "tnn_extend.h")
LIB = os.path.join(ROOT, "tinynn-autograd_amd", "lib", "libtnn_hip.so")
CSRC = os.path.join(ROOT, "tinynn-autograd_amd", "csrc")
SYMBOLS = ["tnn_extend_attn"]
PREFIX = "tnn_extend_"


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
    assert syms == sorted(_lib._EXTEND_SIGNATURES) == _lib.EXTEND_SYMBOLS == SYMBOLS
    assert all(s.startswith(PREFIX) for s in syms)
    assert os.path.exists(LIB), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    exp = exported(LIB)
    assert set(syms) <= exp
    assert {s for s in exp if s.startswith(PREFIX)} == set(syms)                           # the prefix is exclusive


def test_signatures_match_the_declarations():
    """Argument count and the order of pointer / 64-bit / int arguments of the ctypes table follow the header."""
    from tinynn_autograd_amd import _extend_signatures as S
    text = stripped(HEADER)
    table = {ctypes.c_void_p: "p", ctypes.c_int64: "i64", ctypes.c_int: "int", S._i64p: "i64p", ctypes.c_double: "double"}
    for name, argtypes in S._EXTEND_SIGNATURES.items():
        args = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        kinds = []
        for arg in args.split(","):
            arg = arg.strip()
            kinds.append("i64p" if "int64_t*" in arg else "p" if "*" in arg else "i64" if "int64_t" in arg
                         else "double" if "double" in arg else "int")
        assert kinds == [table[t] for t in argtypes], name
    assert len(S._EXTEND_SIGNATURES["tnn_extend_attn"]) == 17


def test_the_prefix_lies_in_no_other_header_or_table():
    from tinynn_autograd_amd import _lib
    for path in glob.glob(os.path.join(ROOT, "include", "*.h")):
        if os.path.abspath(path) != os.path.abspath(HEADER):
            assert not [s for s in declared(path) if s.startswith(PREFIX) or s in SYMBOLS], path
    others = (_lib.EXPORTED_SYMBOLS, _lib._INDEX_SIGNATURES, _lib._BMM_SIGNATURES, _lib._CONV_SIGNATURES, _lib._ATTN_SIGNATURES,
              _lib._NORM_SIGNATURES, _lib._TOKEN_SIGNATURES, _lib._DECODE_SIGNATURES, _lib._DROPOUT_SIGNATURES,
              _lib._OSTEP_SIGNATURES, _lib._RAGGED_SIGNATURES, _lib._GQA_SIGNATURES, _lib._ROPE_SIGNATURES, _lib._GATED_SIGNATURES)
    for other in others:
        assert not set(_lib._EXTEND_SIGNATURES) & set(other)
        assert not [s for s in other if s.startswith(PREFIX)]
    # ... and the new symbol starts with no prefix that another ABI test holds closed (the list of tests/test_gated_abi.py,
    # and that test's own prefix)
    closed = ("tnn_decode_", "tnn_sample_", "tnn_attn", "tnn_embed_", "tnn_xent_", "tnn_norm_", "tnn_gelu_", "tnn_conv",
              "tnn_gemm_batched", "tnn_dropout_", "tnn_ostep_", "tnn_index_", "tnn_ragged_", "tnn_gqa_", "tnn_rope_", "tnn_gated_")
    assert not [s for s in SYMBOLS if s.startswith(closed)]
    # the CPU test twin's source exports none of it
    assert PREFIX not in open(os.path.join(ROOT, "oracle", "cpu_twin", "tnn_cpu.cpp")).read()


def test_the_constants_are_the_headers():
    from tinynn_autograd_amd import extend as ex
    define = lambda name, text: int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))
    own, attn = open(HEADER).read(), open(os.path.join(ROOT, "include", "tnn_attn.h")).read()
    assert define("TNN_EXTEND_BLOCK_K", own) == ex.BLOCK_K == define("TNN_ATTN_BLOCK_K", attn)
    assert define("TNN_ATTN_BLOCK_Q", attn) == ex.BLOCK_Q and define("TNN_ATTN_WAVE_ROWS", attn) == ex.WAVE_ROWS
    assert define("TNN_ATTN_MAX_HEAD_DIM", attn) == ex.MAX_HEAD_DIM and ex.LIMIT == 1 << 31
    srcs = re.search(r"^SRCS\s*:=(.*)$", open(os.path.join(CSRC, "Makefile")).read(), flags=re.M).group(1).split()
    assert "tnn_extend.hip" in srcs


def test_the_kernels_of_tnn_attn_are_used_by_inclusion():
    """tnn_extend.hip includes tnn_attn_kernel.h for the device pieces and defines none of them again."""
    text = open(os.path.join(CSRC, "tnn_extend.hip")).read()
    assert '#include "tnn_attn_kernel.h"' in text
    for piece in ("load_rows", "stage_tile", "rows_times_regs", "cols_times_acc", "store_rows", "group_max", "group_sum"):
        assert re.search(r"\b%s\b" % piece, text), piece
        assert not re.search(r"void\s+%s\s*\(|float\s+%s\s*\(" % (piece, piece), text), piece


def test_the_test_twin_takes_the_composed_route():
    """The twin exports none of it: `has_extend` is False, a raw call says so, and the operation runs its composed form."""
    import tinynn_autograd_amd as tn
    from tinynn_autograd_amd import _lib, device_array as da
    lib = _lib.get()
    if tn.backend_name() == "hip-gfx950":
        assert lib.has_extend
        return
    assert not exported(TWIN_SO) & set(_lib.EXTEND_SYMBOLS)
    assert not lib.has_extend
    with pytest.raises(_lib.TnnError, match="needs libtnn_hip.so"):
        lib.extend_attn()
    # one head, D = Dv = 1, scale 1, one cached row (k 0, v 1) and two new rows (k 0, v 3 and 5): uniform weights
    kc, vc = tn.asarray(np.zeros((1, 3, 1, 1), dtype=np.float32)), tn.asarray(np.ones((1, 3, 1, 1), dtype=np.float32))
    q = kn = np.zeros((1, 2, 1, 1), dtype=np.float32)
    vn = np.array([3.0, 5.0], dtype=np.float32).reshape(1, 2, 1, 1)
    o = da.attention_extend(q, kc, vc, 1, kn, vn, scale=1.0)
    np.testing.assert_allclose(np.asarray(o).ravel(), [2.0, 3.0], rtol=1e-6)
    assert np.asarray(vc).ravel().tolist() == [1.0, 3.0, 5.0]
    with pytest.raises(ValueError, match="native attention_extend route"):
        da.attention_extend(q, kc, vc, 0, kn, vn, route="native")
