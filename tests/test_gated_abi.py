"""The gated-activation C-ABI (include/tnn_gated.h): header, ctypes table and libtnn_hip.so agree, the prefix tnn_gated_ is its
own, none of it leaks into another header or table, the constants of gated.py are the header's, and the CPU test twin takes
the composed route."""

import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, TWIN_SO

HEADER = os.path.join(ROOT, "include", "tnn_gated.h")
LIB = os.path.join(ROOT, "tinynn-autograd_amd", "lib", "libtnn_hip.so")
CSRC = os.path.join(ROOT, "tinynn-autograd_amd", "csrc")
SYMBOLS = ["tnn_gated_bwd", "tnn_gated_fwd"]
PREFIX = "tnn_gated_"


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
    assert syms == sorted(_lib._GATED_SIGNATURES) == _lib.GATED_SYMBOLS == SYMBOLS
    assert all(s.startswith(PREFIX) for s in syms)
    assert os.path.exists(LIB), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    exp = exported(LIB)
    assert set(syms) <= exp
    assert {s for s in exp if s.startswith(PREFIX)} == set(syms)                           # the prefix is exclusive


def test_signatures_match_the_declarations():
    """Argument count and the order of pointer / 64-bit / int arguments of the ctypes table follow the header."""
    from tinynn_autograd_amd import _gated_signatures as S
    text = stripped(HEADER)
    table = {ctypes.c_void_p: "p", ctypes.c_int64: "i64", ctypes.c_int: "int", S._i64p: "i64p", ctypes.c_double: "double"}
    for name, argtypes in S._GATED_SIGNATURES.items():
        args = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        kinds = []
        for arg in args.split(","):
            arg = arg.strip()
            kinds.append("i64p" if "int64_t*" in arg else "p" if "*" in arg else "i64" if "int64_t" in arg
                         else "double" if "double" in arg else "int")
        assert kinds == [table[t] for t in argtypes], name
    assert len(S._GATED_SIGNATURES["tnn_gated_fwd"]) == 9 and len(S._GATED_SIGNATURES["tnn_gated_bwd"]) == 11


def test_the_prefix_lies_in_no_other_header_or_table():
    from tinynn_autograd_amd import _lib
    for path in glob.glob(os.path.join(ROOT, "include", "*.h")):
        if os.path.abspath(path) != os.path.abspath(HEADER):
            assert not [s for s in declared(path) if s.startswith(PREFIX) or s in SYMBOLS], path
    others = (_lib.EXPORTED_SYMBOLS, _lib._INDEX_SIGNATURES, _lib._BMM_SIGNATURES, _lib._CONV_SIGNATURES, _lib._ATTN_SIGNATURES,
              _lib._NORM_SIGNATURES, _lib._TOKEN_SIGNATURES, _lib._DECODE_SIGNATURES, _lib._DROPOUT_SIGNATURES,
              _lib._OSTEP_SIGNATURES, _lib._RAGGED_SIGNATURES, _lib._GQA_SIGNATURES, _lib._ROPE_SIGNATURES)
    for other in others:
        assert not set(_lib._GATED_SIGNATURES) & set(other)
        assert not [s for s in other if s.startswith(PREFIX)]
    # ... and the new symbols start with no prefix that another ABI test holds closed (tnn_gelu_* stays tnn_norm.h's)
    closed = ("tnn_decode_", "tnn_sample_", "tnn_attn", "tnn_embed_", "tnn_xent_", "tnn_norm_", "tnn_gelu_", "tnn_conv",
              "tnn_gemm_batched", "tnn_dropout_", "tnn_ostep_", "tnn_index_", "tnn_ragged_", "tnn_gqa_", "tnn_rope_")
    assert not [s for s in SYMBOLS if s.startswith(closed)]
    assert {"tnn_gelu_fwd", "tnn_gelu_bwd"} <= set(_lib._NORM_SIGNATURES)
    # the CPU test twin's source exports none of it
    assert PREFIX not in open(os.path.join(ROOT, "oracle", "cpu_twin", "tnn_cpu.cpp")).read()


def test_the_constants_are_the_headers():
    from tinynn_autograd_amd import gated as gt
    text = open(HEADER).read()
    define = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))
    assert define("TNN_GATED_VEC") == gt.VEC and define("TNN_GATED_THREADS") == gt.THREADS
    assert define("TNN_GATED_MAX_BLOCKS") == gt.MAX_BLOCKS
    assert [define("TNN_GATED_SILU"), define("TNN_GATED_GELU_TANH"), define("TNN_GATED_GELU_ERF")] == \
        [gt.ACTS.index("silu"), gt.ACTS.index("gelu_tanh"), gt.ACTS.index("gelu")] == [0, 1, 2]
    srcs = re.search(r"^SRCS\s*:=(.*)$", open(os.path.join(CSRC, "Makefile")).read(), flags=re.M).group(1).split()
    assert "tnn_gated.hip" in srcs


def test_the_gelu_functions_exist_once():
    """tnn_norm.hip and tnn_gated.hip include ONE copy of the GELU value / slope functions."""
    shared = open(os.path.join(CSRC, "tnn_gelu_math.h")).read()
    assert len(re.findall(r"\bT gelu_value\(T x\)", shared)) == 1 and len(re.findall(r"\bT gelu_slope\(T x\)", shared)) == 1
    for name in ("tnn_norm.hip", "tnn_gated.hip"):
        text = open(os.path.join(CSRC, name)).read()
        assert '#include "tnn_gelu_math.h"' in text
        assert not re.search(r"\bT gelu_(value|slope)\(T x\)", text), name
        assert "gelu_value<" in text and "gelu_slope<" in text, name


def test_the_test_twin_takes_the_composed_route():
    """The twin exports none of it: `has_gated` is False, a raw call says so, and the operation runs its composed form."""
    import tinynn_autograd_amd as tn
    from tinynn_autograd_amd import _lib, device_array as da
    lib = _lib.get()
    if tn.backend_name() == "hip-gfx950":
        assert lib.has_gated
        return
    assert not exported(TWIN_SO) & set(_lib.GATED_SYMBOLS)
    assert not lib.has_gated
    for name in _lib.GATED_SYMBOLS:
        with pytest.raises(_lib.TnnError, match="needs libtnn_hip.so"):
            getattr(lib, name[4:])()
    # silu(1) * 2 = 2 / (1 + exp(-1))
    y = da.gated(tn.asarray(np.array([[1.0, 0.0]], dtype=np.float32)), tn.asarray(np.array([[2.0, 3.0]], dtype=np.float32)))
    np.testing.assert_allclose(np.asarray(y), [[2.0 / (1.0 + np.exp(-1.0)), 0.0]], rtol=1e-6)
    with pytest.raises(ValueError, match="native gated activation route"):
        da.gated(tn.asarray(np.zeros((1, 2), dtype=np.float32)), route="native")
