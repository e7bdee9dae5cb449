"""The C-ABI of attention with per-sequence lengths (include/tnn_varlen.h): header, ctypes table and libtnn_hip.so agree, the
prefix tnn_varlen_ is its own, none of it leaks into another header or table, the argument kinds follow the declarations (those
of the tnn_attn_* counterpart, then lens and group), and the CPU test twin takes the composed route."""

import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, TWIN_SO

HEADER = os.path.join(ROOT, "include", "tnn_varlen.h")
LIB = os.path.join(ROOT, "tinynn-autograd_amd", "lib", "libtnn_hip.so")
CSRC = os.path.join(ROOT, "tinynn-autograd_amd", "csrc")
SYMBOLS = ["tnn_varlen_bwd_kv", "tnn_varlen_bwd_q", "tnn_varlen_fwd"]
PREFIX = "tnn_varlen_"


def stripped(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def declared(path):
    return sorted(set(re.findall(r"TNN_API\s+[\w\s\*]+?\b(tnn_\w+)\s*\(", stripped(path))))


def exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def kinds_of(name, text):
    args = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
    kinds = []
    for arg in args.split(","):
        arg = arg.strip()
        kinds.append("i64p" if "int64_t*" in arg else "p" if "*" in arg else "i64" if "int64_t" in arg
                     else "double" if "double" in arg else "int")
    return kinds


def test_header_table_and_library_agree():
    from tinynn_autograd_amd import _lib
    syms = declared(HEADER)
    assert syms == sorted(_lib._VARLEN_SIGNATURES) == _lib.VARLEN_SYMBOLS == SYMBOLS
    assert all(s.startswith(PREFIX) for s in syms)
    assert os.path.exists(LIB), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    exp = exported(LIB)
    assert set(syms) <= exp
    assert {s for s in exp if s.startswith(PREFIX)} == set(syms)                           # the prefix is exclusive


def test_signatures_match_the_declarations():
    """Argument kinds of the ctypes table follow the header, and every entry point is its tnn_attn_* counterpart plus
    (lens, group)."""
    from tinynn_autograd_amd import _varlen_signatures as S
    text, attn = stripped(HEADER), stripped(os.path.join(ROOT, "include", "tnn_attn.h"))
    table = {ctypes.c_void_p: "p", ctypes.c_int64: "i64", ctypes.c_int: "int", S._i64p: "i64p", ctypes.c_double: "double"}
    for name, argtypes in S._VARLEN_SIGNATURES.items():
        kinds = kinds_of(name, text)
        assert kinds == [table[t] for t in argtypes], name
        assert kinds == kinds_of(name.replace("tnn_varlen_", "tnn_attn_"), attn) + ["p", "i64"], name
    assert [len(S._VARLEN_SIGNATURES[s]) for s in SYMBOLS] == [20, 20, 17]


def test_the_prefix_lies_in_no_other_header_or_table():
    from tinynn_autograd_amd import _lib
    for path in glob.glob(os.path.join(ROOT, "include", "*.h")):
        if os.path.abspath(path) != os.path.abspath(HEADER):
            assert not [s for s in declared(path) if s.startswith(PREFIX) or s in SYMBOLS], path
    others = (_lib.EXPORTED_SYMBOLS, _lib._INDEX_SIGNATURES, _lib._BMM_SIGNATURES, _lib._CONV_SIGNATURES, _lib._ATTN_SIGNATURES,
              _lib._NORM_SIGNATURES, _lib._TOKEN_SIGNATURES, _lib._DECODE_SIGNATURES, _lib._DROPOUT_SIGNATURES,
              _lib._OSTEP_SIGNATURES, _lib._RAGGED_SIGNATURES, _lib._GQA_SIGNATURES, _lib._ROPE_SIGNATURES, _lib._GATED_SIGNATURES,
              _lib._EXTEND_SIGNATURES)
    for other in others:
        assert not set(_lib._VARLEN_SIGNATURES) & set(other)
        assert not [s for s in other if s.startswith(PREFIX)]
    # ... and the new symbols start with no prefix that another ABI test holds closed: tnn_attn and tnn_gqa_ stay exclusive
    closed = ("tnn_decode_", "tnn_sample_", "tnn_attn", "tnn_embed_", "tnn_xent_", "tnn_norm_", "tnn_gelu_", "tnn_conv",
              "tnn_gemm_batched", "tnn_dropout_", "tnn_ostep_", "tnn_index_", "tnn_ragged_", "tnn_gqa_", "tnn_rope_", "tnn_gated_",
              "tnn_extend_")
    assert not [s for s in SYMBOLS if s.startswith(closed)]
    # the CPU test twin's source exports none of it
    assert PREFIX not in open(os.path.join(ROOT, "oracle", "cpu_twin", "tnn_cpu.cpp")).read()


def test_the_unit_is_built_and_holds_no_kernel_body():
    srcs = re.search(r"^SRCS\s*:=(.*)$", open(os.path.join(CSRC, "Makefile")).read(), flags=re.M).group(1).split()
    assert "tnn_varlen.hip" in srcs
    text = open(os.path.join(CSRC, "tnn_varlen.hip")).read()
    assert '#include "tnn_attn_kernel.h"' in text and "__global__" not in text
    for entry in ("launch_fwd<true, true>", "launch_bwd_q<true, true>", "launch_bwd_kv<true, true>"):
        assert entry in text
    # the other two units keep instantiating LENS = false alone
    for unit in ("tnn_attn.hip", "tnn_gqa.hip"):
        assert not re.search(r"launch_\w+<\w+, true>", open(os.path.join(CSRC, unit)).read()), unit


def test_the_test_twin_takes_the_composed_route():
    """The twin exports none of it: `has_varlen` is False, a raw call says so, and the operation runs its composed form."""
    import tinynn_autograd_amd as tn
    from tinynn_autograd_amd import _lib, device_array as da
    lib = _lib.get()
    if tn.backend_name() == "hip-gfx950":
        assert lib.has_varlen
        return
    assert not exported(TWIN_SO) & set(_lib.VARLEN_SYMBOLS)
    assert not lib.has_varlen
    with pytest.raises(_lib.TnnError, match="needs libtnn_hip.so"):
        lib.varlen_fwd()
    # D = Dv = 1, scale 1, zero queries and keys: uniform weights over the live keys; sequence 1 has two of three
    q = k = np.zeros((2, 3, 1), dtype=np.float32)
    v = np.array([[1.0, 3.0, 5.0], [2.0, 6.0, 100.0]], dtype=np.float32).reshape(2, 3, 1)
    o, lse = da.attention(q, k, v, scale=1.0, lens=da.lengths([3, 2]))
    np.testing.assert_allclose(np.asarray(o).reshape(2, 3), [[3.0, 3.0, 3.0], [4.0, 4.0, 0.0]], rtol=1e-6)
    np.testing.assert_allclose(np.asarray(lse), np.log([[3.0, 3.0, 3.0], [2.0, 2.0, 1.0]]), rtol=1e-6, atol=1e-7)
    with pytest.raises(ValueError, match="native attention route with lens="):
        da.attention(q, k, v, lens=da.lengths([3, 2]), route="native")
