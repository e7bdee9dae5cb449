"""The rotary C-ABI (include/tnn_rope.h): header, ctypes table and libtnn_hip.so agree, the prefix tnn_rope_ is its own, none
of it leaks into another header or table, the constants of rope.py are the header's, and the CPU test twin takes the composed
route."""

import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, TWIN_SO

HEADER = os.path.join(ROOT, "include", "tnn_rope.h")
LIB = os.path.join(ROOT, "tinynn-autograd_amd", "lib", "libtnn_hip.so")
SYMBOLS = ["tnn_rope_apply"]
PREFIX = "tnn_rope_"


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
    assert syms == sorted(_lib._ROPE_SIGNATURES) == _lib.ROPE_SYMBOLS == SYMBOLS
    assert all(s.startswith(PREFIX) for s in syms)
    assert os.path.exists(LIB), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    exp = exported(LIB)
    assert set(syms) <= exp
    assert {s for s in exp if s.startswith(PREFIX)} == set(syms)                           # the prefix is exclusive


def test_signatures_match_the_declarations():
    """Argument count and the order of pointer / 64-bit / int arguments of the ctypes table follow the header."""
    from tinynn_autograd_amd import _rope_signatures as S
    text = stripped(HEADER)
    table = {ctypes.c_void_p: "p", ctypes.c_int64: "i64", ctypes.c_int: "int", S._i64p: "i64p", ctypes.c_double: "double"}
    for name, argtypes in S._ROPE_SIGNATURES.items():
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
              _lib._OSTEP_SIGNATURES, _lib._RAGGED_SIGNATURES, _lib._GQA_SIGNATURES)
    for other in others:
        assert not set(_lib._ROPE_SIGNATURES) & set(other)
        assert not [s for s in other if s.startswith(PREFIX)]
    # ... and the new symbols start with no prefix that another ABI test holds closed
    closed = ("tnn_decode_", "tnn_sample_", "tnn_attn", "tnn_embed_", "tnn_xent_", "tnn_norm_", "tnn_conv", "tnn_gemm_batched",
              "tnn_dropout_", "tnn_ostep_", "tnn_index_", "tnn_ragged_", "tnn_gqa_")
    assert not [s for s in SYMBOLS if s.startswith(closed)]
    # the CPU test twin's source exports none of it
    assert PREFIX not in open(os.path.join(ROOT, "oracle", "cpu_twin", "tnn_cpu.cpp")).read()


def test_the_constants_are_the_headers():
    from tinynn_autograd_amd import rope as rp
    text = open(HEADER).read()
    define = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))
    assert define("TNN_ROPE_VEC") == rp.VEC and define("TNN_ROPE_THREADS") == rp.THREADS
    assert define("TNN_ROPE_MAX_BLOCKS") == rp.MAX_BLOCKS
    assert define("TNN_ROPE_HALF") == rp.PAIRINGS.index("half") and define("TNN_ROPE_INTERLEAVED") == rp.PAIRINGS.index("interleaved")
    assert "tnn_rope.hip" in open(os.path.join(ROOT, "tinynn-autograd_amd", "csrc", "Makefile")).read()


def test_the_test_twin_takes_the_composed_route():
    """The twin exports none of it: `has_rope` is False, a raw call says so, and the operation runs its composed form."""
    import tinynn_autograd_amd as tn
    from tinynn_autograd_amd import _lib, device_array as da, rope as rp
    lib = _lib.get()
    if tn.backend_name() == "hip-gfx950":
        assert lib.has_rope
        return
    assert not exported(TWIN_SO) & set(_lib.ROPE_SYMBOLS)
    assert not lib.has_rope
    for name in _lib.ROPE_SYMBOLS:
        with pytest.raises(_lib.TnnError, match="needs libtnn_hip.so"):
            getattr(lib, name[4:])()
    # one pair at position 1 with base 1: the angle is 1 radian — (1, 0) turns into (cos 1, sin 1)
    rot = rp.Rotary(4, base=1.0)
    y = da.rope(tn.asarray(np.array([[[[1.0, 0.0]], [[1.0, 0.0]]]], dtype=np.float32)), rotary=rot)
    np.testing.assert_allclose(np.asarray(y)[0, :, 0], [[1.0, 0.0], [np.cos(1.0), np.sin(1.0)]], rtol=1e-6)
    with pytest.raises(ValueError, match="native rotary embedding route"):
        da.rope(tn.asarray(np.zeros((1, 1, 1, 2), dtype=np.float32)), rotary=rot, route="native")
