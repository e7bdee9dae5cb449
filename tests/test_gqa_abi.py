"""The grouped-query C-ABI (include/tnn_gqa.h): header, ctypes table and libtnn_hip.so agree, the prefix tnn_gqa_ is its own,
none of it leaks into another header or table, and the constants of gqa.py are the header's."""

import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, TWIN_SO

HEADER = os.path.join(ROOT, "include", "tnn_gqa.h")
LIB = os.path.join(ROOT, "tinynn-autograd_amd", "lib", "libtnn_hip.so")
SYMBOLS = ["tnn_gqa_bwd_kv", "tnn_gqa_bwd_q", "tnn_gqa_decode_attn", "tnn_gqa_decode_workspace", "tnn_gqa_fwd",
           "tnn_gqa_ragged_decode_attn"]
PREFIX = "tnn_gqa_"


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
    assert syms == sorted(_lib._GQA_SIGNATURES) == _lib.GQA_SYMBOLS == SYMBOLS
    assert all(s.startswith(PREFIX) for s in syms)
    assert os.path.exists(LIB), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    exp = exported(LIB)
    assert set(syms) <= exp
    assert {s for s in exp if s.startswith(PREFIX)} == set(syms)                           # the prefix is exclusive


def test_signatures_match_the_declarations():
    """Argument count and the order of pointer / 64-bit / double / int arguments of the ctypes table follow the header."""
    from tinynn_autograd_amd import _gqa_signatures as S
    text = stripped(HEADER)
    table = {ctypes.c_void_p: "p", ctypes.c_int64: "i64", ctypes.c_int: "int", S._i64p: "i64p", ctypes.c_double: "double"}
    for name, argtypes in S._GQA_SIGNATURES.items():
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
              _lib._OSTEP_SIGNATURES, _lib._RAGGED_SIGNATURES)
    for other in others:
        assert not set(_lib._GQA_SIGNATURES) & set(other)
        assert not [s for s in other if s.startswith(PREFIX)]
    # ... and the new symbols start with no prefix that another ABI test holds closed
    closed = ("tnn_decode_", "tnn_sample_", "tnn_attn", "tnn_embed_", "tnn_xent_", "tnn_norm_", "tnn_conv", "tnn_gemm_batched",
              "tnn_dropout_", "tnn_ostep_", "tnn_index_", "tnn_ragged_")
    assert not [s for s in SYMBOLS if s.startswith(closed)]


def test_the_constants_are_the_headers():
    from tinynn_autograd_amd import gqa
    import gqa_oracle as go
    text = open(HEADER).read()
    assert int(re.search(r"#define\s+TNN_GQA_MAX_GROUP\s+(\d+)", text).group(1)) == gqa.MAX_GROUP == go.MAX_GROUP
    assert gqa.DECODE_STATES[-1] == gqa.MAX_GROUP and gqa.DECODE_STATES[0] == 1
    src = open(os.path.join(ROOT, "tinynn-autograd_amd", "csrc", "tnn_decode_kernel.h")).read()     # (launch_call: the Q dispatch)
    assert sorted(int(n) for n in re.findall(r"launch_states<T, (\d+)>", src)) == list(gqa.DECODE_STATES)


def test_the_test_twin_takes_the_composed_route():
    """The twin exports none of it: `has_gqa` is False, a raw call says so, and the operations run their composed form."""
    import tinynn_autograd_amd as tn
    from tinynn_autograd_amd import _lib, device_array as da
    lib = _lib.get()
    if tn.backend_name() == "hip-gfx950":
        assert lib.has_gqa
        return
    assert not exported(TWIN_SO) & set(_lib.GQA_SYMBOLS)
    assert not lib.has_gqa
    for name in _lib.GQA_SYMBOLS:
        with pytest.raises(_lib.TnnError, match="needs libtnn_hip.so"):
            getattr(lib, name[4:])()
    # two query heads over one key / value head, equal scores: both heads get the mean of the rows (row 3 replaced by 6, 7)
    k = tn.asarray(np.zeros((1, 4, 1, 2), dtype=np.float32))
    v = tn.asarray(np.arange(8, dtype=np.float32).reshape(1, 4, 1, 2))
    q = tn.asarray(np.zeros((1, 2, 2), dtype=np.float32))
    new = tn.asarray(np.array([[[6.0, 7.0]]], dtype=np.float32))
    o = da.gqa_decode(q, k, v, 3, tn.asarray(np.zeros((1, 1, 2), dtype=np.float32)), new)
    np.testing.assert_allclose(np.asarray(o), [[[3.0, 4.0], [3.0, 4.0]]], rtol=1e-6)
    assert np.asarray(v)[0, 3, 0].tolist() == [6.0, 7.0]
    with pytest.raises(ValueError, match="native grouped-query decode attention route"):
        da.gqa_decode(q, k, v, 3, route="native")
    with pytest.raises(ValueError, match="native grouped-query attention route"):
        da.gqa_attention(tn.asarray(np.zeros((1, 3, 2, 2), dtype=np.float32)), k, v, route="native")
