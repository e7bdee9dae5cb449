"""The random-generator / dropout C-ABI (include/tnn_dropout.h): header, ctypes table, planner constants and libtnn_hip.so
agree, and none of it leaks into include/tnn_hip.h (whose every symbol the CPU test twin must export)."""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, TWIN_SO

HEADER = os.path.join(ROOT, "include", "tnn_dropout.h")
MAIN_HEADER = os.path.join(ROOT, "include", "tnn_hip.h")
LIB = os.path.join(ROOT, "tinynn-autograd_amd", "lib", "libtnn_hip.so")
SYMBOLS = ["tnn_dropout_bwd", "tnn_dropout_fwd", "tnn_rng_set", "tnn_rng_uniform"]


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
    assert syms == sorted(_lib._DROPOUT_SIGNATURES) == _lib.DROPOUT_SYMBOLS == SYMBOLS
    assert all(s.startswith(("tnn_rng_", "tnn_dropout_")) for s in syms)
    assert os.path.exists(LIB), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    exp = exported(LIB)
    assert set(syms) <= exp
    assert {s for s in exp if s.startswith(("tnn_rng", "tnn_dropout"))} == set(syms)


def test_signatures_match_the_declarations():
    """Argument count and the order of pointer / 64-bit / unsigned 64-bit / double / int arguments of the ctypes table follow
    the header."""
    from tinynn_autograd_amd import _dropout_signatures as S
    text = stripped(HEADER)
    table = {ctypes.c_void_p: "p", ctypes.c_int64: "i64", ctypes.c_uint64: "u64", ctypes.c_int: "int", ctypes.c_double: "double"}
    for name, argtypes in S._DROPOUT_SIGNATURES.items():
        args = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        kinds = []
        for arg in args.split(","):
            arg = arg.strip()
            kinds.append("p" if "*" in arg else "u64" if "uint64_t" in arg else "i64" if "int64_t" in arg
                         else "double" if "double" in arg else "int")
        assert kinds == [table[t] for t in argtypes], name


def test_constants_agree_between_header_and_planner():
    from tinynn_autograd_amd import dropout as dp
    text = stripped(HEADER)
    for macro, value in (("TNN_RNG_ROUNDS", dp.ROUNDS), ("TNN_RNG_STATE_BYTES", dp.STATE_BYTES), ("TNN_RNG_DRAW_BITS", dp.DRAW_BITS),
                         ("TNN_DROPOUT_THREADS", dp.THREADS), ("TNN_DROPOUT_VEC", dp.VEC),
                         ("TNN_DROPOUT_MAX_BLOCKS", dp.MAX_BLOCKS)):
        found = re.search(r"#define %s (\d+)\b" % macro, text)
        assert found, macro
        assert int(found.group(1)) == value, macro
    kernel = open(os.path.join(ROOT, "tinynn-autograd_amd", "csrc", "tnn_dropout.hip")).read()
    for value in (dp.MUL0, dp.MUL1, dp.KEY0, dp.KEY1):                # the generator's constants, in the kernel and the header text
        assert "0x%08X" % value in kernel and "0x%08X" % value in open(HEADER).read()


def test_not_declared_in_the_main_header():
    from tinynn_autograd_amd import _lib
    assert not set(declared(HEADER)) & set(declared(MAIN_HEADER))
    for other in (_lib.EXPORTED_SYMBOLS, _lib._INDEX_SIGNATURES, _lib._BMM_SIGNATURES, _lib._CONV_SIGNATURES,
                  _lib._ATTN_SIGNATURES, _lib._NORM_SIGNATURES, _lib._TOKEN_SIGNATURES, _lib._DECODE_SIGNATURES):
        assert not set(_lib._DROPOUT_SIGNATURES) & set(other)


def test_the_test_twin_takes_the_composed_route():
    """The twin exports none of it: `has_dropout` is False, a raw call says so, the generator keeps its state on the host and
    dropout runs the composed chain with the planner's mask."""
    import tinynn_autograd_amd as tn
    from tinynn_autograd_amd import _lib, device_array as da, dropout as dp, rng
    if tn.backend_name() == "hip-gfx950":
        pytest.skip("the product library is loaded (GPU machine)")
    assert not exported(TWIN_SO) & set(_lib.DROPOUT_SYMBOLS)
    lib = _lib.get()
    assert not lib.has_dropout
    for call in (lib.rng_set, lib.rng_uniform, lib.dropout_fwd, lib.dropout_bwd):
        with pytest.raises(_lib.TnnError, match="needs libtnn_hip.so"):
            call()
    g = rng.Generator(5)
    assert not g.native() and g._dev is None
    x = np.arange(1, 13, dtype=np.float32).reshape(3, 4)
    y, mask = da.dropout(tn.asarray(x), 0.5, generator=g)
    assert mask.ticket is None and g._dev is None and g.state() == (5, 1)
    np.testing.assert_array_equal(np.asarray(y), dp.reference(x, 5, 0, 0.5))
    with pytest.raises(ValueError, match="native dropout route"):
        da.dropout(tn.asarray(x), 0.5, generator=g, route="native")
    np.testing.assert_array_equal(np.asarray(g.uniform((5,))), dp.uniform(5, 1, 0, 5))
    assert g.state() == (5, 2)
