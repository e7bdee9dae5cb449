"""The token C-ABI (include/tnn_token.h): header, ctypes table, planner constants and libtnn_hip.so agree, the symbol prefixes
are its own, and none of it leaks into include/tnn_hip.h (whose every symbol the CPU test twin must export)."""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, TWIN_SO

HEADER = os.path.join(ROOT, "include", "tnn_token.h")
MAIN_HEADER = os.path.join(ROOT, "include", "tnn_hip.h")
LIB = os.path.join(ROOT, "tinynn-autograd_amd", "lib", "libtnn_hip.so")
SYMBOLS = ["tnn_embed_bwd", "tnn_embed_bwd_workspace", "tnn_embed_fwd", "tnn_xent_bwd", "tnn_xent_fwd"]
PREFIXES = ("tnn_embed_", "tnn_xent_")


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
    assert syms == sorted(_lib._TOKEN_SIGNATURES) == _lib.TOKEN_SYMBOLS == SYMBOLS
    assert all(s.startswith(PREFIXES) for s in syms)
    assert os.path.exists(LIB), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    exp = exported(LIB)
    assert set(syms) <= exp
    assert {s for s in exp if s.startswith(("tnn_embed", "tnn_xent"))} == set(syms)       # the prefixes are exclusive


def test_signatures_match_the_declarations():
    """Argument count and the order of pointer / 64-bit / int arguments of the ctypes table follow the header."""
    from tinynn_autograd_amd import _token_signatures as S
    text = stripped(HEADER)
    table = {ctypes.c_void_p: "p", ctypes.c_int64: "i64", ctypes.c_int: "int", S._i64p: "i64p"}
    for name, argtypes in S._TOKEN_SIGNATURES.items():
        args = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        kinds = []
        for arg in args.split(","):
            arg = arg.strip()
            kinds.append("i64p" if "int64_t*" in arg else "p" if "*" in arg else "i64" if "int64_t" in arg else "int")
        assert kinds == [table[t] for t in argtypes], name


def test_constants_agree_between_header_and_planner():
    from tinynn_autograd_amd import tokens as tk
    text = stripped(HEADER)
    for macro, name in (("TOKEN_VEC", "VEC"), ("EMBED_SEGMENT", "EMBED_SEGMENT"), ("EMBED_VOCAB_PER_BLOCK", "EMBED_VOCAB_PER_BLOCK"),
                        ("EMBED_WALK_CHUNK", "EMBED_WALK_CHUNK"), ("XENT_WAVE_MAX_V", "XENT_WAVE_MAX_V"),
                        ("XENT_ROWS_PER_BLOCK", "XENT_ROWS_PER_BLOCK"), ("XENT_BLOCK_STEP", "XENT_BLOCK_STEP")):
        found = re.search(r"#define TNN_%s (\d+)\b" % macro, text)
        assert found, macro
        assert int(found.group(1)) == getattr(tk, name), macro
    for macro, kind in (("MEAN", "mean"), ("SUM", "sum")):
        assert int(re.search(r"#define TNN_XENT_%s (\d+)\b" % macro, text).group(1)) == tk.REDUCTION_CODE[kind]
    assert tk.XENT_WAVE_MAX_V % 64 == 0 and tk.XENT_BLOCK_STEP % (64 * tk.XENT_ROWS_PER_BLOCK) == 0


def test_not_declared_in_the_main_header_nor_in_another_table():
    from tinynn_autograd_amd import _lib
    assert not set(declared(HEADER)) & set(declared(MAIN_HEADER))
    for other in (_lib.EXPORTED_SYMBOLS, _lib._INDEX_SIGNATURES, _lib._BMM_SIGNATURES, _lib._CONV_SIGNATURES,
                  _lib._ATTN_SIGNATURES, _lib._NORM_SIGNATURES):
        assert not set(_lib._TOKEN_SIGNATURES) & set(other)
        assert not [s for s in other if s.startswith(PREFIXES)]


def test_the_test_twin_takes_the_composed_route():
    """The twin exports none of it: `has_token` is False, a raw call says so, and both ends run the composed chain."""
    import tinynn_autograd_amd as tn
    from tinynn_autograd_amd import _lib, device_array as da
    lib = _lib.get()
    if tn.backend_name() == "hip-gfx950":
        assert lib.has_token
        return
    assert not exported(TWIN_SO) & set(_lib.TOKEN_SYMBOLS)
    assert not lib.has_token
    for call in (lib.embed_fwd, lib.embed_bwd, lib.embed_bwd_workspace, lib.xent_fwd, lib.xent_bwd):
        with pytest.raises(_lib.TnnError, match="needs libtnn_hip.so"):
            call()
    table = np.arange(12, dtype=np.float32).reshape(4, 3)
    np.testing.assert_array_equal(np.asarray(da.embedding(tn.asarray(table), [3, 1, 3])), table[[3, 1, 3]])
    loss, losses, lse, count = da.cross_entropy(tn.asarray(np.zeros((2, 4), dtype=np.float32)), [0, 3])
    np.testing.assert_allclose(np.asarray(lse), np.log(4.0) * np.ones(2), rtol=1e-6)
    assert float(count) == 2.0 and abs(float(loss) - np.log(4.0)) < 1e-6
    with pytest.raises(ValueError, match="native embedding route"):
        da.embedding(tn.asarray(table), [0], route="native")
    with pytest.raises(ValueError, match="native cross-entropy route"):
        da.cross_entropy(tn.asarray(table), [0, 1, 2, 0], route="native")
