"""include/tnn_lce.h: header, ctypes table and library agree, argument kinds, exclusive prefix, the constants of lce.py."""

import ctypes
import glob
import os
import re

from conftest import ROOT
from test_gated_abi import CSRC, LIB, declared, exported, stripped

HEADER = os.path.join(ROOT, "include", "tnn_lce.h")
SYMBOLS = ["tnn_lce_dlogits", "tnn_lce_fwd", "tnn_lce_fwd_workspace"]
PREFIX = "tnn_lce_"


def test_header_table_and_library_agree():
    from tinynn_autograd_amd import _lib
    assert declared(HEADER) == sorted(_lib._LCE_SIGNATURES) == _lib.LCE_SYMBOLS == SYMBOLS
    assert os.path.exists(LIB), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    assert {s for s in exported(LIB) if s.startswith(PREFIX)} == set(SYMBOLS)
    assert (_lib.get().kind == 1) == _lib.get().has_lce


def test_signatures_match_the_declarations():
    from tinynn_autograd_amd import _lce_signatures as S
    text = stripped(HEADER)
    table = {ctypes.c_void_p: "p", ctypes.c_int64: "i64", ctypes.c_int: "int", S._i64p: "i64p"}
    for name, argtypes in S._LCE_SIGNATURES.items():
        args = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        kinds = ["i64p" if "int64_t*" in a else "p" if "*" in a else "i64" if "int64_t" in a else "int" for a in args.split(",")]
        assert kinds == [table[t] for t in argtypes], name
    assert [len(S._LCE_SIGNATURES[s]) for s in SYMBOLS] == [18, 19, 5]


def test_the_prefix_lies_in_no_other_header_or_table():
    from tinynn_autograd_amd import _lib
    for path in glob.glob(os.path.join(ROOT, "include", "*.h")):
        if os.path.abspath(path) != os.path.abspath(HEADER):
            assert not [s for s in declared(path) if s.startswith(PREFIX)], path
    tables = [getattr(_lib, n) for n in dir(_lib) if n.endswith("_SIGNATURES") and n != "_LCE_SIGNATURES"]
    assert len(tables) >= 18 and not [s for t in tables for s in t if s.startswith(PREFIX)]
    assert PREFIX not in open(os.path.join(ROOT, "oracle", "cpu_twin", "tnn_cpu.cpp")).read()      # the CPU twin exports none


def test_the_constants_are_the_headers():
    from tinynn_autograd_amd import lce
    text = open(HEADER).read()
    define = lambda name: int(re.search(r"#define\s+TNN_LCE_%s\s+(\d+)" % name, text).group(1))
    names = ("WAVES", "WAVE_ROWS", "BLOCK_M", "BLOCK_V", "KC", "MAX_SPLITS")
    assert [define(n) for n in names] == [getattr(lce, n) for n in names] == [4, 16, 64, 256, 16, 64]
    srcs = re.search(r"^SRCS\s*:=(.*)$", open(os.path.join(CSRC, "Makefile")).read(), flags=re.M).group(1).split()
    assert "tnn_lce.hip" in srcs
