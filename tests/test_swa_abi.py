"""include/tnn_swa.h: header, ctypes table and library agree, exclusive prefix, the constants of swa.py."""

import glob
import os
import re

from conftest import ROOT
from test_gated_abi import CSRC, LIB, declared, exported

HEADER = os.path.join(ROOT, "include", "tnn_swa.h")
SYMBOLS = ["tnn_swa_bwd_kv", "tnn_swa_bwd_q", "tnn_swa_decode_attn", "tnn_swa_decode_attn_workspace", "tnn_swa_fill", "tnn_swa_fwd"]
PREFIX = "tnn_swa_"


def test_header_table_and_library_agree():
    from tinynn_autograd_amd import _lib
    assert declared(HEADER) == sorted(_lib._SWA_SIGNATURES) == _lib.SWA_SYMBOLS == SYMBOLS
    assert os.path.exists(LIB), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    assert {s for s in exported(LIB) if s.startswith(PREFIX)} == set(SYMBOLS)
    assert (_lib.get().kind == 1) == _lib.get().has_swa


def test_the_prefix_lies_in_no_other_header_or_table():
    from tinynn_autograd_amd import _lib
    for path in glob.glob(os.path.join(ROOT, "include", "*.h")):
        if os.path.abspath(path) != os.path.abspath(HEADER):
            assert not [s for s in declared(path) if s.startswith(PREFIX)], path
    tables = [getattr(_lib, n) for n in dir(_lib) if n.endswith("_SIGNATURES") and n != "_SWA_SIGNATURES"]
    assert len(tables) >= 19 and not [s for t in tables for s in t if s.startswith(PREFIX)]
    assert PREFIX not in open(os.path.join(ROOT, "oracle", "cpu_twin", "tnn_cpu.cpp")).read()      # the CPU twin exports none


def test_the_constants_are_the_headers():
    from tinynn_autograd_amd import swa
    text = open(HEADER).read()
    define = lambda name: int(re.search(r"#define\s+TNN_SWA_%s\s+(\d+)" % name, text).group(1))
    assert [define(n) for n in ("BLOCK", "MAX_GROUP")] == [swa.BLOCK, swa.MAX_GROUP] == [64, 8]
    srcs = re.search(r"^SRCS\s*:=(.*)$", open(os.path.join(CSRC, "Makefile")).read(), flags=re.M).group(1).split()
    assert "tnn_swa.hip" in srcs
