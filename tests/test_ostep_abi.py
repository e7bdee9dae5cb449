"""The optimizer-step C-ABI (include/tnn_ostep.h): header, ctypes table, planner constants and libtnn_hip.so agree, and none of
it leaks into include/tnn_hip.h (whose every symbol the CPU test twin must export)."""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, TWIN_SO

HEADER = os.path.join(ROOT, "include", "tnn_ostep.h")
MAIN_HEADER = os.path.join(ROOT, "include", "tnn_hip.h")
LIB = os.path.join(ROOT, "tinynn-autograd_amd", "lib", "libtnn_hip.so")
SYMBOLS = ["tnn_ostep_adamw", "tnn_ostep_begin", "tnn_ostep_scale", "tnn_ostep_sumsq", "tnn_ostep_workspace"]


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
    assert syms == sorted(_lib._OSTEP_SIGNATURES) == _lib.OSTEP_SYMBOLS == SYMBOLS
    assert all(s.startswith("tnn_ostep_") for s in syms)
    assert os.path.exists(LIB), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    exp = exported(LIB)
    assert set(syms) <= exp
    assert {s for s in exp if s.startswith("tnn_ostep")} == set(syms)            # the prefix is exclusive


def test_signatures_match_the_declarations():
    """Argument count and the order of pointer / 64-bit / double / int arguments of the ctypes table follow the header."""
    from tinynn_autograd_amd import _ostep_signatures as S
    text = stripped(HEADER)
    table = {ctypes.c_void_p: "p", ctypes.c_int64: "i64", ctypes.c_int: "int", ctypes.c_double: "double"}
    for name, argtypes in S._OSTEP_SIGNATURES.items():
        args = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        kinds = []
        for arg in args.split(","):
            arg = arg.strip()
            kinds.append("p" if "*" in arg else "i64" if "int64_t" in arg else "double" if "double" in arg else "int")
        assert kinds == [table[t] for t in argtypes], name


def test_constants_agree_between_header_and_planner():
    from tinynn_autograd_amd import ostep
    text = stripped(HEADER)
    pairs = [("TNN_OSTEP_THREADS", ostep.THREADS), ("TNN_OSTEP_VEC", ostep.VEC), ("TNN_OSTEP_MAX_BLOCKS", ostep.MAX_BLOCKS),
             ("TNN_OSTEP_STATE_DOUBLES", ostep.STATE_DOUBLES), ("TNN_OSTEP_B1_POW", ostep.B1_POW),
             ("TNN_OSTEP_B2_POW", ostep.B2_POW), ("TNN_OSTEP_T", ostep.T), ("TNN_OSTEP_LR", ostep.LR),
             ("TNN_OSTEP_GNORM", ostep.GNORM), ("TNN_OSTEP_COEF", ostep.COEF), ("TNN_OSTEP_SKIPPED", ostep.SKIPPED),
             ("TNN_OSTEP_SKIP", ostep.SKIP), ("TNN_OSTEP_SCHED_CONST", ostep.SCHED_CONST),
             ("TNN_OSTEP_SCHED_COSINE", ostep.SCHED_COSINE), ("TNN_OSTEP_SCHED_LINEAR", ostep.SCHED_LINEAR)]
    for macro, value in pairs:
        found = re.search(r"#define %s (\d+)\b" % macro, text)
        assert found, macro
        assert int(found.group(1)) == value, macro
    assert len(re.findall(r"#define TNN_OSTEP_\w+ \d+", text)) == len(pairs)        # nothing in the header the planner lacks
    assert len(ostep.STATE_NAMES) == ostep.STATE_DOUBLES == len(ostep.initial_state(0.0))
    assert ostep.MAX_BLOCKS == 2048                                                 # the cap of the other streaming kernels
    kernel = open(os.path.join(ROOT, "tinynn-autograd_amd", "csrc", "tnn_ostep.hip")).read()
    assert "1e-6" in kernel and ostep.CLIP_EPS == 1e-6 and "1e-6" in open(HEADER).read()
    assert "atomic" not in re.sub(r"//.*", "", kernel).lower()                      # stream order is the only synchronisation


def test_not_declared_in_the_main_header():
    from tinynn_autograd_amd import _lib
    assert not set(declared(HEADER)) & set(declared(MAIN_HEADER))
    assert "ostep" not in open(MAIN_HEADER).read()
    for other in (_lib.EXPORTED_SYMBOLS, _lib._INDEX_SIGNATURES, _lib._BMM_SIGNATURES, _lib._CONV_SIGNATURES,
                  _lib._ATTN_SIGNATURES, _lib._NORM_SIGNATURES, _lib._TOKEN_SIGNATURES, _lib._DECODE_SIGNATURES,
                  _lib._DROPOUT_SIGNATURES):
        assert not set(_lib._OSTEP_SIGNATURES) & set(other)
        assert not [s for s in other if s.startswith("tnn_ostep")]


def test_the_test_twin_takes_the_composed_route():
    """The twin exports none of it: `has_ostep` is False, a raw call says so, and AdamW runs the composed chain with its record
    on the host."""
    import tinynn_autograd_amd as tn
    from tinynn_autograd_amd import _lib, ostep
    from tinynn_autograd_amd.core.optimizer import AdamW
    if tn.backend_name() == "hip-gfx950":
        pytest.skip("the product library is loaded (GPU machine)")
    assert not exported(TWIN_SO) & set(_lib.OSTEP_SYMBOLS)
    lib = _lib.get()
    assert not lib.has_ostep
    for call in (lib.ostep_workspace, lib.ostep_sumsq, lib.ostep_begin, lib.ostep_adamw, lib.ostep_scale):
        with pytest.raises(_lib.TnnError, match="needs libtnn_hip.so"):
            call()
    opt = AdamW(lr=1e-2, weight_decay=0.1, max_norm=1.0)
    p0 = np.linspace(-1, 1, 6)
    g = np.array([0.5, -0.25, 1.0, -2.0, 0.75, 0.125])
    p = tn.asarray(p0, dtype=np.float64)
    assert opt.apply_flat(p, tn.asarray(g, dtype=np.float64))
    assert opt.route == "composed" and opt._rec is None
    want = ostep.reference(p0, g, p0 * 0, p0 * 0, ostep.initial_state(1e-2), ostep.Hyper(lr=1e-2, wd=0.1, max_norm=1.0),
                           ostep.decay_runs([(0, 6)], [True]))
    np.testing.assert_allclose(np.asarray(p), want[0], rtol=0, atol=1e-15)
    st = opt.state()
    assert st["t"] == 1 and st["skipped"] == 0 and st["gnorm"] == pytest.approx(float(np.sqrt((g * g).sum())), rel=1e-15)
    assert opt.last_norm() == st["gnorm"] and opt.lr_now() == 1e-2
