"""The normalisation C-ABI (include/tnn_norm.h): header, ctypes table, planner constants and libtnn_hip.so agree, and none of it
leaks into include/tnn_hip.h (whose every symbol the CPU test twin must export)."""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, TWIN_SO

HEADER = os.path.join(ROOT, "include", "tnn_norm.h")
MAIN_HEADER = os.path.join(ROOT, "include", "tnn_hip.h")
LIB = os.path.join(ROOT, "tinynn-autograd_amd", "lib", "libtnn_hip.so")
SYMBOLS = ["tnn_gelu_bwd", "tnn_gelu_fwd", "tnn_norm_bwd", "tnn_norm_bwd_workspace", "tnn_norm_fwd"]


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
    assert syms == sorted(_lib._NORM_SIGNATURES) == _lib.NORM_SYMBOLS == SYMBOLS
    assert all(s.startswith(("tnn_norm_", "tnn_gelu_")) for s in syms)
    assert os.path.exists(LIB), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    exp = exported(LIB)
    assert set(syms) <= exp
    assert {s for s in exp if s.startswith(("tnn_norm", "tnn_gelu"))} == set(syms)


def test_signatures_match_the_declarations():
    """Argument count and the order of pointer / 64-bit / double / int arguments of the ctypes table follow the header."""
    from tinynn_autograd_amd import _norm_signatures as S
    text = stripped(HEADER)
    table = {ctypes.c_void_p: "p", ctypes.c_int64: "i64", ctypes.c_int: "int", ctypes.c_double: "double", S._i64p: "i64p"}
    for name, argtypes in S._NORM_SIGNATURES.items():
        args = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        kinds = []
        for arg in args.split(","):
            arg = arg.strip()
            kinds.append("i64p" if "int64_t*" in arg else "p" if "*" in arg else "i64" if "int64_t" in arg
                         else "double" if "double" in arg else "int")
        assert kinds == [table[t] for t in argtypes], name


def test_constants_agree_between_header_and_planner():
    from tinynn_autograd_amd import norm as nm
    text = stripped(HEADER)
    for macro in ("WAVE_MAX_N", "BLOCK_MAX_N", "ROWS_PER_BLOCK", "VEC", "MAX_PARTIALS"):
        found = re.search(r"#define TNN_NORM_%s (\d+)\b" % macro, text)
        assert found, macro
        assert int(found.group(1)) == getattr(nm, macro), macro
    for macro, kind in (("LAYER", "layer"), ("RMS", "rms")):
        assert int(re.search(r"#define TNN_NORM_%s (\d+)\b" % macro, text).group(1)) == nm.KIND_CODE[kind]
    assert nm.WAVE_MAX_N % 64 == 0 and nm.BLOCK_MAX_N == nm.WAVE_MAX_N * nm.ROWS_PER_BLOCK


def test_not_declared_in_the_main_header():
    from tinynn_autograd_amd import _lib
    assert not set(declared(HEADER)) & set(declared(MAIN_HEADER))
    for other in (_lib.EXPORTED_SYMBOLS, _lib._INDEX_SIGNATURES, _lib._BMM_SIGNATURES, _lib._CONV_SIGNATURES,
                  _lib._ATTN_SIGNATURES):
        assert not set(_lib._NORM_SIGNATURES) & set(other)


def test_the_test_twin_takes_the_composed_route():
    """The twin exports none of it: `has_norm` is False, a raw call says so, the norms run the composed chain instead, and the
    exact GELU — which has no composed form — raises."""
    import tinynn_autograd_amd as tn
    from tinynn_autograd_amd import _lib, device_array as da
    if tn.backend_name() == "hip-gfx950":
        pytest.skip("the product library is loaded (GPU machine)")
    assert not exported(TWIN_SO) & set(_lib.NORM_SYMBOLS)
    lib = _lib.get()
    assert not lib.has_norm
    for call in (lib.norm_fwd, lib.norm_bwd, lib.norm_bwd_workspace, lib.gelu_fwd, lib.gelu_bwd):
        with pytest.raises(_lib.TnnError, match="needs libtnn_hip.so"):
            call()
    x = np.array([[1.0, 2.0, 3.0, 4.0], [5.0, 5.0, 5.0, 9.0]], dtype=np.float32)
    y, mean, rstd = da.layer_norm(tn.asarray(x), eps=0.0)
    np.testing.assert_allclose(np.asarray(mean), [2.5, 6.0], rtol=1e-6)
    np.testing.assert_allclose(np.asarray(rstd), 1.0 / x.std(axis=1), rtol=1e-6)
    np.testing.assert_allclose(np.asarray(y), (x - x.mean(1, keepdims=True)) / x.std(1, keepdims=True), rtol=1e-5, atol=1e-6)
    y, rstd = da.rms_norm(tn.asarray(x), eps=0.0)
    np.testing.assert_allclose(np.asarray(y), x / np.sqrt((x * x).mean(1, keepdims=True)), rtol=1e-6)
    with pytest.raises(ValueError, match="native normalisation route"):
        da.layer_norm(tn.asarray(x), route="native")
    np.testing.assert_allclose(np.asarray(da.gelu(tn.asarray(x), "tanh"))[0, 0], 0.8411919906082768, rtol=1e-6)
    with pytest.raises(ValueError, match="exact .erf. GELU needs the native route"):
        da.gelu(tn.asarray(x))
    with pytest.raises(ValueError, match="exact .erf. GELU needs the native route"):
        da.gelu_bwd(tn.asarray(x), tn.asarray(x), "none")
