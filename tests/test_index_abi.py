"""The advanced-indexing C-ABI (include/tnn_index.h): header, ctypes table and libtnn_hip.so agree, and none of it leaks into
include/tnn_hip.h (whose every symbol the CPU test twin must export)."""

import os
import re
import subprocess

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "tnn_index.h")
MAIN_HEADER = os.path.join(ROOT, "include", "tnn_hip.h")
LIB = os.path.join(ROOT, "tinynn-autograd_amd", "lib", "libtnn_hip.so")


def declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"TNN_API\s+[\w\s\*]+?\b(tnn_\w+)\s*\(", text)))


def exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_header_table_and_library_agree():
    from tinynn_autograd_amd import _lib
    syms = declared(HEADER)
    assert syms == sorted(_lib._INDEX_SIGNATURES) == _lib.INDEX_SYMBOLS
    assert {"tnn_index_gather", "tnn_index_scatter", "tnn_mask_count", "tnn_mask_nonzero"} <= set(syms)
    assert os.path.exists(LIB), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    exp = exported(LIB)
    assert set(syms) <= exp
    assert {s for s in exp if s.startswith(("tnn_index_", "tnn_mask_"))} == set(syms)


def test_not_declared_in_the_main_header():
    from tinynn_autograd_amd import _lib
    assert not set(declared(HEADER)) & set(declared(MAIN_HEADER))
    assert not set(_lib._INDEX_SIGNATURES) & set(_lib.EXPORTED_SYMBOLS)


def test_descriptor_layout_matches_the_header():
    """The ctypes structure has the C struct's size: 2 int32, then 8-B fields."""
    import ctypes
    from tinynn_autograd_amd import _lib
    text = open(HEADER).read()
    assert "TNN_INDEX_MAX_DIM 6" in text and "TNN_INDEX_MAX_ARRAYS 6" in text
    assert ctypes.sizeof(_lib.IndexDesc) == 8 + 8 + 6 * 8 * 2 + 6 * 8 + 6 * 6 * 8 + 6 * 8 * 2


def test_the_test_twin_raises_on_the_new_paths():
    """Under the CPU test twin the index entry points are absent: the paths that need them say so."""
    import numpy as np
    import tinynn_autograd_amd as tn
    from tinynn_autograd_amd import _lib
    if tn.backend_name() == "hip-gfx950":
        pytest.skip("the product library is loaded (GPU machine)")
    x = tn.asarray(np.arange(12.0).reshape(3, 4))
    with pytest.raises(_lib.TnnError, match="needs libtnn_hip.so"):
        x[:, [0, 2]]
    with pytest.raises(_lib.TnnError, match="needs libtnn_hip.so"):
        np.nonzero(x > 3.0)
    np.testing.assert_array_equal(np.asarray(x[[2, 0]]), np.arange(12.0).reshape(3, 4)[[2, 0]])   # the row gather stays
