"""Signature table of include/tnn_index.h (the advanced-indexing entry points of libtnn_hip.so; tests/test_index_abi.py holds
the two together).  Kept apart from _signatures.py: the CPU test twin does not export these, and `_lib` binds them with plain
ctypes (no compiled call wrappers)."""

import ctypes
from ctypes import c_int, c_int32, c_int64, c_void_p, POINTER

MAX_DIM = 6        # TNN_INDEX_MAX_DIM
MAX_ARRAYS = 6     # TNN_INDEX_MAX_ARRAYS


class IndexDesc(ctypes.Structure):
    """struct tnn_index_desc"""
    _fields_ = [("ndim", c_int32), ("narr", c_int32), ("base", c_int64),
                ("shape", c_int64 * MAX_DIM), ("stride", c_int64 * MAX_DIM),
                ("idx", c_void_p * MAX_ARRAYS),
                ("istride", (c_int64 * MAX_DIM) * MAX_ARRAYS),
                ("astride", c_int64 * MAX_ARRAYS), ("alen", c_int64 * MAX_ARRAYS)]


_p = c_void_p
_i64p = POINTER(c_int64)

# name -> argtypes; every entry point returns int
_INDEX_SIGNATURES = {
    "tnn_index_gather": [_p, _p, POINTER(IndexDesc), c_int],
    "tnn_index_scatter": [_p, _i64p, _p, POINTER(IndexDesc), c_int, _p, c_int],
    "tnn_mask_scratch_elems": [c_int64, _i64p],
    "tnn_mask_count": [_p, c_int64, _p],
    "tnn_mask_nonzero": [_p, c_int64, _p, c_int, _i64p, _p, c_int64],
}
