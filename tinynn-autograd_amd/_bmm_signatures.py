"""Signature table of include/tnn_bmm.h (the strided-batched GEMM of libtnn_hip.so; tests/test_bmm_abi.py holds the two
together).  Kept apart from _signatures.py: the CPU test twin does not export it, and `_lib` binds it with plain ctypes."""

from ctypes import c_int, c_int64, c_void_p, POINTER

MAX_BATCH_DIMS = 4     # TNN_BMM_MAX_BATCH_DIMS
FORM_AUTO, FORM_TILE, FORM_SMALL = 0, 1, 2      # TNN_BMM_FORM_*

_p = c_void_p
_i64p = POINTER(c_int64)

# name -> argtypes; every entry point returns int
_BMM_SIGNATURES = {
    "tnn_gemm_batched": [c_int, c_int, c_int64, c_int64, c_int64, _p, c_int64, _p, c_int64, _p,
                         c_int, _i64p, _i64p, _i64p, c_int, c_int],
}
