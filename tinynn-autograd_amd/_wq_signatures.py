"""Signature table of include/tnn_wq.h (the int8 weight-only linear layer of libtnn_hip.so: the quantizer, its inverse and
the skinny product over the codes).  Kept apart from _signatures.py: the CPU test twin does not export it, and `_lib` binds
it with plain ctypes."""

from ctypes import c_int, c_int64, c_void_p, POINTER

# (the constants are those of include/tnn_wq.h, whose one Python copy is in wq.py)

_p = c_void_p
_i64 = c_int64
_i64p = POINTER(c_int64)

# name -> argtypes; every entry point returns int
_WQ_SIGNATURES = {
    # w, ldw, codes, scales | K, N | dtype
    "tnn_wq_quantize": [_p, _i64, _p, _p, _i64, _i64, c_int],
    # codes, scales, out | K, N | dtype
    "tnn_wq_dequantize": [_p] * 3 + [_i64] * 2 + [c_int],
    # M, N, splits | dtype | bytes (host)
    "tnn_wq_linear_workspace": [_i64] * 3 + [c_int, _i64p],
    # x, ldx, codes, scales, b, y, workspace | workspace_bytes | M, K, N, splits | dtype
    "tnn_wq_linear": [_p, _i64] + [_p] * 5 + [_i64] * 5 + [c_int],
}
