"""Signature table of include/tnn_norm.h (layer norm, RMS norm and GELU of libtnn_hip.so; tests/test_norm_abi.py holds the
two together).  Kept apart from _signatures.py: the CPU test twin does not export it, and `_lib` binds it with plain
ctypes."""

from ctypes import c_double, c_int, c_int64, c_void_p, POINTER

# (the header's constants — TNN_NORM_WAVE_MAX_N and the rest — have their one Python copy in norm.py)

_p = c_void_p
_i64 = c_int64
_i64p = POINTER(c_int64)

# name -> argtypes; every entry point returns int
_NORM_SIGNATURES = {
    "tnn_norm_fwd": [_p] * 6 + [_i64, _i64, c_double, c_int, c_int],       # x, gamma, beta, y, mean, rstd | M, N, eps, kind, dtype
    "tnn_norm_bwd_workspace": [_i64, _i64, c_int, c_int, c_int, _i64p],    # M, N, with_dgamma, with_dbeta, dtype -> bytes
    # x, dy, gamma, mean, rstd, dx, dgamma, dbeta, workspace | workspace_bytes, M, N, kind, dtype
    "tnn_norm_bwd": [_p] * 9 + [_i64, _i64, _i64, c_int, c_int],
    "tnn_gelu_fwd": [_p, _p, _i64, c_int, c_int],                          # x, y | n, approx, dtype
    "tnn_gelu_bwd": [_p, _p, _p, _i64, c_int, c_int],                      # x, dy, dx | n, approx, dtype
}
