"""Signature table of include/tnn_lce.h (the fused linear + cross-entropy of libtnn_hip.so: the loss of a vocabulary head
without its logits, and the gradient of the logits for a run of rows).  Kept apart from _signatures.py: the CPU test twin
does not export it, and `_lib` binds it with plain ctypes."""

from ctypes import c_int, c_int64, c_void_p, POINTER

# (the constants are those of include/tnn_lce.h, whose one Python copy is in lce.py)

_p = c_void_p
_i64 = c_int64
_i64p = POINTER(c_int64)

# name -> argtypes; every entry point returns int
_LCE_SIGNATURES = {
    # M, V, splits | dtype | bytes (host)
    "tnn_lce_fwd_workspace": [_i64] * 3 + [c_int, _i64p],
    # h, ldh, w, ldw, b, targets | losses, lse, loss, count | workspace, workspace_bytes | M, K, V, splits, ignore_index |
    # reduction, dtype
    "tnn_lce_fwd": [_p, _i64, _p, _i64] + [_p] * 7 + [_i64] * 6 + [c_int, c_int],
    # h, ldh, w, ldw, b, targets, lse, count, g, dz | m0, C, M, K, V, ignore_index | reduction, dtype
    "tnn_lce_dlogits": [_p, _i64, _p, _i64] + [_p] * 6 + [_i64] * 6 + [c_int, c_int],
}
