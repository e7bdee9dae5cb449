"""Signature table of include/tnn_gated.h (the gated activations of libtnn_hip.so: SwiGLU, GEGLU and SiLU, one launch forward
and one backward; tests/test_gated_abi.py holds the two together).  Kept apart from _signatures.py: the CPU test twin does
not export it, and `_lib` binds it with plain ctypes."""

from ctypes import c_int, c_int64, c_void_p, POINTER

# (the constants are those of include/tnn_gated.h, whose one Python copy is in gated.py)

_p = c_void_p
_i64 = c_int64
_i64p = POINTER(c_int64)

# name -> argtypes; every entry point returns int
_GATED_SIGNATURES = {
    # gate, up, y | M, F | strides (ld_gate, ld_up, ld_y) | act, blocks, dtype
    "tnn_gated_fwd": [_p] * 3 + [_i64, _i64, _i64p] + [c_int] * 3,
    # gate, up, dy, dgate, dup | M, F | strides (ld_gate, ld_up, ld_dy, ld_dgate, ld_dup) | act, blocks, dtype
    "tnn_gated_bwd": [_p] * 5 + [_i64, _i64, _i64p] + [c_int] * 3,
}
