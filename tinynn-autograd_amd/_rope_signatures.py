"""Signature table of include/tnn_rope.h (the rotary position embedding of libtnn_hip.so: one launch rotates up to two
tensors; tests/test_rope_abi.py holds the two together).  Kept apart from _signatures.py: the CPU test twin does not export
it, and `_lib` binds it with plain ctypes."""

from ctypes import c_int, c_int64, c_void_p, POINTER

# (the constants are those of include/tnn_rope.h, whose one Python copy is in rope.py)

_p = c_void_p
_i64 = c_int64
_i64p = POINTER(c_int64)

# name -> argtypes; every entry point returns int
_ROPE_SIGNATURES = {
    # xa, ya, xb, yb, cos_t, sin_t, positions | geometry (B, T, Ha, Hb, D, R, P), strides | offset | inverse, pairing, blocks, dtype
    "tnn_rope_apply": [_p] * 7 + [_i64p, _i64p, _i64] + [c_int] * 4,
}
