"""Signature table of include/tnn_extend.h (cache-extending attention of libtnn_hip.so; tests/test_extend_abi.py holds the two
together).  Kept apart from _signatures.py: the CPU test twin does not export it, and `_lib` binds it with plain ctypes."""

from ctypes import c_double, c_int, c_int64, c_void_p, POINTER

# (the header's constants have their one Python copy in extend.py)

_p = c_void_p
_i64 = c_int64
_i64p = POINTER(c_int64)

# name -> argtypes; every entry point returns int
_EXTEND_SIGNATURES = {
    # q, k_new, v_new, k_cache, v_cache, o | B, H, Hkv, T, len, Tmax, D, Dv | strides | scale | dtype
    "tnn_extend_attn": [_p] * 6 + [_i64] * 8 + [_i64p, c_double, c_int],
}
