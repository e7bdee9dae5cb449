"""Signature table of include/tnn_kvq.h (the int8 key / value cache of libtnn_hip.so: the quantizing fill and the decoding
step over the codes).  Kept apart from _signatures.py: the CPU test twin does not export it, and `_lib` binds it with plain
ctypes."""

from ctypes import c_double, c_int, c_int64, c_void_p, POINTER

# (the constants are those of include/tnn_kvq.h, whose one Python copy is in kvq.py)

_p = c_void_p
_i64 = c_int64
_i64p = POINTER(c_int64)

# name -> argtypes; every entry point returns int
_KVQ_SIGNATURES = {
    # k, v, k_codes, v_codes, k_scales, v_scales | B, T, Hkv, D, Dv, row0, Tmax | strides | dtype
    "tnn_kvq_quantize_rows": [_p] * 6 + [_i64] * 7 + [_i64p, c_int],
    # B, H, splits, Dv | dtype | bytes (host)
    "tnn_kvq_decode_workspace": [_i64] * 4 + [c_int, _i64p],
    # q, k_new, v_new, k_codes, v_codes, k_scales, v_scales, o, workspace | workspace_bytes | lens | B, H, Hkv, len, Tmax, D, Dv |
    # strides | scale | splits, dtype
    "tnn_kvq_decode_attn": [_p] * 9 + [_i64, _p] + [_i64] * 7 + [_i64p, c_double, _i64, c_int],
}
