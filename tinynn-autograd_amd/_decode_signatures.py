"""Signature table of include/tnn_decode.h (decode attention over a key / value cache and token sampling of libtnn_hip.so;
tests/test_decode_abi.py holds the two together).  Kept apart from _signatures.py: the CPU test twin does not export it, and
`_lib` binds it with plain ctypes."""

from ctypes import c_double, c_int, c_int64, c_void_p, POINTER

# (the header's constants — TNN_DECODE_CHUNK and the rest — have their one Python copy in decoding.py)

_p = c_void_p
_i64 = c_int64
_i64p = POINTER(c_int64)

# name -> argtypes; every entry point returns int
_DECODE_SIGNATURES = {
    "tnn_decode_attn_workspace": [_i64, _i64, _i64, _i64, c_int, _i64p],           # B, H, splits, Dv, dtype -> bytes
    # q, k_new, v_new, k_cache, v_cache, o, workspace | workspace_bytes, B, H, len, Tmax, D, Dv | strides | scale | splits, dtype
    "tnn_decode_attn": [_p] * 7 + [_i64] * 7 + [_i64p, c_double, _i64, c_int],
    # logits, u, out_ids | M, V | temperature | top_k, dtype
    "tnn_sample_rows": [_p] * 3 + [_i64] * 2 + [c_double, _i64, c_int],
}
