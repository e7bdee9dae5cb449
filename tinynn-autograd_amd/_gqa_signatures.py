"""Signature table of include/tnn_gqa.h (grouped-query attention of libtnn_hip.so: the training kernels and the decode step
with H query heads over Hkv key / value heads; tests/test_gqa_abi.py holds the two together).  Kept apart from
_signatures.py: the CPU test twin does not export it, and `_lib` binds it with plain ctypes."""

from ctypes import c_double, c_int, c_int64, c_void_p, POINTER

# (the constants are those of include/tnn_gqa.h, whose one Python copy is in gqa.py)

_p = c_void_p
_i64 = c_int64
_i64p = POINTER(c_int64)

# name -> argtypes; every entry point returns int
_GQA_SIGNATURES = {
    # q, k, v, o, lse | B, H, Hkv, Tq, Tk, D, Dv | strides | scale | causal, dtype
    "tnn_gqa_fwd": [_p] * 5 + [_i64] * 7 + [_i64p, c_double, c_int, c_int],
    # q, k, v, o, do, lse, dq, delta | B, H, Hkv, Tq, Tk, D, Dv | strides | scale | causal, dtype
    "tnn_gqa_bwd_q": [_p] * 8 + [_i64] * 7 + [_i64p, c_double, c_int, c_int],
    # q, k, v, do, lse, delta, dk, dv | B, H, Hkv, Tq, Tk, D, Dv | strides | scale | causal, dtype
    "tnn_gqa_bwd_kv": [_p] * 8 + [_i64] * 7 + [_i64p, c_double, c_int, c_int],
    # B, H, splits, Dv | dtype | bytes (host)
    "tnn_gqa_decode_workspace": [_i64] * 4 + [c_int, _i64p],
    # q, k_new, v_new, k_cache, v_cache, o, workspace | workspace_bytes, B, H, Hkv, len, Tmax, D, Dv | strides | scale | splits, dtype
    "tnn_gqa_decode_attn": [_p] * 7 + [_i64] * 8 + [_i64p, c_double, _i64, c_int],
    # q, k_new, v_new, k_cache, v_cache, o, workspace | workspace_bytes | lens | B, H, Hkv, Tmax, D, Dv | strides | scale | splits, dtype
    "tnn_gqa_ragged_decode_attn": [_p] * 7 + [_i64, _p] + [_i64] * 6 + [_i64p, c_double, _i64, c_int],
}
