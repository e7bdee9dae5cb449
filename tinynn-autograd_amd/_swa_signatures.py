"""Signature table of include/tnn_swa.h (sliding-window causal training attention of libtnn_hip.so; tests/test_swa_abi.py
holds the two together).  Kept apart from _signatures.py: the CPU test twin does not export it, and `_lib` binds it with plain
ctypes."""

from ctypes import c_double, c_int64, c_void_p, POINTER

# (the header's constants have their one Python copy in swa.py)

_p = c_void_p
_i64 = c_int64
_i64p = POINTER(c_int64)
_geom = [_i64] * 5                                       # B, H, T, D, Dv
_tail = [_i64p, c_double, _i64, _i64]                    # strides (host array), scale, window, group

# name -> argtypes; every entry point returns int
_SWA_SIGNATURES = {
    "tnn_swa_fwd": [_p] * 5 + _geom + _tail,             # q, k, v, o, lse
    "tnn_swa_bwd_q": [_p] * 8 + _geom + _tail,           # q, k, v, o, do, lse, dq, delta
    "tnn_swa_bwd_kv": [_p] * 8 + _geom + _tail,          # q, k, v, do, lse, delta, dk, dv
    "tnn_swa_fill": [_p] * 4 + [_i64] * 6 + [_i64p, _p],                       # k, v, k_ring, v_ring | B Hkv T R D Dv | strides, lens
    "tnn_swa_decode_attn_workspace": [_i64] * 4 + [_i64p],                     # B, H, splits, Dv -> bytes
    # q, k_new, v_new, k_ring, v_ring, o, workspace | bytes, B, H, pos | lens | R, D, Dv | strides, scale, splits, group
    "tnn_swa_decode_attn": [_p] * 7 + [_i64] * 4 + [_p] + [_i64] * 3 + [_i64p, c_double, _i64, _i64],
}
