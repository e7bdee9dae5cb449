"""Signature table of include/tnn_ragged.h (the ragged decoding step of libtnn_hip.so: decode attention with per-sequence
lengths on the device, the step's bookkeeping, the embedding with a position per row; tests/test_ragged_abi.py holds the two
together).  Kept apart from _signatures.py: the CPU test twin does not export it, and `_lib` binds it with plain ctypes."""

from ctypes import c_double, c_int, c_int64, c_void_p, POINTER

# (the constants are those of include/tnn_decode.h, whose one Python copy is in decoding.py)

_p = c_void_p
_i64 = c_int64
_i64p = POINTER(c_int64)

# name -> argtypes; every entry point returns int
_RAGGED_SIGNATURES = {
    # q, k_new, v_new, k_cache, v_cache, o, workspace | workspace_bytes | lens | B, H, Tmax, D, Dv | strides | scale | splits, dtype
    "tnn_ragged_decode_attn": [_p] * 7 + [_i64, _p] + [_i64] * 5 + [_i64p, c_double, _i64, c_int],
    # picked, lens, start, done, out, cur, u_all, u_cur | B, Tout, N, eos, pad | dtype
    "tnn_ragged_advance": [_p] * 8 + [_i64] * 5 + [c_int],
    # table, ids, pos, positions, out | M, V, E, Tpos | dtype
    "tnn_ragged_embed_fwd": [_p] * 5 + [_i64] * 4 + [c_int],
}
