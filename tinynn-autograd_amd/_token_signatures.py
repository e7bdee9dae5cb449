"""Signature table of include/tnn_token.h (embedding and per-row cross-entropy of libtnn_hip.so; tests/test_token_abi.py holds
the two together).  Kept apart from _signatures.py: the CPU test twin does not export it, and `_lib` binds it with plain
ctypes."""

from ctypes import c_int, c_int64, c_void_p, POINTER

# (the header's constants — TNN_EMBED_SEGMENT and the rest — have their one Python copy in tokens.py)

_p = c_void_p
_i64 = c_int64
_i64p = POINTER(c_int64)

# name -> argtypes; every entry point returns int
_TOKEN_SIGNATURES = {
    "tnn_embed_fwd": [_p] * 4 + [_i64] * 4 + [c_int],                      # table, ids, pos, out | M, V, E, T, dtype
    "tnn_embed_bwd_workspace": [_i64, _i64, _i64, c_int, _i64p],           # M, V, E, dtype -> bytes
    # dy, ids, dtable, dpos, workspace | workspace_bytes, M, V, E, T, padding_idx, dtype
    "tnn_embed_bwd": [_p] * 5 + [_i64] * 6 + [c_int],
    # logits, targets, losses, lse, loss, count | M, V, ignore_index, reduction, dtype
    "tnn_xent_fwd": [_p] * 6 + [_i64] * 3 + [c_int, c_int],
    # logits, targets, lse, count, g, dlogits | M, V, ignore_index, reduction, dtype
    "tnn_xent_bwd": [_p] * 6 + [_i64] * 3 + [c_int, c_int],
}
