"""Signature table of include/tnn_varlen.h (training attention over a right-padded batch of libtnn_hip.so;
tests/test_varlen_abi.py holds the two together).  Kept apart from _signatures.py: the CPU test twin does not export it, and
`_lib` binds it with plain ctypes."""

from ctypes import c_double, c_int, c_int64, c_void_p, POINTER

# (the header's constants have their one Python copy in varlen.py)

_p = c_void_p
_i64 = c_int64
_i64p = POINTER(c_int64)
_geom = [_i64] * 6                                       # B, H, Tq, Tk, D, Dv
_tail = [_i64p, c_double, c_int, c_int, _p, _i64]        # strides (host array), scale, causal, dtype | lens (device), group

# name -> argtypes; every entry point returns int
_VARLEN_SIGNATURES = {
    "tnn_varlen_fwd": [_p] * 5 + _geom + _tail,          # q, k, v, o, lse
    "tnn_varlen_bwd_q": [_p] * 8 + _geom + _tail,        # q, k, v, o, do, lse, dq, delta
    "tnn_varlen_bwd_kv": [_p] * 8 + _geom + _tail,       # q, k, v, do, lse, delta, dk, dv
}
