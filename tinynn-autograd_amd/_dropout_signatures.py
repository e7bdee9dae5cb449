"""Signature table of include/tnn_dropout.h (the device random generator and dropout of libtnn_hip.so;
tests/test_dropout_abi.py holds the two together).  Kept apart from _signatures.py: the CPU test twin does not export it, and
`_lib` binds it with plain ctypes."""

from ctypes import c_double, c_int, c_int64, c_uint64, c_void_p

# (the header's constants — TNN_DROPOUT_MAX_BLOCKS and the rest — have their one Python copy in dropout.py)

_p = c_void_p
_i64 = c_int64
_u64 = c_uint64

# name -> argtypes; every entry point returns int
_DROPOUT_SIGNATURES = {
    "tnn_rng_set": [_p, _u64, _u64],                                               # state | seed, calls
    "tnn_rng_uniform": [_p, _p, _p, _i64, _i64, c_int],                            # state, ticket, out | first, n, dtype
    # state, ticket, x, residual, y | first, n, threshold, scale, dtype
    "tnn_dropout_fwd": [_p] * 5 + [_i64, _i64, c_int, c_double, c_int],
    "tnn_dropout_bwd": [_p, _p, _p, _i64, _i64, c_int, c_double, c_int],           # ticket, dy, dx | first, n, threshold, scale, dtype
}
