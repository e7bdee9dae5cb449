"""Signature table of include/tnn_conv.h (2-D convolution and max pooling of libtnn_hip.so; tests/test_conv_abi.py holds the
two together).  Kept apart from _signatures.py: the CPU test twin does not export it, and `_lib` binds it with plain ctypes."""

from ctypes import c_int, c_int64, c_void_p, POINTER

FORM_AUTO, FORM_TILE, FORM_SMALL = 0, 1, 2      # TNN_CONV_FORM_*
TILE_ELEMS = 4096                               # TNN_CONV_TILE_ELEMS

_p = c_void_p
_i64 = c_int64
_i64p = POINTER(c_int64)
_geom = [_i64] * 11                              # N, C, H, W, F, KH, KW, sh, sw, ph, pw
_pool = [_i64] * 9                               # planes, H, W, KH, KW, sh, sw, ph, pw

# name -> argtypes; every entry point returns int
_CONV_SIGNATURES = {
    "tnn_conv2d_fwd": [_p, _p, _p, _p] + _geom + [c_int, c_int, c_int],
    "tnn_conv2d_bwd_data": [_p, _p, _p] + _geom + [c_int, c_int],
    "tnn_conv2d_bwd_filter": [_p, _p, _p, _p, _p, _i64] + _geom + [c_int, c_int, c_int],
    "tnn_conv2d_bwd_filter_workspace": [_i64, _i64, c_int, c_int, c_int, _i64p],
    "tnn_maxpool2d_fwd": [_p, _p, _p] + _pool + [c_int],
    "tnn_maxpool2d_bwd": [_p, _p, _p] + _pool + [c_int],
}
