"""Signature table of include/tnn_ostep.h (the device-resident optimizer step of libtnn_hip.so: global-norm clipping, AdamW,
learning-rate schedules; tests/test_ostep_abi.py holds the two together).  Kept apart from _signatures.py: the CPU test twin
does not export it, and `_lib` binds it with plain ctypes."""

from ctypes import c_double, c_int, c_int64, c_void_p

# (the header's constants — TNN_OSTEP_MAX_BLOCKS, the record's indices and the rest — have their one Python copy in ostep.py)

_p = c_void_p
_i64 = c_int64

# name -> argtypes; every entry point returns int
_OSTEP_SIGNATURES = {
    "tnn_ostep_workspace": [_i64, c_int, _p],                                      # n, dtype | bytes (host int64*)
    "tnn_ostep_sumsq": [_p, _i64, _p, _i64, c_int],                                # g | n | workspace | workspace_bytes, dtype
    # state, workspace | n, max_norm, guard, b1, b2, sched, base_lr, min_lr, warmup, total
    "tnn_ostep_begin": [_p, _p, _i64, c_double, c_int, c_double, c_double, c_int, c_double, c_double, _i64, _i64],
    # p, g, m, v, step_out | n | state, runs | n_runs, b1, b2, eps, wd, dtype
    "tnn_ostep_adamw": [_p] * 5 + [_i64, _p, _p, _i64] + [c_double] * 4 + [c_int],
    "tnn_ostep_scale": [_p, _i64, _p, c_int],                                      # g | n | state | dtype
}
