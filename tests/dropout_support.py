"""TEST INFRASTRUCTURE shared by tests/test_dropout_host.py (CPU twin) and tests/test_gpu_dropout.py (MI355X): operands at
chosen alignments, bit views, and a counter of native calls."""

import numpy as np

import tinynn_autograd_amd as tn
from tinynn_autograd_amd import _lib

UINT = {np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64}


def bits(a):
    """The array's bit patterns (so that +0 and -0, and NaN payloads, count)."""
    a = np.ascontiguousarray(np.asarray(a))
    return a.view(UINT[a.dtype])


def dev(a, dtype, unaligned=False):
    """The array on the device in `dtype`; unaligned: at an address that is only element-aligned (one element past a
    16-byte boundary)."""
    a = np.ascontiguousarray(a, dtype=dtype)
    if not unaligned:
        return tn.asarray(a, dtype=dtype)
    buf = tn.empty((a.size + 1,), dtype)
    view = buf[1:].reshape(a.shape)
    view[...] = tn.asarray(a, dtype=dtype)
    return view


def values(n, dtype, seed=0):
    """n finite, non-zero numbers of both signs (so a result of +0 can only be a dropped element)."""
    rs = np.random.RandomState(seed)
    v = rs.standard_normal(n) + np.where(rs.rand(n) < 0.5, -3.0, 3.0)
    return v.astype(dtype)


def count_calls(monkeypatch):
    """Wrap every bound entry point of the loaded library that launches or copies; returns the list the names of the calls
    are appended to."""
    lib, seen = _lib.get(), []
    tables = [_lib._SIGNATURES, _lib._INDEX_SIGNATURES, _lib._BMM_SIGNATURES, _lib._CONV_SIGNATURES, _lib._ATTN_SIGNATURES,
              _lib._NORM_SIGNATURES, _lib._TOKEN_SIGNATURES, _lib._DECODE_SIGNATURES, _lib._DROPOUT_SIGNATURES,
              _lib._GQA_SIGNATURES, _lib._RAGGED_SIGNATURES, _lib._OSTEP_SIGNATURES]
    quiet = {"malloc", "free", "last_error", "pool_stats", "stream_sync", "backend_kind"}
    for table in tables:
        for name in table:
            short = name[4:]
            if short in quiet or not hasattr(lib, short):
                continue
            real = getattr(lib, short)

            def call(*args, _real=real, _short=short):
                seen.append(_short)
                return _real(*args)
            monkeypatch.setattr(lib, short, call)
    return seen
