"""TEST INFRASTRUCTURE — the float64 yardstick of the int8 weight-only linear layer (numpy only): the properties of a
quantized weight and x (code scale) + b over the codes as they are, under a derived float32 bound.

Quantized weights (include/tnn_wq.h).  scale[n] is BIT-equal to float32(absmax_k |w[k, n]|) / float32(127), |code| <= 127,
|w - code scale| <= scale / 2 elementwise in float64, and a zero column has scale 0 and codes 0.

The product.  The reference is formed in float64 over code * scale (exact: 8 x 24 bits), so the quantization is not part of
the error — only the kernel's float32 arithmetic is.  A code converts exactly; the K terms x[m, k] code[k, n] are added by
fused multiply-adds and plain adds in SOME order (lane groups, waves, splits), every operation one rounding, so the sum is
off by at most (K - 1) u sum_k |x| |code| to first order; the scale's product and the bias's sum are one rounding each.  With
the second-order terms covered by the three spare units:

    |y - y64| <= (K + 3) 2^-24 (|scale[n]| sum_k |x[m, k]| |code[k, n]| + |b[n]|)
"""

import numpy as np

from tinynn_autograd_amd import wq

U = 2.0 ** -24


def check_weight(w, codes, scales, what="weight"):
    """The properties of a quantized weight: w float32 [K, N], codes uint8 [K / 4, N, 4], scales float32 [N]."""
    w = np.asarray(w, dtype=np.float32)
    codes, s = np.asarray(codes), np.asarray(scales)
    assert codes.dtype == np.uint8 and codes.shape == wq.codes_shape(*w.shape) and s.dtype == np.float32 and s.shape == w.shape[1:]
    want = np.abs(w).max(axis=0).astype(np.float32) / np.float32(127)
    assert np.array_equal(s.view(np.uint32), want.view(np.uint32)), "%s: a scale is not float32(absmax) / float32(127)" % what
    c = wq.unpack_codes(codes).astype(np.float64)
    assert (np.abs(c) <= 127).all(), "%s: a code outside [-127, 127]" % what
    err = np.abs(w.astype(np.float64) - c * s.astype(np.float64)[None, :])
    assert (err <= s.astype(np.float64)[None, :] / 2).all(), "%s: |w - code scale| exceeds scale / 2" % what
    zero = np.abs(w).max(axis=0) == 0
    assert (s[zero] == 0).all() and (c[:, zero] == 0).all(), "%s: a zero column must have scale 0 and codes 0" % what


def linear_reference(x, codes, scales, b=None):
    """(y [M, N] float64, its elementwise bound) over the codes and scales as they are."""
    x = np.asarray(x, dtype=np.float64)
    c = wq.unpack_codes(np.asarray(codes)).astype(np.float64)
    s = np.asarray(scales, dtype=np.float32).astype(np.float64)
    bias = np.zeros_like(s) if b is None else np.asarray(b, dtype=np.float64).reshape(-1)
    want = (x @ c) * s[None, :] + bias[None, :]
    bound = (x.shape[1] + 3) * U * (np.abs(s)[None, :] * (np.abs(x) @ np.abs(c)) + np.abs(bias)[None, :])
    return want, bound
