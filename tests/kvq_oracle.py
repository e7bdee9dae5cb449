"""TEST INFRASTRUCTURE — the float64 yardstick of the int8 key / value cache (numpy only): the properties of a quantized row
and decode attention over DEQUANTIZED codes under a derived float32 bound.

Quantized rows (include/tnn_kvq.h).  scale is float32 absmax / 127 to within one ulp, |code| <= 127,
|x - code scale| <= scale (0.5 + 2^-20) elementwise in float64, and a zero row has scale 0 and codes 0.

Decode attention.  The reference is softmax(scale q k^^T) v^ in float64 over k^ = code scale and v^ = code scale formed in
float64 (exact: 8 x 24 bits), so quantization rounding is not part of the error — only the kernel's float32 arithmetic is.
The bound is decode_oracle's on those operands with R, the number of rescaling factors a contribution meets, counted for
THIS kernel, plus the term of its dequantize sequence:

    R = ceil(run / (UNROLL * 16)) + 1 + 6 + 1 + 1      run = the keys of the longest split's run of chunks of CHUNK
        the loop's steps (a step takes UNROLL keys per lane group; a workgroup holds at least 4 waves x 64 / 16 groups), the
        step's own row folded in after the loop, the exchange tree, the waves' meeting, the combine

    dequantize.  No zero point is folded: a code converts to float32 exactly.  Scores: the kernel forms
    fl(fl(sum q c) fl(ks scale)) where decode_oracle's model has fl(scale fl(sum q k^)); the sums carry the same relative
    error (k^ = c ks: a common factor), and the kernel has ONE rounding more, <= u |s| <= u S; 2 u S is allowed.  A score off
    by e moves every weight by a relative 2 e at most (numerator and denominator): 4 u S (p |v^|).  Values: the kernel
    accumulates fl(p vs) c where the model has p v^ — one rounding more per term, u (p |v^|); 2 u is allowed.

    |o - o64| <= decode_oracle's bound with this R + (4 S + 2) u (p |v^|)
"""

import numpy as np

import attn_oracle as ao
import decode_oracle as do
from tinynn_autograd_amd import kvq

CHUNK, UNROLL = kvq.CHUNK, kvq.UNROLL


def check_rows(x, codes, scales, what):
    """The properties of quantized rows: x float32 [..., W], codes uint8 [..., W], scales float32 [...]."""
    x = np.asarray(x, dtype=np.float32)
    c = np.asarray(codes).view(np.int8).astype(np.float64)
    s = np.asarray(scales, dtype=np.float32)
    want = (np.abs(x).max(axis=-1) / np.float32(127)).astype(np.float32)
    assert (np.abs(s.astype(np.float64) - want) <= np.spacing(want)).all(), "%s: a scale is more than one ulp from absmax / 127" % what
    assert (np.abs(c) <= 127).all(), "%s: a code outside [-127, 127]" % what
    err = np.abs(x.astype(np.float64) - c * s.astype(np.float64)[..., None])
    assert (err <= s.astype(np.float64)[..., None] * (0.5 + 2.0 ** -20)).all(), "%s: |x - code scale| exceeds scale / 2" % what
    zero = np.abs(x).max(axis=-1) == 0
    assert (s[zero] == 0).all() and (c[zero] == 0).all(), "%s: a zero row must have scale 0 and codes 0" % what


def rescales(keys, splits):
    chunks = -(-keys // CHUNK)
    run = max((s + 1) * chunks // splits - s * chunks // splits for s in range(splits)) * CHUNK
    return -(-run // (UNROLL * 16)) + 1 + 6 + 1 + 1


def decode_reference(q, k_codes, v_codes, k_scales, v_scales, keys, scale=None, layout="bthd", splits=1):
    """(o [B, H, Dv] float64, its elementwise bound) over cache rows [0, keys) of the codes and scales as they are."""
    h_axis = 2 if layout == "bthd" else 1
    group = q.shape[1] // k_codes.shape[h_axis]
    k = np.repeat(kvq.dequantize_host(k_codes, k_scales), group, axis=h_axis)
    v = np.repeat(kvq.dequantize_host(v_codes, v_scales), group, axis=h_axis)
    base = do.decode_reference(q, k, v, keys, None, None, scale, layout, np.float32, 1)
    b, h, d = q.shape
    q4 = np.asarray(q, dtype=np.float64).reshape((b, 1, h, d) if layout == "bthd" else (b, h, 1, d))
    q3, k3, v3 = ao.to3(q4, layout), ao.to3(do.live_rows(k, layout, keys), layout), ao.to3(do.live_rows(v, layout, keys), layout)
    scale = float(ao.default_scale(q4) if scale is None else scale)
    S = abs(scale) * np.einsum("bid,bjd->bij", np.abs(q3), np.abs(k3)).max(axis=-1, keepdims=True)
    s = scale * np.einsum("bid,bjd->bij", q3, k3)
    p = np.exp(s - s.max(axis=-1, keepdims=True))
    p /= p.sum(axis=-1, keepdims=True)
    pv = p @ np.abs(v3)
    u = ao.unit(np.float32)
    per_factor = 2 * ((2 * do.EXP_ULP + 1) * u + 2 * u * S) * pv
    extra = (rescales(keys, splits) - do.rescales(keys, 1)) * per_factor + (4 * S + 2) * u * pv
    return base.values["o"], base.bounds["o"] + extra.reshape(base.bounds["o"].shape)
