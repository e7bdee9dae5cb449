"""Host planner of the int8 key / value cache (numpy only, no device import): the format, stated in numpy, and from operand
shapes and options to ONE plan per call — validated extents, element strides, the key split, the workspace size, the route.

The format (include/tnn_kvq.h).  Every cache row (b, t, hk) holds D codes of K and Dv codes of V — int8 two's-complement
bytes in uint8 arrays — and one float32 scale per row and tensor.  Symmetric, per row:

    scale = absmax / 127          code = clamp(rne(x / scale), -127, 127)          x^ = code * scale

in float32; a row of zeros has scale 0 and codes 0.  The float32 quotient is itself rounded, so one residual step moves a
code that is more than scale / 2 from x by one: |x - code scale| <= scale / 2 for every element (quantize_host).
A row of D codes costs D + 4 bytes instead of 4 D: 3.88x less at D 128.  Non-finite inputs are out of scope.

Layouts (dense arrays; q and o are dense [B, H, D] / [B, H, Dv], k_new and v_new [B, Hkv, D] / [B, Hkv, Dv] in both)
    "bthd"  codes [B, Tmax, Hkv, D | Dv] uint8, scales [B, Tmax, Hkv] float32
    "bhtd"  codes [B, Hkv, Tmax, D | Dv] uint8, scales [B, Hkv, Tmax] float32

Key split.  decoding.choose_splits on chunks of CHUNK = 256 keys (the BYTES of a float chunk of 64 keys) and on B Hkv
workgroup rows: one workgroup serves all H / Hkv queries of a key / value head.

Routes
    native    csrc/tnn_kvq.hip.  Needs the entry points, float32 operands, D and Dv multiples of 16 up to MAX_HEAD_DIM,
              16-byte aligned bases and a group <= MAX_GROUP.
    composed  the step's row is quantized on the host (quantize_host) and slice-assigned, the live prefix is dequantized on
              the host and the existing composed decode runs over it.  What runs under the CPU test twin and the second,
              independent implementation the GPU tests compare the kernel with; it reads values back, so it raises inside an
              open graph capture.

SLOWER_RULES lists the regions in which the probe (tools/probes/kvq_ab.py, profiles/kvq_vs_float.txt) found the int8 step
SLOWER than the float32 step of the same logical shape — the cache still saves its memory there; expect_slower() tells a
caller who quantizes for speed alone.  Out of scope: fp8 / int4 codes, per-channel scales, chunked prefill over a quantized
cache, training, float64.
"""

import math

import numpy as np

from . import decoding as _dc
from . import gqa as _gq

VEC = 16                  # TNN_KVQ_VEC: codes per lane and access
CHUNK = 256               # TNN_KVQ_CHUNK: keys per chunk
MAX_SPLITS = 256          # TNN_KVQ_MAX_SPLITS
UNROLL = 4                # TNN_KVQ_UNROLL: keys a lane group has in flight
MAX_HEAD_DIM = 256        # TNN_KVQ_MAX_HEAD_DIM
MAX_GROUP = _gq.MAX_GROUP
STATES = _gq.DECODE_STATES
MAX_BH = _dc.MAX_BH
ROUTES = ("native", "composed")
LAYOUTS = _dc.LAYOUTS
QUANTS = ("int8",)
# (group, most B Hkv, most keys): a native plan with that group, B Hkv <= the first and keys <= the second is SLOWER than the
# float32 step — profiles/kvq_vs_float.txt, section (a): at 256 keys (ONE chunk, so one workgroup per key / value head, and
# the step's row handled after the loop) the call takes 0.79x .. 0.93x the float call's speed, both within 10 us of an empty
# two-launch call; from 4096 keys on every measured shape is faster (1.2x .. 3.6x).  Groups 2 and 4 and the lengths between
# 256 and 4096 were not measured.
SLOWER_RULES = ((1, 64, 257), (8, 64, 257))


def expect_slower(group, bhk, keys):
    """Whether SLOWER_RULES marks the shape: the int8 step then costs more time than the float32 one (it still saves memory)."""
    return any(group == g and bhk <= most_bhk and keys <= most_keys for g, most_bhk, most_keys in SLOWER_RULES)


# ---------------------------------------------------------------------- the format
def quantize_host(x):
    """x float32 [..., W] -> (codes uint8 [..., W] holding int8 bytes, scales float32 [...]): the rule of the module's head."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    amax = np.abs(x).max(axis=-1) if x.shape[-1] else np.zeros(x.shape[:-1], np.float32)
    scales = (amax / np.float32(127)).astype(np.float32)
    s = scales[..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.rint((x / s).astype(np.float32))
    r = np.where(s > 0, r, np.float32(0)).astype(np.float32)
    # the residual step: what the rounded quotient left (a fused multiply-add's single rounding), at most one step off
    e = (x.astype(np.float64) - r.astype(np.float64) * s.astype(np.float64)).astype(np.float32)
    half = np.float32(0.5) * s
    r = r + np.where(e > half, 1, 0) - np.where(e < -half, 1, 0)
    r = np.where(s > 0, np.clip(r, -127, 127), 0)
    return r.astype(np.int8).view(np.uint8), scales


def dequantize_host(codes, scales, dtype=np.float64):
    """code * scale in `dtype` (float64: exact)."""
    c = np.ascontiguousarray(codes, dtype=np.uint8).view(np.int8).astype(dtype)
    return c * np.asarray(scales, dtype=np.float32).astype(dtype)[..., None]


def codes_shape(layout, B, Hkv, Tmax, W):
    return _dc.cache_shape(layout, B, Hkv, Tmax, W)


def scales_shape(layout, B, Hkv, Tmax):
    if layout not in LAYOUTS:
        raise ValueError("kvq: layout must be one of %s, got %r" % (LAYOUTS, layout))
    return (B, Tmax, Hkv) if layout == "bthd" else (B, Hkv, Tmax)


def _cache_strides(layout, Hkv, Tmax, W):
    """(batch, head, row) element strides of a dense cache operand of row width W (1: the scales)."""
    return (Tmax * Hkv * W, W, Hkv * W) if layout == "bthd" else (Hkv * Tmax * W, Tmax * W, W)


def _route(what, ok, why, route):
    if route is not None:
        if route not in ROUTES:
            raise ValueError("route must be one of %s or None, got %r" % (ROUTES, route))
        if route == "native" and not ok:
            raise ValueError("the native %s route needs libtnn_hip.so, float32 operands, head dimensions in multiples of %d up "
                             "to %d, 16-byte aligned operands and a group <= %d (%s)" % (what, VEC, MAX_HEAD_DIM, MAX_GROUP, why))
        return route
    return "native" if ok else "composed"


def _fits(D, Dv):
    return all(w % VEC == 0 and VEC <= w <= MAX_HEAD_DIM for w in (D, Dv))


def _caches(what, layout, k_codes_shape, v_codes_shape, k_scales_shape, v_scales_shape):
    """(B, Hkv, Tmax, D, Dv) of the four cache operands after the checks that tie them together."""
    if layout not in LAYOUTS:
        raise ValueError("%s: layout must be one of %s, got %r" % (what, LAYOUTS, layout))
    kc, vc, ks, vs = (tuple(int(s) for s in sh) for sh in (k_codes_shape, v_codes_shape, k_scales_shape, v_scales_shape))
    if len(kc) != 4 or len(vc) != 4:
        raise ValueError("%s: the code arrays must have four axes (layout %r), got shapes %s and %s" % (what, layout, kc, vc))
    tv, hv = (1, 2) if layout == "bthd" else (2, 1)
    B, Tmax, Hkv, D, Dv = kc[0], kc[tv], kc[hv], kc[3], vc[3]
    if vc != codes_shape(layout, B, Hkv, Tmax, Dv):
        raise ValueError("%s: v_codes %s does not match k_codes %s" % (what, vc, kc))
    want = scales_shape(layout, B, Hkv, Tmax)
    if ks != want or vs != want:
        raise ValueError("%s: the scales must be %s (one per cache row), got %s and %s" % (what, want, ks, vs))
    if D < 1 or Dv < 1 or Tmax < 1:
        raise ValueError("%s: empty head dimension or cache (k_codes %s, v_codes %s)" % (what, kc, vc))
    if B * Hkv >= MAX_BH:
        raise ValueError("%s: B Hkv = %d must stay below %d" % (what, B * Hkv, MAX_BH))
    return B, Hkv, Tmax, D, Dv


class KvqFillPlan(object):
    __slots__ = ("B", "T", "Hkv", "D", "Dv", "row0", "Tmax", "layout", "k_strides", "v_strides", "kcodes_strides",
                 "vcodes_strides", "kscales_strides", "vscales_strides", "route")

    def geometry(self):
        """B, T, Hkv, D, Dv, row0, Tmax in the order tnn_kvq_quantize_rows takes them."""
        return (self.B, self.T, self.Hkv, self.D, self.Dv, self.row0, self.Tmax)

    def strides(self):
        return (self.k_strides + self.v_strides + self.kcodes_strides + self.vcodes_strides + self.kscales_strides
                + self.vscales_strides)

    def empty(self):
        return self.B * self.T * self.Hkv == 0


def plan_kvq_fill(k_shape, v_shape, k_codes_shape, v_codes_shape, k_scales_shape, v_scales_shape, row0=0, layout="bthd",
                  native=True, float_ok=True, aligned=True, route=None):
    """The plan of kvq_quantize_rows: k [B, T, Hkv, D] and v [B, T, Hkv, Dv] (dense) into cache rows [row0, row0 + T)."""
    what = "kvq_quantize_rows"
    p = KvqFillPlan()
    p.B, p.Hkv, p.Tmax, p.D, p.Dv = _caches(what, layout, k_codes_shape, v_codes_shape, k_scales_shape, v_scales_shape)
    k_shape, v_shape = tuple(int(s) for s in k_shape), tuple(int(s) for s in v_shape)
    if len(k_shape) != 4 or k_shape[:1] + k_shape[2:] != (p.B, p.Hkv, p.D) or v_shape != k_shape[:3] + (p.Dv,):
        raise ValueError("%s: k and v must be [B, T, Hkv, D] = [%d, T, %d, %d] and [.., %d], got %s and %s"
                         % (what, p.B, p.Hkv, p.D, p.Dv, k_shape, v_shape))
    p.T, p.layout = k_shape[1], layout
    p.row0 = _dc._int(row0, what + ": row0")
    if p.row0 < 0 or p.row0 + p.T > p.Tmax:
        raise ValueError("%s: rows [%d, %d) lie outside the cache's %d rows" % (what, p.row0, p.row0 + p.T, p.Tmax))
    p.k_strides, p.v_strides = (p.T * p.Hkv * p.D, p.D, p.Hkv * p.D), (p.T * p.Hkv * p.Dv, p.Dv, p.Hkv * p.Dv)
    p.kcodes_strides, p.vcodes_strides = _cache_strides(layout, p.Hkv, p.Tmax, p.D), _cache_strides(layout, p.Hkv, p.Tmax, p.Dv)
    p.kscales_strides = p.vscales_strides = _cache_strides(layout, p.Hkv, p.Tmax, 1)
    ok = native and float_ok and aligned and _fits(p.D, p.Dv)
    p.route = _route("int8 cache fill", ok, "D %d, Dv %d" % (p.D, p.Dv), route)
    return p


class KvqDecodePlan(object):
    __slots__ = ("B", "H", "Hkv", "group", "D", "Dv", "Tmax", "length", "ragged", "keys", "chunks", "splits", "layout", "scale",
                 "q_strides", "knew_strides", "vnew_strides", "kcodes_strides", "vcodes_strides", "o_strides", "kscales_strides",
                 "vscales_strides", "out_shape", "states", "route")

    def geometry(self):
        """B, H, Hkv, len, Tmax, D, Dv in the order tnn_kvq_decode_attn takes them (ragged: len 0, it is not read)."""
        return (self.B, self.H, self.Hkv, 0 if self.ragged else self.length, self.Tmax, self.D, self.Dv)

    def strides(self):
        """The eight (batch, head, row) element stride triples, flattened, in the order of include/tnn_kvq.h."""
        return (self.q_strides + self.knew_strides + self.vnew_strides + self.kcodes_strides + self.vcodes_strides
                + self.o_strides + self.kscales_strides + self.vscales_strides)

    def empty(self):
        return self.B * self.H == 0

    def workspace_bytes(self):
        """What tnn_kvq_decode_workspace returns: a float32 record (m, l, acc[Dv]) per (b, QUERY head, split)."""
        if self.splits == 1:
            return 0
        return _dc._round16(self.B * self.H * self.splits * (self.Dv + 2) * 4)

    def __repr__(self):
        return "KvqDecodePlan(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.__slots__)


def plan_kvq_decode(q_shape, k_codes_shape, v_codes_shape, k_scales_shape, v_scales_shape, length=None, k_new_shape=None,
                    v_new_shape=None, scale=None, layout="bthd", splits=None, lens_shape=None, native=True, float_ok=True,
                    aligned=True, route=None):
    """The plan of attention_decode_kvq.  q [B, H, D]; k_new [B, Hkv, D] and v_new [B, Hkv, Dv] (required: the step appends
    its row at `length`, or — lens_shape given, length None — at lens[b], read on the device; the grid is then sized for a
    cache one row short of full)."""
    what = "attention_decode_kvq"
    ragged = lens_shape is not None
    if ragged == (length is not None):
        raise ValueError("%s: give length= (a host integer shared by the batch) or lens= (one per sequence), not both" % what)
    p = KvqDecodePlan()
    p.B, p.Hkv, p.Tmax, p.D, p.Dv = _caches(what, layout, k_codes_shape, v_codes_shape, k_scales_shape, v_scales_shape)
    q_shape = tuple(int(s) for s in q_shape)
    if len(q_shape) != 3 or q_shape[0] != p.B or q_shape[2] != p.D:
        raise ValueError("%s: q must be [B, H, D] = [%d, H, %d], got shape %s" % (what, p.B, p.D, q_shape))
    p.H = q_shape[1]
    p.group = _gq.group_of(p.H, p.Hkv, what)
    if k_new_shape is None or v_new_shape is None:
        raise ValueError("%s: k_new and v_new are required (the step quantizes and appends its row)" % what)
    if tuple(int(s) for s in k_new_shape) != (p.B, p.Hkv, p.D) or tuple(int(s) for s in v_new_shape) != (p.B, p.Hkv, p.Dv):
        raise ValueError("%s: k_new and v_new must be %s and %s, got %s and %s"
                         % (what, (p.B, p.Hkv, p.D), (p.B, p.Hkv, p.Dv), tuple(k_new_shape), tuple(v_new_shape)))
    p.ragged, p.layout = ragged, layout
    if ragged:
        if tuple(int(s) for s in lens_shape) != (p.B,):
            raise ValueError("%s: lens must hold one length per sequence, shape (%d,), got %s" % (what, p.B, tuple(lens_shape)))
        p.length, bound = None, p.Tmax
    else:
        p.length = _dc._int(length, what + ": length")
        if not 0 <= p.length < p.Tmax:
            raise ValueError("%s: the cache is full — length %d of %d rows, no room for the new row" % (what, p.length, p.Tmax)
                             if p.length == p.Tmax else "%s: length %d outside [0, %d)" % (what, p.length, p.Tmax))
        bound = p.length + 1
    p.keys = bound
    p.chunks = -(-bound // CHUNK)
    most = min(p.chunks, MAX_SPLITS)
    if splits is None:
        p.splits = _dc.choose_splits(p.B * p.Hkv, p.chunks)
    else:
        p.splits = _dc._int(splits, what + ": splits")
        if not 1 <= p.splits <= most:
            raise ValueError("%s: splits %d outside [1, %d] (%d chunks of %d keys)" % (what, p.splits, most, p.chunks, CHUNK))
    p.scale = float(1.0 / math.sqrt(p.D) if scale is None else scale)
    if not math.isfinite(p.scale):
        raise ValueError("%s: scale must be finite, got %r" % (what, scale))
    p.q_strides, p.o_strides = (p.H * p.D, p.D, 0), (p.H * p.Dv, p.Dv, 0)
    p.knew_strides, p.vnew_strides = (p.Hkv * p.D, p.D, 0), (p.Hkv * p.Dv, p.Dv, 0)
    p.kcodes_strides, p.vcodes_strides = _cache_strides(layout, p.Hkv, p.Tmax, p.D), _cache_strides(layout, p.Hkv, p.Tmax, p.Dv)
    p.kscales_strides = p.vscales_strides = _cache_strides(layout, p.Hkv, p.Tmax, 1)
    p.out_shape = (p.B, p.H, p.Dv)
    p.states = next((s for s in STATES if s >= p.group), None)
    ok = native and float_ok and aligned and _fits(p.D, p.Dv) and p.group <= MAX_GROUP
    p.route = _route("int8 decode attention", ok, "D %d, Dv %d, group %d" % (p.D, p.Dv, p.group), route)
    return p
