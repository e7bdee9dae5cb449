"""Host planner of cache-extending attention (numpy only, no device import): from operand shapes and options to ONE plan —
validated extents, the element strides of every operand, the scale, the grid and the route.

    attention_extend    T NEW rows per sequence attend over the `length` cached rows and over themselves and are appended to
                        the cache: query row i sits at the absolute position length + i and sees the absolute keys
                        j <= length + i (the bottom-right causal rule); key j < length is cache row j, key j >= length is new
                        row j - length.  Afterwards cache rows [length, length + T) hold k_new / v_new bit for bit.  `length`
                        is a host integer shared by the batch; length == 0 is a prefill straight into the cache.

Layouts (dense arrays; every operand of a call is in the same one)
    "bthd"  q [B, T, H, D], k_new [B, T, Hkv, D], v_new [B, T, Hkv, Dv], k_cache [B, Tmax, Hkv, D], v_cache [B, Tmax, Hkv, Dv],
            o [B, T, H, Dv]: what [B T, H D] projections reshape to
    "bhtd"  q [B, H, T, D], k_new [B, Hkv, T, D], v_new [B, Hkv, T, Dv], k_cache [B, Hkv, Tmax, D], v_cache [B, Hkv, Tmax, Dv],
            o [B, H, T, Dv]
H % Hkv == 0: query head h reads key / value head h // (H / Hkv); Hkv == H is plain multi-head attention.  There is no group
limit: a group only changes the head index.

Routes
    native    csrc/tnn_extend.hip: ONE tnn_extend_attn launch of B H ceil(T / BLOCK_Q) workgroups (float64: one wave per
              row).  Needs the entry point, float32 / float64 operands, D, Dv <= MAX_HEAD_DIM and tensors below 2^31 elements.
    composed  a slice assignment of the new rows, k and v repeated over the group, then the composed attention over rows
              [0, length + T) with the offset mask j <= length + i.  What runs under the CPU test twin and the second,
              independent implementation the GPU tests compare the kernel with.

The keys are not split: a short chunk over a long cache leaves the machine idle (T == 1 stays decoding.py's).  RULES is where
a probe may later send such regions elsewhere; nothing is fixed in advance.  Out of scope: lengths read on the device (ragged
chunks), bf16.
"""

import math

import numpy as np

BLOCK_Q = 64              # TNN_ATTN_BLOCK_Q: query rows per workgroup
BLOCK_K = 64              # TNN_EXTEND_BLOCK_K: keys per block, aligned to the absolute key index
WAVE_ROWS = 16            # TNN_ATTN_WAVE_ROWS
MAX_HEAD_DIM = 128        # TNN_ATTN_MAX_HEAD_DIM
LIMIT = 1 << 31           # every tensor holds fewer elements than this
ROUTES = ("native", "composed")
LAYOUTS = ("bthd", "bhtd")
# Regions that the probe marks SLOWER than another route would be listed here as (most T, least keys) and sent there, as
# decoding.FWD_RULES does for the decode step.  Empty, and nothing reads it yet: profiles/extend_vs_fwd.txt shows one such
# region (T 16 over 4096 cached rows loses to 16 decode steps, T = 1 loses everywhere and is the layer's decode step anyway),
# and the route it would go to — a loop of decode steps — is not one of ROUTES.
RULES = ()

_WHAT = "attention_extend"


def _int(value, what):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise ValueError("%s: %s must be an integer, got %r" % (_WHAT, what, value))
    return int(value)


class ExtendPlan(object):
    __slots__ = ("B", "H", "Hkv", "group", "T", "D", "Dv", "Tmax", "length", "keys", "layout", "scale", "q_strides",
                 "knew_strides", "vnew_strides", "kcache_strides", "vcache_strides", "o_strides", "out_shape", "route")

    def geometry(self):
        """B, H, Hkv, T, len, Tmax, D, Dv in the order tnn_extend_attn takes them."""
        return (self.B, self.H, self.Hkv, self.T, self.length, self.Tmax, self.D, self.Dv)

    def strides(self):
        """The six (batch, head, row) element stride triples, flattened: q, k_new, v_new, k_cache, v_cache, o."""
        return (self.q_strides + self.knew_strides + self.vnew_strides + self.kcache_strides + self.vcache_strides
                + self.o_strides)

    def empty(self):
        return self.B * self.H == 0

    def query_blocks(self):
        return -(-self.T // BLOCK_Q)

    def grid(self, itemsize=4):
        """Workgroups of the launch: B H ceil(T / BLOCK_Q) (float32); float64 runs one wave per row, four per workgroup."""
        if itemsize == 8:
            return -(-self.B * self.H * self.T // 4)
        return self.B * self.H * self.query_blocks()

    def key_blocks(self, q0):
        """The key blocks [(first key, end key)] that the query block starting at row q0 walks: aligned to the ABSOLUTE key
        index, up to the one that holds position length + q0 + BLOCK_Q - 1 (or the last key)."""
        end = min(self.length + q0 + BLOCK_Q, self.keys)
        return [(k0, min(k0 + BLOCK_K, self.keys)) for k0 in range(0, end, BLOCK_K)]

    def __repr__(self):
        return "ExtendPlan(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.__slots__)


def operand_shape(layout, B, H, rows, W):
    if layout not in LAYOUTS:
        raise ValueError("%s: layout must be one of %s, got %r" % (_WHAT, LAYOUTS, layout))
    return (B, rows, H, W) if layout == "bthd" else (B, H, rows, W)


def _strides(layout, H, rows, W):
    """(batch, head, row) element strides of a dense operand."""
    return (rows * H * W, W, H * W) if layout == "bthd" else (H * rows * W, rows * W, W)


def plan_extend(q_shape, k_cache_shape, v_cache_shape, length, k_new_shape, v_new_shape, scale=None, layout="bthd",
                native=True, route=None, float_ok=True, pointers=None):
    """The plan of attention_extend.  pointers: the addresses (k_new, v_new, k_cache, v_cache) when the caller has them —
    a new operand that IS a cache is refused (the appended rows would be read after being written)."""
    if layout not in LAYOUTS:
        raise ValueError("%s: layout must be one of %s, got %r" % (_WHAT, LAYOUTS, layout))
    shapes = [tuple(int(s) for s in sh) for sh in (q_shape, k_cache_shape, v_cache_shape, k_new_shape, v_new_shape)]
    q_shape, k_cache_shape, v_cache_shape, k_new_shape, v_new_shape = shapes
    if any(len(sh) != 4 for sh in shapes):
        raise ValueError("%s: every operand must have four axes (layout %r), got q %s, k_cache %s, v_cache %s, k_new %s, "
                         "v_new %s" % ((_WHAT, layout) + tuple(shapes)))
    ta, ha = (1, 2) if layout == "bthd" else (2, 1)
    p = ExtendPlan()
    p.layout = layout
    p.B, p.T, p.H, p.D = q_shape[0], q_shape[ta], q_shape[ha], q_shape[3]
    p.Tmax, p.Hkv, p.Dv = k_cache_shape[ta], k_cache_shape[ha], v_cache_shape[3]
    if k_cache_shape != operand_shape(layout, p.B, p.Hkv, p.Tmax, p.D):
        raise ValueError("%s: k_cache %s does not match q %s in layout %r" % (_WHAT, k_cache_shape, q_shape, layout))
    if v_cache_shape != operand_shape(layout, p.B, p.Hkv, p.Tmax, p.Dv):
        raise ValueError("%s: v_cache %s does not match k_cache %s" % (_WHAT, v_cache_shape, k_cache_shape))
    if p.D < 1 or p.Dv < 1 or p.Tmax < 1:
        raise ValueError("%s: empty head dimension or cache (q %s, k_cache %s, v_cache %s)"
                         % (_WHAT, q_shape, k_cache_shape, v_cache_shape))
    if (p.H == 0) != (p.Hkv == 0) or (p.Hkv and p.H % p.Hkv != 0):
        raise ValueError("%s: H %d query heads is no multiple of Hkv %d key / value heads" % (_WHAT, p.H, p.Hkv))
    p.group = p.H // p.Hkv if p.Hkv else 1
    if p.T < 1:
        raise ValueError("%s: T = %d new rows (T >= 1)" % (_WHAT, p.T))
    if k_new_shape != operand_shape(layout, p.B, p.Hkv, p.T, p.D):
        raise ValueError("%s: k_new must be %s, got %s" % (_WHAT, operand_shape(layout, p.B, p.Hkv, p.T, p.D), k_new_shape))
    if v_new_shape != operand_shape(layout, p.B, p.Hkv, p.T, p.Dv):
        raise ValueError("%s: v_new must be %s, got %s" % (_WHAT, operand_shape(layout, p.B, p.Hkv, p.T, p.Dv), v_new_shape))
    p.length = _int(length, "length")
    if p.length < 0:
        raise ValueError("%s: length %d must be >= 0" % (_WHAT, p.length))
    if p.length + p.T > p.Tmax:
        raise ValueError("%s: length %d + T %d new rows overflow a cache of %d rows" % (_WHAT, p.length, p.T, p.Tmax))
    p.keys = p.length + p.T
    if pointers is not None:
        kn, vn, kc, vc = pointers
        if kn in (kc, vc) or vn in (kc, vc):
            raise ValueError("%s: k_new / v_new alias a cache (the appended rows would be read after being written)" % _WHAT)
    if scale is None:
        scale = 1.0 / math.sqrt(p.D)
    p.scale = float(scale)
    if not math.isfinite(p.scale):
        raise ValueError("%s: scale must be finite, got %r" % (_WHAT, scale))
    p.q_strides, p.o_strides = _strides(layout, p.H, p.T, p.D), _strides(layout, p.H, p.T, p.Dv)
    p.knew_strides, p.vnew_strides = _strides(layout, p.Hkv, p.T, p.D), _strides(layout, p.Hkv, p.T, p.Dv)
    p.kcache_strides, p.vcache_strides = _strides(layout, p.Hkv, p.Tmax, p.D), _strides(layout, p.Hkv, p.Tmax, p.Dv)
    p.out_shape = operand_shape(layout, p.B, p.H, p.T, p.Dv)
    wide = max(p.D, p.Dv)
    fits = (p.D <= MAX_HEAD_DIM and p.Dv <= MAX_HEAD_DIM and p.B * p.H * p.T * wide < LIMIT
            and p.B * p.Hkv * p.Tmax * wide < LIMIT)
    if route is not None and route not in ROUTES:
        raise ValueError("%s: route must be one of %s or None, got %r" % (_WHAT, ROUTES, route))
    if route == "native" and not (native and float_ok and fits):
        raise ValueError("the native %s route needs libtnn_hip.so, float32 / float64 operands, head dimensions <= %d and "
                         "tensors below 2^31 elements" % (_WHAT, MAX_HEAD_DIM))
    p.route = route or ("native" if native and float_ok and fits else "composed")
    return p
