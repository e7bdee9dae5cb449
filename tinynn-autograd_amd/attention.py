"""Host planner of scaled-dot-product attention (numpy only, no device import): from operand shapes, layout and options to
ONE plan — validated extents, the element strides of every operand, the output shape, the scale and the route.

    o = softmax(scale q k^T) v        softmax over the keys; scale defaults to 1 / sqrt(D)

Layouts (dense arrays)
    "bhtd"  q [..., Tq, D], k [..., Tk, D], v [..., Tk, Dv] -> o [..., Tq, Dv]; the leading dimensions (zero or more, identical
            on all three, no broadcasting) fold into the batch, H = 1
    "bthd"  q [B, Tq, H, D], k [B, Tk, H, D], v [B, Tk, H, Dv] -> o [B, Tq, H, Dv]: what a [B T, H D] projection reshapes to
            for free; the kernels take strides, so a multi-head layer needs no transpose at all

causal=True keeps key j for query i iff j <= i (top-left aligned for any Tq, Tk: every row keeps key 0, no row is empty).

Routes
    native    csrc/tnn_attn.hip: one launch forward, one for dq (+ delta), one for dk + dv; the scores never reach memory.
              Needs the entry points, float32 / float64 operands and D, Dv <= MAX_HEAD_DIM (where the output accumulator
              and the K / V tiles still fit registers and LDS).
    composed  the same mathematics on the array operations that already exist (two batched products, a max-subtract, exp,
              sum, divide).  What runs under the CPU test twin, what `fused=False` layers use, and the second, independent
              implementation the GPU tests compare the kernels with.
"""

import math

MAX_HEAD_DIM = 128        # TNN_ATTN_MAX_HEAD_DIM
BLOCK_Q = 64              # TNN_ATTN_BLOCK_Q: query rows per workgroup (key rows per workgroup of the dk / dv launch)
WAVE_ROWS = 16            # TNN_ATTN_WAVE_ROWS: rows of the block each of its four waves owns
BLOCK_K = 64              # TNN_ATTN_BLOCK_K: keys per step of the inner loop
MFMA_K = 4                # TNN_ATTN_MFMA_K: contraction depth of one MFMA
ROUTES = ("native", "composed")
LAYOUTS = ("bhtd", "bthd")


class AttnPlan(object):
    __slots__ = ("B", "H", "Tq", "Tk", "D", "Dv", "layout", "causal", "scale", "q_strides", "k_strides", "v_strides",
                 "o_strides", "out_shape", "lse_shape", "route")
    group = 1                 # query heads per key / value head (gqa.GqaAttnPlan: H / Hkv)

    def geometry(self):
        """The six extents every native entry point takes, in its argument order."""
        return (self.B, self.H, self.Tq, self.Tk, self.D, self.Dv)

    def strides(self, *names):
        """The (batch, head, row) element strides of the named operands ("q", "k", "v", "o"), flattened in that order; the
        gradient of an operand has the operand's strides."""
        out = []
        for n in names:
            out.extend(getattr(self, n + "_strides"))
        return out

    def empty(self):
        return self.B * self.H * self.Tq == 0

    def __repr__(self):
        return "AttnPlan(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.__slots__)


def _route(native, float_ok, fits, route):
    if route is not None:
        if route not in ROUTES:
            raise ValueError("route must be one of %s or None, got %r" % (ROUTES, route))
        if route == "native" and not (native and float_ok and fits):
            raise ValueError("the native attention route needs libtnn_hip.so, float32 / float64 operands and head "
                             "dimensions <= %d" % MAX_HEAD_DIM)
        return route
    return "native" if native and float_ok and fits else "composed"


def _strides(layout, H, T, W):
    """(batch, head, row) element strides of a dense operand with T rows of W elements per (batch, head)."""
    if layout == "bhtd":
        return (H * T * W, T * W, W)
    return (T * H * W, W, H * W)


def plan_attention(q_shape, k_shape, v_shape, causal=False, scale=None, layout="bhtd", native=True, float_ok=True,
                   route=None):
    """The plan of attention(q, k, v).  native: the library has the entry points; float_ok: every operand is (or will be
    made) float32 / float64 of one kind; route: force one ("native" / "composed"), None picks."""
    if layout not in LAYOUTS:
        raise ValueError("attention: layout must be one of %s, got %r" % (LAYOUTS, layout))
    q_shape, k_shape, v_shape = (tuple(int(s) for s in sh) for sh in (q_shape, k_shape, v_shape))
    p = AttnPlan()
    if layout == "bhtd":
        if min(len(q_shape), len(k_shape), len(v_shape)) < 2:
            raise ValueError("attention: the operands must be [..., T, D], got shapes q %s, k %s, v %s"
                             % (q_shape, k_shape, v_shape))
        lead = q_shape[:-2]
        if k_shape[:-2] != lead or v_shape[:-2] != lead:
            raise ValueError("attention: the leading dimensions must be identical (no broadcasting), got q %s, k %s, v %s"
                             % (q_shape, k_shape, v_shape))
        p.B, p.H = math.prod(lead), 1
        (p.Tq, p.D), (tk, dk), (tv, p.Dv) = q_shape[-2:], k_shape[-2:], v_shape[-2:]
    else:
        if not len(q_shape) == len(k_shape) == len(v_shape) == 4:
            raise ValueError("attention: layout \"bthd\" takes [B, T, H, D] operands, got shapes q %s, k %s, v %s"
                             % (q_shape, k_shape, v_shape))
        if not (q_shape[0] == k_shape[0] == v_shape[0] and q_shape[2] == k_shape[2] == v_shape[2]):
            raise ValueError("attention: batch and head extents must be identical (no broadcasting), got q %s, k %s, v %s"
                             % (q_shape, k_shape, v_shape))
        p.B, p.Tq, p.H, p.D = q_shape
        tk, dk = k_shape[1], k_shape[3]
        tv, p.Dv = v_shape[1], v_shape[3]
        lead = None
    if dk != p.D:
        raise ValueError("attention: q has head dimension %d, k has %d" % (p.D, dk))
    if tv != tk:
        raise ValueError("attention: k holds %d keys, v holds %d" % (tk, tv))
    p.Tk = tk
    if p.Tk < 1:
        raise ValueError("attention: no keys (k %s): the softmax of an empty row is undefined" % (k_shape,))
    if p.D < 1:
        raise ValueError("attention: empty head dimension (q %s, k %s)" % (q_shape, k_shape))
    if p.Dv < 1:
        raise ValueError("attention: empty value dimension (v %s)" % (v_shape,))
    p.layout, p.causal = layout, bool(causal)
    if scale is None:
        scale = 1.0 / math.sqrt(p.D)
    p.scale = float(scale)
    if not math.isfinite(p.scale):
        raise ValueError("attention: scale must be finite, got %r" % (scale,))
    p.q_strides = _strides(layout, p.H, p.Tq, p.D)
    p.k_strides = _strides(layout, p.H, p.Tk, p.D)
    p.v_strides = _strides(layout, p.H, p.Tk, p.Dv)
    p.o_strides = _strides(layout, p.H, p.Tq, p.Dv)
    if layout == "bhtd":
        p.out_shape = lead + (p.Tq, p.Dv)
        p.lse_shape = lead + (p.Tq,)
    else:
        p.out_shape = (p.B, p.Tq, p.H, p.Dv)
        p.lse_shape = (p.B, p.H, p.Tq)
    fits = p.D <= MAX_HEAD_DIM and p.Dv <= MAX_HEAD_DIM
    p.route = _route(native, float_ok, fits, route)
    return p

