"""Host planner of grouped-query attention (numpy only, no device import): H query heads share Hkv key / value heads,
H % Hkv == 0, group = H / Hkv, query head h reads key / value head h // group.  Hkv == 1 is multi-query attention, Hkv == H
multi-head attention.  From operand shapes and options to ONE plan, in the style of attention.py and decoding.py, whose
checks, strides and split rule it reuses.

    training    layout "bthd" only (what a [B T, H D] projection reshapes to): q [B, Tq, H, D], k [B, Tk, Hkv, D],
                v [B, Tk, Hkv, Dv] -> o [B, Tq, H, Dv]; lse and delta [B, H, Tq]; dk and dv have the shapes of k and v and are
                the sums over the group's query heads
    decode      q [B, H, D] -> o [B, H, Dv]; k_new [B, Hkv, D], v_new [B, Hkv, Dv]; the caches hold Hkv heads in either layout
                of decoding.LAYOUTS.  `length` is a host integer, or (ragged) every sequence's length is read on the device.
                The key split follows decoding.choose_splits with B Hkv in place of B H: that is the number of workgroup rows,
                one workgroup serving all `group` queries of a key / value head from one read of each K / V row.

Routes
    native    csrc/tnn_gqa.hip.  Needs the entry points, float32 / float64 operands, D, Dv <= MAX_HEAD_DIM and
              group <= MAX_GROUP.
    composed  k and v repeated over the group with the array operations that exist, then the composed attention / decode of
              device_array; dk and dv are summed over the group axis.  What runs under the CPU test twin, for groups above
              MAX_GROUP, and the second, independent implementation the GPU tests compare the kernels with.  The ragged
              composed decode loops over the sequences on the host and raises inside an open graph capture.

No routing rule between the two is drawn from measurements yet (profiles/gqa_vs_expanded.txt is written by
tools/probes/gqa_ab.py).  Out of scope: groups above MAX_GROUP on the native route, bf16 (chunked
prefill over grouped caches is extend.py's).
"""

from . import attention as _at
from . import decoding as _dc

MAX_GROUP = 8             # TNN_GQA_MAX_GROUP: most query heads per key / value head on the native route
DECODE_STATES = (1, 2, 4, 8)   # query states the decode kernel is compiled for; a group runs in the next one that holds it
MAX_HEAD_DIM = _at.MAX_HEAD_DIM
ROUTES = ("native", "composed")
LAYOUTS = _dc.LAYOUTS


def group_of(H, Hkv, what):
    """group = H / Hkv after the divisibility checks (0 heads on both sides: group 1)."""
    H, Hkv = int(H), int(Hkv)
    if H == 0 and Hkv == 0:
        return 1
    if Hkv < 1 or H < 1:
        raise ValueError("%s: %d query heads over %d key / value heads" % (what, H, Hkv))
    if H % Hkv:
        raise ValueError("%s: the %d query heads are no multiple of the %d key / value heads" % (what, H, Hkv))
    return H // Hkv


def _route(native, float_ok, fits, group, route, what):
    ok = native and float_ok and fits and group <= MAX_GROUP
    if route is not None:
        if route not in ROUTES:
            raise ValueError("route must be one of %s or None, got %r" % (ROUTES, route))
        if route == "native" and not ok:
            raise ValueError("the native %s route needs libtnn_hip.so, float32 / float64 operands, head dimensions <= %d and "
                             "a group <= %d (got group %d)" % (what, MAX_HEAD_DIM, MAX_GROUP, group))
        return route
    return "native" if ok else "composed"


class GqaAttnPlan(object):
    __slots__ = ("B", "H", "Hkv", "group", "Tq", "Tk", "D", "Dv", "causal", "scale", "q_strides", "k_strides", "v_strides",
                 "o_strides", "out_shape", "lse_shape", "k_shape", "v_shape", "route")
    layout = "bthd"

    def geometry(self):
        """The seven extents every native training entry point takes, in its argument order."""
        return (self.B, self.H, self.Hkv, self.Tq, self.Tk, self.D, self.Dv)

    def strides(self, *names):
        """The (batch, head, row) element strides of the named operands ("q", "k", "v", "o"), flattened in that order."""
        out = []
        for n in names:
            out.extend(getattr(self, n + "_strides"))
        return out

    def empty(self):
        return self.B * self.H * self.Tq == 0

    def expanded_shape(self, width):
        """[B, Tk, H, width]: k or v repeated over the group (the composed route)."""
        return (self.B, self.Tk, self.H, width)

    def __repr__(self):
        return "GqaAttnPlan(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.__slots__)


def plan_gqa_attention(q_shape, k_shape, v_shape, causal=False, scale=None, native=True, float_ok=True, route=None):
    """The plan of gqa_attention(q, k, v): q [B, Tq, H, D], k [B, Tk, Hkv, D], v [B, Tk, Hkv, Dv]."""
    what = "gqa_attention"
    q_shape, k_shape, v_shape = (tuple(int(s) for s in sh) for sh in (q_shape, k_shape, v_shape))
    if not len(q_shape) == len(k_shape) == len(v_shape) == 4:
        raise ValueError("%s: the operands are q [B, Tq, H, D], k [B, Tk, Hkv, D], v [B, Tk, Hkv, Dv], got shapes q %s, k %s, "
                         "v %s" % (what, q_shape, k_shape, v_shape))
    if k_shape[2] != v_shape[2]:
        raise ValueError("%s: k holds %d heads, v holds %d" % (what, k_shape[2], v_shape[2]))
    p = GqaAttnPlan()
    p.H, p.Hkv = q_shape[2], k_shape[2]
    p.group = group_of(p.H, p.Hkv, what)
    # everything attention.py checks, on the operands as they are after the repeat over the group
    try:
        base = _at.plan_attention(q_shape, k_shape[:2] + (p.H, k_shape[3]), v_shape[:2] + (p.H, v_shape[3]), causal, scale,
                                  "bthd", route="composed")
    except ValueError as exc:
        raise ValueError(str(exc).replace("attention:", what + ":"))
    p.B, p.Tq, p.Tk, p.D, p.Dv = base.B, base.Tq, base.Tk, base.D, base.Dv
    p.causal, p.scale = base.causal, base.scale
    p.q_strides, p.o_strides = base.q_strides, base.o_strides
    p.k_strides = _at._strides("bthd", p.Hkv, p.Tk, p.D)
    p.v_strides = _at._strides("bthd", p.Hkv, p.Tk, p.Dv)
    p.out_shape, p.lse_shape = base.out_shape, base.lse_shape
    p.k_shape, p.v_shape = k_shape, v_shape
    fits = p.D <= MAX_HEAD_DIM and p.Dv <= MAX_HEAD_DIM
    p.route = _route(native, float_ok, fits, p.group, route, "grouped-query attention")
    return p


class GqaDecodePlan(object):
    __slots__ = ("B", "H", "Hkv", "group", "D", "Dv", "Tmax", "length", "ragged", "append", "keys", "chunks", "splits", "layout",
                 "scale", "q_strides", "knew_strides", "vnew_strides", "kcache_strides", "vcache_strides", "o_strides",
                 "out_shape", "states", "route")

    def geometry(self):
        """B, H, Hkv, len, Tmax, D, Dv in the order tnn_gqa_decode_attn takes them (ragged: without len)."""
        if self.ragged:
            return (self.B, self.H, self.Hkv, self.Tmax, self.D, self.Dv)
        return (self.B, self.H, self.Hkv, self.length, self.Tmax, self.D, self.Dv)

    def strides(self):
        """The six (batch, head, row) element stride triples, flattened: q, k_new, v_new, k_cache, v_cache, o."""
        return (self.q_strides + self.knew_strides + self.vnew_strides + self.kcache_strides + self.vcache_strides
                + self.o_strides)

    def empty(self):
        return self.B * self.H == 0

    def workspace_bytes(self, itemsize):
        """What tnn_gqa_decode_workspace returns: a record (m, l, acc[Dv]) per (b, QUERY head, split), 0 for one split."""
        if self.splits == 1:
            return 0
        return _dc._round16(self.B * self.H * self.splits * (self.Dv + 2) * itemsize)

    def __repr__(self):
        return "GqaDecodePlan(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.__slots__)


def plan_gqa_decode(q_shape, k_cache_shape, v_cache_shape, length=None, append=True, k_new_shape=None, v_new_shape=None,
                    scale=None, layout="bthd", splits=None, lens_shape=None, native=True, float_ok=True, route=None):
    """The plan of gqa_decode.  q [B, H, D]; the caches hold Hkv heads in `layout`; append: k_new [B, Hkv, D] and v_new
    [B, Hkv, Dv] go into row `length`.  Ragged (lens_shape given, length None): lens [B] is read on the device, the grid is
    sized for a cache one row short of full (ragged.plan_ragged_decode's rule) and the append is required."""
    ragged = lens_shape is not None
    what = "gqa_decode"
    if ragged == (length is not None):
        raise ValueError("%s: give length= (a host integer shared by the batch) or lens= (one per sequence), not both" % what)
    if layout not in LAYOUTS:
        raise ValueError("%s: layout must be one of %s, got %r" % (what, LAYOUTS, layout))
    q_shape, k_cache_shape, v_cache_shape = (tuple(int(s) for s in sh) for sh in (q_shape, k_cache_shape, v_cache_shape))
    if len(q_shape) != 3:
        raise ValueError("%s: q must be [B, H, D] (one query per batch and head), got shape %s" % (what, q_shape))
    if len(k_cache_shape) != 4 or len(v_cache_shape) != 4:
        raise ValueError("%s: the caches must have four axes (layout %r), got shapes %s and %s"
                         % (what, layout, k_cache_shape, v_cache_shape))
    tv, hv = (1, 2) if layout == "bthd" else (2, 1)
    p = GqaDecodePlan()
    p.B, p.H, p.D = q_shape
    p.Hkv = k_cache_shape[hv]
    p.group = group_of(p.H, p.Hkv, what)
    p.ragged = ragged
    if ragged:
        if not append or k_new_shape is None or v_new_shape is None:
            raise ValueError("%s: with lens= k_new and v_new are required (the step appends its row)" % what)
        if tuple(int(s) for s in lens_shape) != (p.B,):
            raise ValueError("%s: lens must hold one length per sequence, shape (%d,), got %s" % (what, p.B, tuple(lens_shape)))
        length = max(k_cache_shape[tv] - 1, 0)
    # everything decoding.py checks, the strides of the Hkv-head operands and the split over B Hkv workgroup rows
    try:
        base = _dc.plan_decode((p.B, p.Hkv, p.D), k_cache_shape, v_cache_shape, length, append, k_new_shape, v_new_shape, scale,
                               layout, splits, route="composed")
    except ValueError as exc:
        raise ValueError(str(exc).replace("attention_decode:", what + ":"))
    p.Dv, p.Tmax, p.length, p.append = base.Dv, base.Tmax, (None if ragged else base.length), base.append
    p.keys, p.chunks, p.splits, p.layout, p.scale = base.keys, base.chunks, base.splits, layout, base.scale
    p.knew_strides, p.vnew_strides = base.knew_strides, base.vnew_strides
    p.kcache_strides, p.vcache_strides = base.kcache_strides, base.vcache_strides
    p.q_strides, p.o_strides = (p.H * p.D, p.D, 0), (p.H * p.Dv, p.Dv, 0)
    p.out_shape = (p.B, p.H, p.Dv)
    p.states = next((s for s in DECODE_STATES if s >= p.group), None)
    fits = p.D <= MAX_HEAD_DIM and p.Dv <= MAX_HEAD_DIM
    p.route = _route(native, float_ok, fits, p.group, route, "grouped-query decode attention")
    return p
