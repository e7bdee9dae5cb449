"""Host planner of the two ends of a token model (numpy only, no device import): from operand shapes and options to ONE plan
— validated extents, the kernel form, workspace sizes and the route.

    embedding       out[..., :] = table[ids[...], :] (+ pos[t, :], t the index along the LAST axis of ids)
                    dtable[v, :] = the sum of dy over the positions that hold v (a scatter-ADD: repeated ids accumulate);
                    padding_idx gets a zero gradient row
    cross-entropy   per ROW of logits [..., V]: lse = log sum exp, losses = lse - x[target]; rows whose target is ignore_index
                    count for nothing; loss = sum of losses ("sum") or sum / counted rows ("mean")

Every leading axis folds into M.  ids and targets are integers.

Forms of the cross-entropy (csrc/tnn_token.hip)
    "wave"    V <= XENT_WAVE_MAX_V: one wave owns a row in registers; XENT_ROWS_PER_BLOCK rows per workgroup
    "block"   any wider V: a workgroup streams the row, XENT_BLOCK_STEP float32 columns per step, online max and sum

Routes
    native    csrc/tnn_token.hip.  Needs the entry points and float32 / float64 operands.
    composed  the same mathematics on the array operations that already exist: take, a one-hot product through matmul,
              max / exp / sum / log and a row gather of the flattened logits.  What runs under the CPU test twin, what `fused=False`
              layers use, and the second, independent implementation the GPU tests compare the kernels with.  The composed
              embedding backward builds its one-hot from a HOST copy of the ids: it cannot be captured into a graph.
"""

import math

VEC = 16                      # TNN_TOKEN_VEC: bytes per lane of a wide access
EMBED_SEGMENT = 64            # TNN_EMBED_SEGMENT: K, sorted positions per workgroup of the segmented sum
EMBED_VOCAB_PER_BLOCK = 256   # TNN_EMBED_VOCAB_PER_BLOCK: tokens per placement workgroup
EMBED_WALK_CHUNK = 64         # TNN_EMBED_WALK_CHUNK: ids a placement workgroup ranks per step
XENT_WAVE_MAX_V = 1024        # TNN_XENT_WAVE_MAX_V: widest row of the wave form
XENT_ROWS_PER_BLOCK = 4       # TNN_XENT_ROWS_PER_BLOCK: rows in flight per workgroup of the wave form
XENT_BLOCK_STEP = 4096        # TNN_XENT_BLOCK_STEP: float32 columns per step of the streaming form (float64: half)
ROUTES = ("native", "composed")
REDUCTIONS = ("mean", "sum")
REDUCTION_CODE = {"mean": 0, "sum": 1}        # TNN_XENT_MEAN, TNN_XENT_SUM
LIMIT = 1 << 31               # M and V of the embedding backward are 32-bit in the sort


def _round16(nbytes):
    return (nbytes + 15) // 16 * 16


def _route(native, float_ok, route, what):
    if route is not None:
        if route not in ROUTES:
            raise ValueError("route must be one of %s or None, got %r" % (ROUTES, route))
        if route == "native" and not (native and float_ok):
            raise ValueError("the native %s route needs libtnn_hip.so and float32 / float64 operands" % what)
        return route
    return "native" if native and float_ok else "composed"


def _index(value, what):
    if value is None:
        return -1
    if isinstance(value, bool) or int(value) != value:
        raise ValueError("%s must be an integer or None, got %r" % (what, value))
    return int(value)


class EmbedPlan(object):
    __slots__ = ("M", "V", "E", "T", "has_pos", "padding_idx", "ids_shape", "out_shape", "route")

    def empty(self):
        return self.M == 0

    def segments(self):
        return (self.M + EMBED_SEGMENT - 1) // EMBED_SEGMENT

    def placement_blocks(self):
        return (self.V + EMBED_VOCAB_PER_BLOCK - 1) // EMBED_VOCAB_PER_BLOCK

    def workspace_bytes(self, itemsize):
        """What tnn_embed_bwd_workspace returns: counts [V], offsets [V + 1] and the sorted positions [M] as int32, then two
        partial rows per segment, each part rounded up to 16 bytes."""
        if self.empty():
            return 0
        return (_round16(4 * self.V) + _round16(4 * (self.V + 1)) + _round16(4 * self.M)
                + _round16(2 * self.segments() * self.E * itemsize))

    def __repr__(self):
        return "EmbedPlan(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.__slots__)


def plan_embedding(table_shape, ids_shape, pos_shape=None, padding_idx=None, native=True, float_ok=True, route=None):
    """The plan of table[ids] (+ pos).  table [V, E]; ids any shape (a scalar is one position); pos [T', E] with
    T' >= T = ids_shape[-1]: the first T rows are used."""
    table_shape = tuple(int(s) for s in table_shape)
    ids_shape = tuple(int(s) for s in ids_shape)
    if len(table_shape) != 2 or table_shape[0] < 1 or table_shape[1] < 1:
        raise ValueError("embedding: the table must be [V, E] with V, E >= 1, got shape %s" % (table_shape,))
    p = EmbedPlan()
    p.V, p.E = table_shape
    p.ids_shape, p.out_shape = ids_shape, ids_shape + (p.E,)
    p.M = math.prod(ids_shape)
    p.has_pos = pos_shape is not None
    p.T = 1
    if p.has_pos:
        pos_shape = tuple(int(s) for s in pos_shape)
        if not ids_shape:
            raise ValueError("embedding: positions need ids with at least one axis")
        p.T = ids_shape[-1]
        if len(pos_shape) != 2 or pos_shape[1] != p.E:
            raise ValueError("embedding: pos must be [T, %d], got shape %s" % (p.E, pos_shape))
        if p.T > pos_shape[0]:
            raise ValueError("embedding: %d positions per sequence but pos holds %d rows" % (p.T, pos_shape[0]))
    p.padding_idx = _index(padding_idx, "embedding: padding_idx")
    if padding_idx is not None and not 0 <= p.padding_idx < p.V:
        raise ValueError("embedding: padding_idx %d outside [0, %d)" % (p.padding_idx, p.V))
    if p.M >= LIMIT or p.V >= LIMIT:
        raise ValueError("embedding: M %d and V %d must be below 2^31" % (p.M, p.V))
    p.route = _route(native, float_ok, route, "embedding")
    return p


class XentPlan(object):
    __slots__ = ("M", "V", "ignore_index", "reduction", "rows_shape", "logits_shape", "form", "route")

    def empty(self):
        return self.M == 0

    def rows_per_block(self):
        return XENT_ROWS_PER_BLOCK if self.form == "wave" else 1

    def steps(self, itemsize):
        """Steps of the streaming form over one row (1 for the wave form)."""
        if self.form == "wave":
            return 1
        step = XENT_BLOCK_STEP * 4 // itemsize
        return (self.V + step - 1) // step

    def __repr__(self):
        return "XentPlan(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.__slots__)


def plan_cross_entropy(logits_shape, targets_shape, ignore_index=None, reduction="mean", native=True, float_ok=True, route=None):
    """The plan of the per-row cross-entropy of logits [..., V] with integer targets [...]."""
    logits_shape = tuple(int(s) for s in logits_shape)
    targets_shape = tuple(int(s) for s in targets_shape)
    if len(logits_shape) < 1 or logits_shape[-1] < 1:
        raise ValueError("cross_entropy: the logits need a last axis of at least one class, got shape %s" % (logits_shape,))
    if targets_shape != logits_shape[:-1]:
        raise ValueError("cross_entropy: targets must have shape %s (the logits without their last axis), got %s"
                         % (logits_shape[:-1], targets_shape))
    if reduction not in REDUCTIONS:
        raise ValueError("cross_entropy: reduction must be one of %s, got %r" % (REDUCTIONS, reduction))
    p = XentPlan()
    p.V = logits_shape[-1]
    p.logits_shape, p.rows_shape = logits_shape, targets_shape
    p.M = math.prod(targets_shape)
    p.ignore_index = _index(ignore_index, "cross_entropy: ignore_index")
    if ignore_index is None:
        p.ignore_index = -1                       # (never a valid class: a target of -1 is then simply not counted)
    p.reduction = reduction
    p.form = "wave" if p.V <= XENT_WAVE_MAX_V else "block"
    p.route = _route(native, float_ok, route, "cross-entropy")
    return p
