"""Host planner of the fused linear + cross-entropy of a vocabulary head (numpy only, no device import): from operand shapes
and options to ONE plan per call — validated extents, the row and vocabulary blocks, the split of the vocabulary over
workgroups, the rows per backward chunk, the workspace size, the route.

    z = h w + b        h [.., K] (leading axes fold into M), w [K, V] as Dense stores it, b [V] / [1, V] or None
    loss               per row lse - z[target], summed ("sum") or averaged over the counted rows ("mean"), with the
                       ignore_index and out-of-range rules of tokens.plan_cross_entropy

Routes
    native    csrc/tnn_lce.hip (include/tnn_lce.h).  Forward: tnn_lce_fwd, no [M, V] quantity is written.  Backward: rows in
              ascending chunks of `chunk_rows`; tnn_lce_dlogits fills a chunk buffer [chunk_rows, V] and the library's GEMMs
              turn it into dh, dw and db (beta = 1 from the second chunk on), so the result is a pure function of the extents
              and chunk_rows.  float32 only.
    composed  ops.dense_ followed by cross_entropy_ over whole logits.  What runs under the CPU test twin, for float64, with
              fused=False, and the second, independent implementation the GPU tests compare the kernels with.

SLOWER_RULES lists the region in which the probe (tools/probes/lce_ab.py, profiles/lce_vs_composed.txt) found the fused op
SLOWER than dense_ + cross_entropy_ — every shape it measured: the op is there for the memory, and expect_slower() tells a
caller who wants speed alone.  Out of scope: bf16, a weight stored [V, K] or tied to the embedding,
label smoothing, z-loss, float64 on the native route.
"""

import math

from . import tokens as _tk

WAVES = 4                 # TNN_LCE_WAVES
WAVE_ROWS = 16            # TNN_LCE_WAVE_ROWS
BLOCK_M = 64              # TNN_LCE_BLOCK_M: rows per workgroup
BLOCK_V = 256             # TNN_LCE_BLOCK_V: columns per vocabulary block
KC = 16                   # TNN_LCE_KC: k values per staged chunk
MAX_SPLITS = 64           # TNN_LCE_MAX_SPLITS
ROUTES = ("native", "composed")
CUS = 256                 # compute units of one MI355X: what choose_splits fills
WORKGROUPS_PER_CU = 2     # ... and how many workgroups per unit it aims at (42 KiB of LDS each: two fit)
# most bytes of the backward's chunk buffer [chunk_rows, V].  profiles/lce_vs_composed.txt, section (c), forward + backward at
# M 8192, K 1024: 16 / 64 / 256 / 1024 MiB take 29.6 / 21.0 / 19.0 / 18.9 ms at V 32768 and 143 / 109 / 84 / 76 ms at V 131072
# (the GEMMs of a chunk of 64 or 128 rows are skinny).  256 MiB is where the curve flattens at V 32768 and still a quarter of
# that shape's logits; section (a) of the file was measured with 64 MiB.
CHUNK_BYTES = 256 << 20
LIMIT = 1 << 31           # M and V are below this; M V need not be
# (most M V, most K): ops.linear_cross_entropy_ with M V <= the first and K <= the second is SLOWER than dense_ + cross_entropy_ —
# profiles/lce_vs_composed.txt, section (a): at EVERY measured shape (M 2048 and 8192, K 512 .. 4096, V 4096 .. 131072) the
# forward takes 1.2x .. 1.4x the composed forward's time (the 16x16x4 MFMA tile walk reaches 102 TFLOP/s at 8192 x 4096 x 32768
# against the GEMM's 139) and forward + backward 1.3x .. 2.2x (four GEMM-sized passes against three, and skinny chunk GEMMs).
# It never holds the logits or their gradient there.  Nothing beyond these extents was measured.
SLOWER_RULES = ((8192 * 131072, 4096),)


def expect_slower(M, K, V):
    """Whether SLOWER_RULES marks the shape: the fused op then costs more time than the composed one (it still saves the
    2 M V floats of the logits and their gradient)."""
    return any(M * V <= most_mv and K <= most_k for most_mv, most_k in SLOWER_RULES)


def row_blocks(M):
    return -(-M // BLOCK_M)


def vocab_blocks(V):
    return -(-V // BLOCK_V)


def most_splits(V):
    return max(1, min(vocab_blocks(V), MAX_SPLITS))


def choose_splits(M, V):
    """Runs the vocabulary blocks are cut into: enough to put WORKGROUPS_PER_CU workgroups on every unit given the row blocks,
    never more than there are vocabulary blocks (or MAX_SPLITS); a pure function of the extents, so a repeated call merges in
    the same order.  profiles/lce_vs_composed.txt, section (b): at K 1024, V 32768 the best of 1 .. 64 was 16 at M 2048 (1.54
    ms against 14.8 with one) and 4 at M 8192, and 16 at M 2048, V 4096 — what this gives."""
    want = -(-CUS * WORKGROUPS_PER_CU // row_blocks(M))
    return max(1, min(want, most_splits(V)))


def split_range(V, splits, s):
    """The vocabulary blocks [first, stop) of split s."""
    nvb = vocab_blocks(V)
    return s * nvb // splits, (s + 1) * nvb // splits


def workspace_bytes(M, splits):
    """What tnn_lce_fwd_workspace returns: a (max, sum) pair per row and split and the target's logit per row."""
    return 0 if splits == 1 else -(-(2 * splits + 1) * M * 4 // 16) * 16


def choose_chunk_rows(M, V, chunk_bytes=None):
    """Rows per backward chunk: as many as keep chunk_rows V 4 bytes under CHUNK_BYTES, a multiple of BLOCK_M, at least
    BLOCK_M, and no more than M rounded up to BLOCK_M."""
    budget = CHUNK_BYTES if chunk_bytes is None else int(chunk_bytes)
    rows = max(BLOCK_M, budget // (4 * V) // BLOCK_M * BLOCK_M)
    return min(rows, row_blocks(M) * BLOCK_M)


class LcePlan(object):
    __slots__ = ("M", "K", "V", "bias", "ignore_index", "reduction", "rows_shape", "row_blocks", "vocab_blocks", "splits",
                 "chunk_rows", "route")

    def empty(self):
        return self.M == 0

    def workspace_bytes(self):
        return workspace_bytes(self.M, self.splits)

    def chunks(self):
        """(first row, rows) of every backward chunk, ascending."""
        return [(m0, min(self.chunk_rows, self.M - m0)) for m0 in range(0, self.M, self.chunk_rows)]

    def chunk_elements(self):
        """Elements of the chunk buffer; a Python integer: min(chunk_rows, M) V may exceed 2^31."""
        return min(self.chunk_rows, self.M) * self.V

    def logits_elements(self):
        """M V, what the composed route writes twice; a Python integer."""
        return self.M * self.V

    def __repr__(self):
        return "LcePlan(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.__slots__)


def plan_linear_cross_entropy(h_shape, w_shape, b_shape, targets_shape, ignore_index=None, reduction="mean", splits=None,
                              chunk_rows=None, native=True, float_ok=True, route=None):
    """The plan of the loss of h [.., K] through w [K, V] (+ b) against integer targets [..]."""
    what = "linear_cross_entropy"
    h_shape, w_shape = tuple(int(s) for s in h_shape), tuple(int(s) for s in w_shape)
    targets_shape = tuple(int(s) for s in targets_shape)
    if len(w_shape) != 2 or w_shape[0] < 1 or w_shape[1] < 1:
        raise ValueError("%s: w must be [K, V] with K, V >= 1, got shape %s" % (what, w_shape))
    p = LcePlan()
    p.K, p.V = w_shape
    if len(h_shape) < 1 or h_shape[-1] != p.K:
        raise ValueError("%s: h must be [.., K] = [.., %d], got shape %s" % (what, p.K, h_shape))
    if targets_shape != h_shape[:-1]:
        raise ValueError("%s: targets must have shape %s (h without its last axis), got %s" % (what, h_shape[:-1], targets_shape))
    if b_shape is not None and math.prod(tuple(int(s) for s in b_shape)) != p.V:
        raise ValueError("%s: b must hold V = %d elements, got shape %s" % (what, p.V, tuple(b_shape)))
    if reduction not in _tk.REDUCTIONS:
        raise ValueError("%s: reduction must be one of %s, got %r" % (what, _tk.REDUCTIONS, reduction))
    p.M, p.rows_shape, p.bias, p.reduction = math.prod(targets_shape), targets_shape, b_shape is not None, reduction
    if p.M >= LIMIT or p.V >= LIMIT:
        raise ValueError("%s: M %d and V %d must be below 2^31 (their product need not be)" % (what, p.M, p.V))
    p.ignore_index = -1 if ignore_index is None else _tk._index(ignore_index, what + ": ignore_index")
    p.row_blocks, p.vocab_blocks = row_blocks(p.M), vocab_blocks(p.V)
    if route is not None and route not in ROUTES:
        raise ValueError("route must be one of %s or None, got %r" % (ROUTES, route))
    ok = native and float_ok and p.M >= 1
    if route == "native" and not ok:
        raise ValueError("the native linear + cross-entropy route needs libtnn_hip.so, float32 operands and at least one row")
    p.route = route or ("native" if ok else "composed")
    if splits is None:
        p.splits = choose_splits(max(p.M, 1), p.V)
    else:
        p.splits = int(splits)
        if not 1 <= p.splits <= most_splits(p.V):
            raise ValueError("%s: splits %d outside [1, %d] (%d vocabulary blocks)" % (what, p.splits, most_splits(p.V), p.vocab_blocks))
    if chunk_rows is None:
        p.chunk_rows = choose_chunk_rows(max(p.M, 1), p.V)
    else:
        p.chunk_rows = int(chunk_rows)
        if p.chunk_rows < BLOCK_M or p.chunk_rows % BLOCK_M:
            raise ValueError("%s: chunk_rows %d must be a positive multiple of %d" % (what, p.chunk_rows, BLOCK_M))
    return p
