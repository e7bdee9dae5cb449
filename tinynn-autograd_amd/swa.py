"""Host planner of SLIDING-WINDOW (local) causal training attention (numpy only, no device import): self-attention
(Tq == Tk == T) in which a query sees its last `window` keys.  From operand shapes and the window to ONE plan, on top of the
checks, strides and shapes of attention.py (plain heads) and gqa.py (grouped-query heads), which it wraps.

The rule (include/tnn_swa.h; one rule at every layer)
    key j is kept for query i iff  i - window < j <= i          window >= 1; every query keeps its own key
    window >= T is plain causal attention (natively: bit for bit)

The walk of the native kernels over BLOCK x BLOCK score blocks (csrc/tnn_swa.hip; key_blocks / query_blocks below)
    query block q0 visits key blocks   BLOCK floor(max(0, q0 - window + 1) / BLOCK) .. q0
    key block j0 visits query blocks   j0 .. BLOCK floor(min(T - 1, j0 + window + BLOCK - 2) / BLOCK)
    a block with k0 + BLOCK - 1 <= q0 and k0 >= q0 + BLOCK - window is interior: no mask comparison runs in it

Layouts
    "bthd"  q [B, T, H, D], k [B, T, Hkv, D], v [B, T, Hkv, Dv]; Hkv == H for the plain form
    "bhtd"  q [..., T, D], k [..., T, D], v [..., T, Dv] (plain form only)

Routes
    native    csrc/tnn_swa.hip: three launches whose work follows the band, O(T window).  Needs the entry points, float32
              operands, D, Dv <= MAX_HEAD_DIM and a group <= MAX_GROUP.
    composed  the composed attention of device_array with an additive -inf mask outside the band, built on the host.  What
              float64 and the CPU test twin run, and the second, independent implementation the GPU tests compare the kernels
              with.  It raises inside an open graph capture.

Out of scope: a window over a padded batch (lens=), Tq != Tk, attention sinks, bf16, native float64.
"""

import numpy as np

from . import attention as _at
from . import decoding as _dc
from . import gqa as _gq

MAX_HEAD_DIM = _at.MAX_HEAD_DIM      # TNN_ATTN_MAX_HEAD_DIM
BLOCK = 64                           # TNN_SWA_BLOCK (== TNN_ATTN_BLOCK_Q == TNN_ATTN_BLOCK_K)
MAX_GROUP = 8                        # TNN_SWA_MAX_GROUP (== TNN_GQA_MAX_GROUP)
ROUTES = ("native", "composed")

# (T, window) shapes at which the native route is SLOWER than full causal attention on the MI355X, as predicates over
# (T, window, D, group) with the profile line they come from.  Documentation only — the planner does not consult it, because a
# window changes the result and cannot be routed away; empty: profiles/swa_vs_full.txt shows no such shape
SLOWER_RULES = []


# ---------------------------------------------------------------------- generation: a ring of R = window slots
def ring_slot(pos, R):
    """The slot of the token at position pos."""
    return int(pos) % int(R)


def ring_live(pos, R):
    """The live slots [0, n) once the token at position pos is written: min(pos + 1, R)."""
    return min(int(pos) + 1, int(R))


def ring_rows(n, T, R):
    """The prefill rows of a sequence of n live tokens (of T) that a fill moves, [max(0, n - R), n), and their slots."""
    n = min(max(int(n), 0), int(T))
    rows = np.arange(max(0, n - int(R)), n)
    return rows, rows % int(R)


def choose_splits(bh, R):
    """The splits of a ring decode step from R ALONE (decoding.choose_splits over the ring's chunks of slots): a captured
    step never needs re-planning however long the sequence grows."""
    return _dc.choose_splits(bh, -(-int(R) // _dc.CHUNK))


def check_window(window, what="attention"):
    """The window as a Python int >= 1 (booleans and non-integers are refused)."""
    if isinstance(window, bool) or not isinstance(window, (int, np.integer)):
        raise TypeError("%s: window must be an integer, got %s" % (what, type(window).__name__))
    if window < 1:
        raise ValueError("%s: window must be >= 1 (a query keeps at least its own key), got %d" % (what, window))
    return int(window)


def band_mask(T, W):
    """[T, T] booleans: key j is kept for query i iff i - W < j <= i."""
    i, j = np.arange(T)[:, None], np.arange(T)[None, :]
    return (j <= i) & (j > i - W)


def key_blocks(q0, T, W):
    """The first rows of the key blocks the query block at row q0 visits, ascending."""
    return list(range(BLOCK * (max(0, q0 - W + 1) // BLOCK), min(T, q0 + BLOCK), BLOCK))


def query_blocks(j0, T, W):
    """The first rows of the query blocks the key block at row j0 visits (tnn_swa_bwd_kv), ascending."""
    return list(range(j0, BLOCK * (min(T - 1, j0 + W + BLOCK - 2) // BLOCK) + 1, BLOCK))


def interior(q0, k0, W):
    """Every (query, key) pair of the block pair is kept: the block runs without a mask comparison."""
    return k0 + BLOCK - 1 <= q0 and k0 >= q0 + BLOCK - W


def visited_blocks(T, W):
    """(band, causal) score blocks per head: what the native route's time is expected to follow."""
    starts = range(0, T, BLOCK)
    return sum(len(key_blocks(q0, T, W)) for q0 in starts), sum(q0 // BLOCK + 1 for q0 in starts)


class SwaPlan(object):
    """The wrapped AttnPlan / GqaAttnPlan (every attribute of it reads through) with the window and the route of THIS family."""
    __slots__ = ("base", "T", "window", "grouped", "route")

    def __getattr__(self, name):
        return getattr(self.base, name)

    def geometry(self):
        """The five extents every native entry point takes, in its argument order (H counts QUERY heads)."""
        b = self.base
        return (b.B, b.H, b.Tq, b.D, b.Dv)

    def __repr__(self):
        return "SwaPlan(T=%r, window=%r, grouped=%r, route=%r, base=%r)" % (self.T, self.window, self.grouped, self.route, self.base)


def plan_swa(q_shape, k_shape, v_shape, window, causal=True, scale=None, layout="bthd", grouped=False, native=True,
             float_ok=True, route=None):
    """The plan of attention(q, k, v, window=) (grouped=False) or gqa_attention(q, k, v, window=) (grouped=True)."""
    what = "gqa_attention" if grouped else "attention"
    window = check_window(window, what)
    if not causal:
        raise ValueError("%s: window= needs causal=True (the window reaches back from the query's own position)" % what)
    if grouped:
        base = _gq.plan_gqa_attention(q_shape, k_shape, v_shape, True, scale, route="composed")
    else:
        base = _at.plan_attention(q_shape, k_shape, v_shape, True, scale, layout, route="composed")
    if base.Tq != base.Tk:
        raise ValueError("%s: window= needs Tq == Tk (self-attention), got Tq %d, Tk %d" % (what, base.Tq, base.Tk))
    p = SwaPlan()
    p.base, p.T, p.window, p.grouped = base, base.Tq, window, bool(grouped)
    ok = bool(native and float_ok and base.D <= MAX_HEAD_DIM and base.Dv <= MAX_HEAD_DIM and base.group <= MAX_GROUP)
    if route is not None:
        if route not in ROUTES:
            raise ValueError("route must be one of %s or None, got %r" % (ROUTES, route))
        if route == "native" and not ok:
            raise ValueError("the native %s route with window= needs libtnn_hip.so, float32 operands, head dimensions <= %d "
                             "and a group <= %d" % (what, MAX_HEAD_DIM, MAX_GROUP))
    p.route = route or ("native" if ok else "composed")
    return p
