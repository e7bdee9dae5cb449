"""Host planner of training attention over a RIGHT-PADDED batch (numpy only, no device import): a self-attention batch
(Tq == Tk == T) in which sequence b has lens[b] live tokens, 0 <= lens[b] <= T.  From operand shapes, the shape of `lens`
and the options to ONE plan, on top of the checks, strides and shapes of attention.py (plain heads) and gqa.py (grouped-query
heads), which it wraps.

The rule (include/tnn_varlen.h; one rule at every layer)
    query row i and key row j of batch b are live iff they are < lens[b]
    live query rows attend over the live keys only, under the causal rule of attention.py
    dead rows get o = +0, lse = 0, delta = 0, dq = +0; dead keys get dk = dv = +0; every output element is written
    lens[b] == 0 is legal: an all-zero sequence

Layouts
    "bthd"  q [B, T, H, D], k [B, T, Hkv, D], v [B, T, Hkv, Dv]; Hkv == H for the plain form
    "bhtd"  exactly three axes, q [B, T, D], k [B, T, D], v [B, T, Dv] (plain form only): with more leading axes the batch
            that `lens` counts would be a fold of several, which is refused

Routes
    native    csrc/tnn_varlen.hip: the three launches of attention.py's native route with the lengths read on the DEVICE —
              whole 64-row blocks of padding are skipped, padding is never read (NaN there reaches no output), and the live
              rows of a sequence have the bits of that sequence run alone.  Needs the entry points, float32 / float64
              operands, D, Dv <= MAX_HEAD_DIM and a group <= MAX_GROUP.
    composed  the composed attention of device_array with an additive -inf mask over the dead keys of live rows (dead rows
              stay unmasked: no empty softmax forms) and a row mask that zeroes outputs and gradients of dead rows and dead
              keys; both are built on the host from the lengths.  What runs under the CPU test twin and the second,
              independent implementation the GPU tests compare the kernels with.  It assumes finite padding and raises
              inside an open graph capture.

Out of scope: Tq != Tk and separate query / key lengths, packed (concatenated) sequences, arbitrary masks, bf16, lengths in
the decode, ragged and extend kernels.
"""

import numpy as np

from . import attention as _at
from . import gqa as _gq

MAX_HEAD_DIM = _at.MAX_HEAD_DIM      # TNN_ATTN_MAX_HEAD_DIM
MAX_GROUP = 8                        # TNN_VARLEN_MAX_GROUP (== TNN_GQA_MAX_GROUP)
BLOCK = _at.BLOCK_Q                  # TNN_ATTN_BLOCK_Q == TNN_ATTN_BLOCK_K: the rows a workgroup skips or runs as one
ROUTES = ("native", "composed")
LAYOUTS = ("bthd", "bhtd")


class VarlenPlan(object):
    """The wrapped AttnPlan / GqaAttnPlan (every attribute of it reads through) with the route of THIS family."""
    __slots__ = ("base", "T", "grouped", "route")

    def __getattr__(self, name):
        return getattr(self.base, name)

    def geometry(self):
        """The six extents every native entry point takes, in its argument order (H counts QUERY heads)."""
        b = self.base
        return (b.B, b.H, b.Tq, b.Tk, b.D, b.Dv)

    def __repr__(self):
        return "VarlenPlan(T=%r, grouped=%r, route=%r, base=%r)" % (self.T, self.grouped, self.route, self.base)


def check_lens(host, T, what="attention"):
    """The host values of the lengths: integers in [0, T]."""
    host = np.asarray(host)
    if host.size and (int(host.min()) < 0 or int(host.max()) > T):
        raise ValueError("%s: lens holds a length outside [0, T = %d]: %s" % (what, T, host.tolist()))
    return host


def live_blocks(host, T, causal):
    """(live, total) 64 x 64 score blocks of a batch with these lengths, per head: what the native route's work follows."""
    nb = lambda n: -(-int(n) // BLOCK)
    count = lambda n: nb(n) * (nb(n) + 1) // 2 if causal else nb(n) * nb(n)
    return sum(count(n) for n in np.asarray(host).reshape(-1)), count(T) * int(np.asarray(host).size)


def key_mask(host, T, heads, dtype):
    """[B heads, T, T] additive mask of the composed route: -inf at (live row, dead key), 0 elsewhere."""
    host = np.asarray(host).reshape(-1)
    idx = np.arange(T)
    live = idx[None, :] < host[:, None]                                        # [B, T]
    m = np.where(live[:, :, None] & ~live[:, None, :], -np.inf, 0.0).astype(dtype)
    return np.repeat(m, heads, axis=0)


def row_mask(host, T, heads, dtype):
    """[B heads, T, 1] mask of the composed route: 1 at live rows, 0 at dead ones."""
    host = np.asarray(host).reshape(-1)
    live = (np.arange(T)[None, :] < host[:, None]).astype(dtype)
    return np.repeat(live, heads, axis=0)[:, :, None]


def plan_varlen(q_shape, k_shape, v_shape, lens_shape, causal=False, scale=None, layout="bthd", grouped=False, native=True,
                float_ok=True, route=None):
    """The plan of attention(q, k, v, lens=) (grouped=False) or gqa_attention(q, k, v, lens=) (grouped=True)."""
    what = "gqa_attention" if grouped else "attention"
    if layout not in LAYOUTS:
        raise ValueError("%s: layout must be one of %s, got %r" % (what, LAYOUTS, layout))
    q_shape = tuple(int(s) for s in q_shape)
    if layout == "bhtd" and (grouped or len(q_shape) != 3):
        raise ValueError("%s: with lens= layout \"bhtd\" takes exactly three axes [B, T, D] (the batch that lens counts), got "
                         "q %s" % (what, q_shape))
    if grouped:
        base = _gq.plan_gqa_attention(q_shape, k_shape, v_shape, causal, scale, route="composed")
    else:
        base = _at.plan_attention(q_shape, k_shape, v_shape, causal, scale, layout, route="composed")
    if base.Tq != base.Tk:
        raise ValueError("%s: lens= needs Tq == Tk (a right-padded self-attention batch), got Tq %d, Tk %d"
                         % (what, base.Tq, base.Tk))
    lens_shape = tuple(int(s) for s in lens_shape)
    if lens_shape != (base.B,):
        raise ValueError("%s: lens must have shape (B,) = (%d,), got %s" % (what, base.B, lens_shape))
    p = VarlenPlan()
    p.base, p.T, p.grouped = base, base.Tq, bool(grouped)
    ok = bool(native and float_ok and base.D <= MAX_HEAD_DIM and base.Dv <= MAX_HEAD_DIM and base.group <= MAX_GROUP)
    if route is not None:
        if route not in ROUTES:
            raise ValueError("route must be one of %s or None, got %r" % (ROUTES, route))
        if route == "native" and not ok:
            raise ValueError("the native %s route with lens= needs libtnn_hip.so, float32 / float64 operands, head dimensions "
                             "<= %d and a group <= %d" % (what, MAX_HEAD_DIM, MAX_GROUP))
    p.route = route or ("native" if ok else "composed")
    return p
