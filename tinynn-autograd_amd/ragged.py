"""Host planner of the RAGGED decoding step (numpy only, no device import): every sequence of a batch has its own length, and
the lengths live on the device (include/tnn_ragged.h), so the launches of a token step take the same arguments every step.

    decode attention    sequence b appends its row at cache row lens[b] and attends over keys [0, lens[b]]; lens is a DEVICE
                        int64 [B].  A sequence with lens[b] outside [0, Tmax) gives zeros and leaves its caches untouched.
    advance             the step's bookkeeping per sequence (advance_host states it): lens + 1, the id into the output, the
                        end-of-sequence flag, the next step's uniform number
    embedding_at        out[m] = table[ids[m]] + pos[positions[m]]: every sequence sits at its own position

Key split.  The host cannot see lens, so the grid depends on the SHAPES alone:

    splits = choose_splits(B H, ceil(Tmax / CHUNK))          (decoding.choose_splits)

workgroups per (b, h); a workgroup derives chunks_b = ceil((lens[b] + 1) / CHUNK) itself and owns chunks
[s chunks_b / splits, (s + 1) chunks_b / splits).  The non-empty ones of these runs are exactly the runs of
min(splits, chunks_b) splits (live_runs), so a batch of uniform lengths gets, at every step, the split decoding.plan_decode
would pick for it: min(ceil(TARGET / (B H)), chunks_now, MAX_SPLITS).  A captured step keeps its grid.

Routes
    native    csrc/tnn_ragged.hip.  Needs the entry points, float32 / float64 operands and D, Dv <= MAX_HEAD_DIM.
    composed  a loop over the sequences that calls the composed attention_decode on batch slices with the HOST MIRROR of the
              lengths; two row gathers and an addition; the advance in numpy, uploaded.  What runs under the CPU test twin; it
              cannot be captured into a graph.

Lengths carries the device array together with its host mirror: every sequence advances by one per step (a finished one emits
the pad token), so lens[b] = start[b] + steps taken - 1 and the host follows without a read-back.
"""

import numpy as np

from . import decoding as _dc

ROUTES = ("native", "composed")


class Lengths(object):
    """lens [B] on the device (`dev`: whatever array type the caller uses) and its host mirror (`host`: numpy int64 [B])."""
    __slots__ = ("dev", "host")

    def __init__(self, dev, host):
        self.dev = dev
        self.host = np.array(host, dtype=np.int64).reshape(-1)

    @property
    def shape(self):
        return self.host.shape


class RaggedDecodePlan(object):
    __slots__ = ("B", "H", "D", "Dv", "Tmax", "chunks", "splits", "layout", "scale", "base", "out_shape", "route")

    def geometry(self):
        """B, H, Tmax, D, Dv in the order tnn_ragged_decode_attn takes them."""
        return (self.B, self.H, self.Tmax, self.D, self.Dv)

    def strides(self):
        return self.base.strides()

    def empty(self):
        return self.B * self.H == 0

    def workspace_bytes(self, itemsize):
        return self.base.workspace_bytes(itemsize)

    def __repr__(self):
        return "RaggedDecodePlan(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.__slots__ if k != "base")


def live_runs(chunks_b, splits):
    """[(first chunk, end chunk)] of the workgroups of one sequence that get keys, in split order."""
    runs = [(s * chunks_b // splits, (s + 1) * chunks_b // splits) for s in range(splits)]
    return [r for r in runs if r[1] > r[0]]


def effective_splits(length, splits):
    """The `splits` of the uniform kernel that a sequence holding `length` cached rows is bit-equal to."""
    return min(splits, -(-(length + 1) // _dc.CHUNK))


def plan_ragged_decode(q_shape, k_cache_shape, v_cache_shape, lens_shape, k_new_shape=None, v_new_shape=None, scale=None,
                       layout="bthd", splits=None, native=True, float_ok=True, route=None):
    """The plan of attention_decode_ragged.  q [B, H, D]; the caches in `layout`; lens [B]; k_new [B, H, D], v_new [B, H, Dv].
    splits: force the grid's split (tests / probes), None picks from the shapes."""
    if route is not None and route not in ROUTES:
        raise ValueError("attention_decode_ragged: route must be one of %s or None, got %r" % (ROUTES, route))
    try:        # the shapes, the strides and the split of a decode step over a cache that is one row short of full
        tmax = int(k_cache_shape[1 if layout == "bthd" else 2]) if len(tuple(k_cache_shape)) == 4 else 1
        base = _dc.plan_decode(q_shape, k_cache_shape, v_cache_shape, max(tmax - 1, 0), True, k_new_shape, v_new_shape, scale,
                               layout, splits, route="composed")
    except ValueError as exc:
        raise ValueError(str(exc).replace("attention_decode:", "attention_decode_ragged:"))
    p = RaggedDecodePlan()
    p.base = base
    p.B, p.H, p.D, p.Dv, p.Tmax = base.B, base.H, base.D, base.Dv, base.Tmax
    if tuple(int(s) for s in lens_shape) != (p.B,):
        raise ValueError("attention_decode_ragged: lens must hold one length per sequence, shape (%d,), got %s"
                         % (p.B, tuple(lens_shape)))
    p.chunks, p.splits, p.layout, p.scale, p.out_shape = base.chunks, base.splits, layout, base.scale, base.out_shape
    fits = p.D <= _dc.MAX_HEAD_DIM and p.Dv <= _dc.MAX_HEAD_DIM
    if route == "native" and not (native and float_ok and fits):
        raise ValueError("the native ragged decode attention route needs libtnn_hip.so, float32 / float64 operands and head "
                         "dimensions <= %d" % _dc.MAX_HEAD_DIM)
    p.route = route or ("native" if native and float_ok and fits else "composed")
    return p


def pick_route(native, route, what):
    if route is not None and route not in ROUTES:
        raise ValueError("%s: route must be one of %s or None, got %r" % (what, ROUTES, route))
    if route == "native" and not native:
        raise ValueError("the native %s route needs libtnn_hip.so" % what)
    return route or ("native" if native else "composed")


def check_advance(picked, lens, start, done, out, cur, u_all, u_cur):
    """Shapes of ragged_advance's operands -> (B, Tout, N)."""
    if len(out) != 2:
        raise ValueError("ragged_advance: out must be [B, Tout], got shape %s" % (tuple(out),))
    B, Tout = (int(s) for s in out)
    for name, shape in (("picked", picked), ("lens", lens), ("start", start), ("done", done), ("cur", cur)):
        if tuple(int(s) for s in shape) != (B,):
            raise ValueError("ragged_advance: %s must have shape (%d,), got %s" % (name, B, tuple(shape)))
    if Tout < 1:
        raise ValueError("ragged_advance: out must hold at least one column")
    if (u_all is None) != (u_cur is None):
        raise ValueError("ragged_advance: u_all and u_cur come together or not at all")
    N = 0
    if u_all is not None:
        if len(u_all) != 2 or int(u_all[1]) != B or tuple(int(s) for s in u_cur) != (B,):
            raise ValueError("ragged_advance: u_all must be [N, %d] and u_cur (%d,), got %s and %s"
                             % (B, B, tuple(u_all), tuple(u_cur)))
        N = int(u_all[0])
    return B, Tout, N


def advance_host(picked, lens, start, done, out, cur, u_all=None, u_cur=None, eos=-1, pad=0):
    """The rule of tnn_ragged_advance on numpy arrays, IN PLACE (the composed route)."""
    B, Tout = out.shape
    N = 0 if u_all is None else u_all.shape[0]
    for b in range(B):
        L = int(lens[b]) + 1
        lens[b] = L
        tok = pad if done[b] else int(picked[b])
        if 0 <= L < Tout:
            out[b, L] = tok
        cur[b] = tok
        if eos >= 0 and tok == eos:
            done[b] = 1
        n = L + 1 - int(start[b])
        if u_all is not None and 0 <= n < N:
            u_cur[b] = u_all[n, b]


def generated_lengths(ids, start, new, eos):
    """[B]: the prompt plus the new tokens up to and including the first end-of-sequence token (all `new` without one)."""
    out = np.empty(len(start), dtype=np.int64)
    for b, p in enumerate(start):
        row = np.asarray(ids[b, p:p + new])
        hit = np.nonzero(row == eos)[0] if eos is not None and eos >= 0 else ()
        out[b] = p + (int(hit[0]) + 1 if len(hit) else new)
    return out
