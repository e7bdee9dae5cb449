"""Host planner of one autoregressive decoding step (numpy only, no device import): from operand shapes and options to ONE
plan — validated extents, the element strides of every operand, the scale, the key split, the workspace size and the route.

    decode attention    o[b, h, :] = softmax(scale q[b, h, :] k^T) v over the LIVE keys of a cache, one query per (b, h), no
                        mask.  With k_new / v_new the step's own row is written into cache row `length` and the keys are
                        [0, length]; without, the keys are [0, length).  `length` is a host integer shared by the batch.
    sampling            per row of logits [M, V] and one uniform number u in [0, 1): greedy (temperature 0), or the inverse
                        CDF of softmax(x / temperature) restricted to the top_k largest (ties at the threshold: lowest
                        indices first)

Cache layouts (dense arrays; q, k_new, v_new and o are dense [B, H, D] / [B, H, Dv] in both)
    "bthd"  k_cache [B, Tmax, H, D], v_cache [B, Tmax, H, Dv]: what a [B T, H D] projection reshapes to, so a prefill's k and
            v are slice-assigned as they are
    "bhtd"  k_cache [B, H, Tmax, D], v_cache [B, H, Tmax, Dv]: the rows of one (b, h) are contiguous

Key split.  The live keys are cut into chunks of CHUNK; `splits` workgroups per (b, h) take contiguous runs of chunks and a
second launch combines them (csrc/tnn_decode.hip).  One (b, h) per workgroup leaves the machine idle when B H is small, so

    splits = clamp(ceil(TARGET / (B H)), 1, min(chunks, MAX_SPLITS))

Routes
    native    csrc/tnn_decode.hip.  Needs the entry points, float32 / float64 operands and D, Dv <= MAX_HEAD_DIM.
    fwd       decode attention only: the route that existed before — a slice assignment of the new row, then tnn_attn_fwd with
              Tq = 1, non-causal, striding into the cache in place (one workgroup per (b, h)).  Chosen where FWD_RULES says the
              probe found it faster; needs caches below 2^31 elements.
    composed  decode attention: a slice assignment of the new row, then attention() on ITS composed route over the live
              prefix.  Sampling: the logits are read back and the same rule runs in numpy (z in the operand dtype, the rest
              in float64) — a host synchronisation per call, so it cannot be captured into a graph.  What runs under the CPU
              test twin and the second, independent implementation the GPU tests compare the kernels with.

Ragged batches — a length per sequence, read on the device — are ragged.py's (csrc/tnn_ragged.hip), which reuses this planner's
strides and split rule; grouped-query heads are gqa.py's (csrc/tnn_gqa.hip).  T > 1 new rows over a filled cache (chunked
prefill, the bottom-right causal rule) are extend.py's (csrc/tnn_extend.hip).  Out of scope: top-p, bf16.
(u is an operand: generation.generate draws it on the host, or on the device with an rng.Generator.)
"""

import math

import numpy as np

VEC = 16                  # TNN_DECODE_VEC: bytes per lane of a wide access
CHUNK = 64                # TNN_DECODE_CHUNK: keys per chunk
MAX_SPLITS = 256          # TNN_DECODE_MAX_SPLITS: most workgroups per (batch, head)
UNROLL = 4                # TNN_DECODE_UNROLL: keys a lane group has in flight per step
RADIX_BITS = 8            # TNN_SAMPLE_RADIX_BITS: digit of the top-k radix select
SAMPLE_ITEMS = 4          # TNN_SAMPLE_ITEMS: consecutive columns per thread and step of the running-sum scan
MAX_HEAD_DIM = 128        # TNN_ATTN_MAX_HEAD_DIM
MAX_BH = 65536            # B H of one launch stays below this (the second grid axis)
# Workgroups the split aims for, from the sweep of `splits` in profiles/decode_vs_fwd.txt, section (b) (tools/probes/decode_ab.py,
# one MI355X, float32; time against the best split of each shape, by workgroups = B H x splits):
#     workgroups            128     256     512     1024    2048
#     B H 8,  len 4096,  D 128   1.07x   1.00x   1.31x     -       -
#     B H 8,  len 32768, D 128   1.97x   1.23x   1.00x   1.32x   2.01x
#     B H 64, len 4096,  D 64    2.10x   1.32x   1.00x   1.20x   1.33x
# 512 — two workgroups of four waves per CU — is the best of two shapes and has the least worst case (1.31x; 256 and 1024:
# 1.32x).  Beyond it the second launch's walk over the splits and the shorter runs cost more than the extra workgroups gain.
TARGET = 512
ROUTES = ("native", "fwd", "composed")
# Regions that the probe marks SLOWER than the route that existed before tnn_decode_attn go back to that route ("fwd"):
# rules (least B H, most keys) — a plan with B H >= the first and keys <= the second takes it.  Empty: section (a) of
# profiles/decode_vs_fwd.txt marks no shape slower.
FWD_RULES = ()
FWD_LIMIT = 1 << 31       # tnn_attn_fwd refuses a tensor of 2^31 elements or more (include/tnn_attn.h)
LAYOUTS = ("bthd", "bhtd")


def _round16(nbytes):
    return (nbytes + 15) // 16 * 16


def _route(native, float_ok, fits, route, what):
    if route is not None:
        if route not in ROUTES or (route == "fwd" and what != "decode attention"):
            raise ValueError("route must be one of %s or None, got %r" % (ROUTES, route))
        if route == "native" and not (native and float_ok and fits):
            raise ValueError("the native %s route needs libtnn_hip.so, float32 / float64 operands%s"
                             % (what, " and head dimensions <= %d" % MAX_HEAD_DIM if what == "decode attention" else ""))
        return route
    return "native" if native and float_ok and fits else "composed"


def _int(value, what):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise ValueError("%s must be an integer, got %r" % (what, value))
    return int(value)


def choose_splits(bh, chunks):
    """Enough workgroups to cover the CUs: clamp(ceil(TARGET / (B H)), 1, min(chunks, MAX_SPLITS))."""
    return max(1, min(-(-TARGET // max(bh, 1)), chunks, MAX_SPLITS))


class DecodePlan(object):
    __slots__ = ("B", "H", "D", "Dv", "Tmax", "length", "append", "keys", "chunks", "splits", "layout", "scale", "q_strides",
                 "knew_strides", "vnew_strides", "kcache_strides", "vcache_strides", "o_strides", "out_shape", "route")

    def geometry(self):
        """B, H, len, Tmax, D, Dv in the order tnn_decode_attn takes them."""
        return (self.B, self.H, self.length, self.Tmax, self.D, self.Dv)

    def strides(self):
        """The six (batch, head, row) element stride triples, flattened: q, k_new, v_new, k_cache, v_cache, o."""
        return (self.q_strides + self.knew_strides + self.vnew_strides + self.kcache_strides + self.vcache_strides
                + self.o_strides)

    def empty(self):
        return self.B * self.H == 0

    def workspace_bytes(self, itemsize):
        """What tnn_decode_attn_workspace returns: a record (m, l, acc[Dv]) per (b, h, split), 0 for one split."""
        if self.splits == 1:
            return 0
        return _round16(self.B * self.H * self.splits * (self.Dv + 2) * itemsize)

    def runs(self):
        """[(first chunk, end chunk)] of every split: contiguous, ascending, none empty."""
        return [(s * self.chunks // self.splits, (s + 1) * self.chunks // self.splits) for s in range(self.splits)]

    def __repr__(self):
        return "DecodePlan(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.__slots__)


def cache_shape(layout, B, H, Tmax, W):
    if layout not in LAYOUTS:
        raise ValueError("attention_decode: layout must be one of %s, got %r" % (LAYOUTS, layout))
    return (B, Tmax, H, W) if layout == "bthd" else (B, H, Tmax, W)


def plan_decode(q_shape, k_cache_shape, v_cache_shape, length, append=True, k_new_shape=None, v_new_shape=None, scale=None,
                layout="bthd", splits=None, native=True, float_ok=True, route=None):
    """The plan of attention_decode.  q [B, H, D]; the caches in `layout`; append: k_new [B, H, D] and v_new [B, H, Dv] are
    written into row `length`.  splits: force the key split (tests / probes), None picks."""
    if layout not in LAYOUTS:
        raise ValueError("attention_decode: layout must be one of %s, got %r" % (LAYOUTS, layout))
    q_shape, k_cache_shape, v_cache_shape = (tuple(int(s) for s in sh) for sh in (q_shape, k_cache_shape, v_cache_shape))
    if len(q_shape) != 3:
        raise ValueError("attention_decode: q must be [B, H, D] (one query per batch and head), got shape %s" % (q_shape,))
    if len(k_cache_shape) != 4 or len(v_cache_shape) != 4:
        raise ValueError("attention_decode: the caches must have four axes (layout %r), got shapes %s and %s"
                         % (layout, k_cache_shape, v_cache_shape))
    p = DecodePlan()
    p.B, p.H, p.D = q_shape
    p.layout = layout
    tv, hv = (1, 2) if layout == "bthd" else (2, 1)
    p.Tmax, p.Dv = k_cache_shape[tv], v_cache_shape[3]
    if k_cache_shape != cache_shape(layout, p.B, p.H, p.Tmax, p.D):
        raise ValueError("attention_decode: k_cache %s does not match q %s in layout %r" % (k_cache_shape, q_shape, layout))
    if v_cache_shape != cache_shape(layout, p.B, p.H, p.Tmax, p.Dv):
        raise ValueError("attention_decode: v_cache %s does not match k_cache %s" % (v_cache_shape, k_cache_shape))
    if p.D < 1 or p.Dv < 1 or p.Tmax < 1:
        raise ValueError("attention_decode: empty head dimension or cache (q %s, k_cache %s, v_cache %s)"
                         % (q_shape, k_cache_shape, v_cache_shape))
    if p.B * p.H >= MAX_BH:
        raise ValueError("attention_decode: B H = %d must stay below %d" % (p.B * p.H, MAX_BH))
    p.append = bool(append)
    if p.append:
        if k_new_shape is not None and tuple(int(s) for s in k_new_shape) != (p.B, p.H, p.D):
            raise ValueError("attention_decode: k_new must be %s, got %s" % ((p.B, p.H, p.D), tuple(k_new_shape)))
        if v_new_shape is not None and tuple(int(s) for s in v_new_shape) != (p.B, p.H, p.Dv):
            raise ValueError("attention_decode: v_new must be %s, got %s" % ((p.B, p.H, p.Dv), tuple(v_new_shape)))
    p.length = _int(length, "attention_decode: length")
    if p.append and not 0 <= p.length < p.Tmax:
        raise ValueError("attention_decode: the cache is full — length %d of %d rows, no room for the new row"
                         % (p.length, p.Tmax) if p.length == p.Tmax else
                         "attention_decode: length %d outside [0, %d)" % (p.length, p.Tmax))
    if not p.append and not 1 <= p.length <= p.Tmax:
        raise ValueError("attention_decode: without k_new / v_new length must be in [1, %d], got %d" % (p.Tmax, p.length))
    p.keys = p.length + (1 if p.append else 0)
    p.chunks = -(-p.keys // CHUNK)
    most = min(p.chunks, MAX_SPLITS)
    if splits is None:
        p.splits = choose_splits(p.B * p.H, p.chunks)
    else:
        p.splits = _int(splits, "attention_decode: splits")
        if not 1 <= p.splits <= most:
            raise ValueError("attention_decode: splits %d outside [1, %d] (%d chunks of %d keys)" % (p.splits, most, p.chunks, CHUNK))
    if scale is None:
        scale = 1.0 / math.sqrt(p.D)
    p.scale = float(scale)
    if not math.isfinite(p.scale):
        raise ValueError("attention_decode: scale must be finite, got %r" % (scale,))
    single = lambda w: (p.H * w, w, 0)                         # dense [B, H, w]; the row stride is ignored
    cache = lambda w: (p.Tmax * p.H * w, w, p.H * w) if layout == "bthd" else (p.H * p.Tmax * w, p.Tmax * w, w)
    p.q_strides, p.knew_strides, p.vnew_strides, p.o_strides = single(p.D), single(p.D), single(p.Dv), single(p.Dv)
    p.kcache_strides, p.vcache_strides = cache(p.D), cache(p.Dv)
    p.out_shape = (p.B, p.H, p.Dv)
    fits = p.D <= MAX_HEAD_DIM and p.Dv <= MAX_HEAD_DIM
    fwd_ok = p.B * p.Tmax * p.H * max(p.D, p.Dv) < FWD_LIMIT
    if route == "fwd":
        if not (native and float_ok and fits and fwd_ok):
            raise ValueError("the fwd decode attention route needs libtnn_hip.so, float32 / float64 operands, head dimensions "
                             "<= %d and caches below 2^31 elements" % MAX_HEAD_DIM)
        p.route = "fwd"
    else:
        p.route = _route(native, float_ok, fits, route, "decode attention")
        if route is None and p.route == "native" and fwd_ok and any(p.B * p.H >= bh and p.keys <= keys for bh, keys in FWD_RULES):
            p.route = "fwd"
    return p


class SamplePlan(object):
    __slots__ = ("M", "V", "temperature", "top_k", "greedy", "passes", "route")

    def empty(self):
        return self.M == 0

    def __repr__(self):
        return "SamplePlan(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.__slots__)


def plan_sample(logits_shape, u_shape, temperature=1.0, top_k=None, itemsize=4, native=True, float_ok=True, route=None):
    """The plan of sample_rows(logits [M, V], u [M]).  top_k None, 0 or >= V: every column is kept (top_k 0 in the plan);
    temperature 0: greedy, u is not read (u_shape may be None)."""
    logits_shape = tuple(int(s) for s in logits_shape)
    if len(logits_shape) != 2 or logits_shape[1] < 1:
        raise ValueError("sample_rows: the logits must be [M, V] with V >= 1, got shape %s" % (logits_shape,))
    p = SamplePlan()
    p.M, p.V = logits_shape
    if p.V >= 1 << 31:
        raise ValueError("sample_rows: V %d must be below 2^31" % p.V)
    p.temperature = float(temperature)
    if not (math.isfinite(p.temperature) and p.temperature >= 0.0):
        raise ValueError("sample_rows: temperature must be finite and >= 0, got %r" % (temperature,))
    p.greedy = p.temperature == 0.0
    if top_k is None:
        p.top_k = 0
    else:
        p.top_k = _int(top_k, "sample_rows: top_k")
        if p.top_k < 1:
            raise ValueError("sample_rows: top_k must be >= 1 or None, got %d" % p.top_k)
        if p.top_k >= p.V:
            p.top_k = 0
    if not p.greedy:
        if u_shape is None or tuple(int(s) for s in u_shape) != (p.M,):
            raise ValueError("sample_rows: u must hold one number per row, shape (%d,), got %s"
                             % (p.M, None if u_shape is None else tuple(u_shape)))
    p.passes = 0 if p.greedy or p.top_k == 0 else 8 * int(itemsize) // RADIX_BITS
    p.route = _route(native, float_ok, True, route, "sampling")
    return p


def sample_host(logits, u, temperature, top_k):
    """The sampling rule on host arrays: the composed route of sample_rows.  z = x / temperature is formed in the dtype of
    `logits` (so that ties are the ties the kernel sees), everything after it in float64."""
    x = np.asarray(logits)
    M, V = x.shape
    if temperature == 0.0:
        return np.argmax(x, axis=1).astype(np.int64)
    z = (x / x.dtype.type(temperature)).astype(np.float64) + 0.0
    out = np.empty(M, dtype=np.int64)
    uu = np.asarray(u, dtype=np.float64)
    for r in range(M):
        kept = np.ones(V, dtype=bool)
        if top_k and top_k < V:
            order = np.lexsort((np.arange(V), -z[r]))          # descending value, ascending index among equals
            kept[:] = False
            kept[order[:top_k]] = True
        w = np.where(kept, np.exp(z[r] - z[r].max()), 0.0)
        run = np.cumsum(w)
        hit = np.nonzero(kept & (run > uu[r] * run[-1]))[0]
        out[r] = hit[0] if hit.size else np.nonzero(w > 0)[0][-1]
    return out
