"""Host planner of dropout and the reference random generator (numpy only, no device import): from a shape and a rate to ONE
plan — the route, the integer threshold and the scale — and the generator of csrc/tnn_dropout.hip in numpy, bit for bit.

Generator (include/tnn_dropout.h)
    Philox4x32 with 10 rounds, multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85.  The state is
    {uint64 seed, uint64 calls}.  Element i (a 64-bit index) of the stream of one call is word i & 3 of the block with

        counter (lo32(i >> 2), hi32(i >> 2), lo32(calls), hi32(calls))      key (lo32(seed), hi32(seed))

    and every drawing call consumes one value of `calls`.  A draw keeps 24 bits: r = word >> 8.  Dropout KEEPS an element iff
    r >= T with T = round(p 2^24); a uniform number is r 2^-24, exact in float32 and float64 and in [0, 1).

Dropout
    y = keep ? x * s : +0 with s = 1 / (1 - p) rounded once to the operand dtype; the fused residual form adds a residual to
    that, product and sum rounded separately.  The mask is never stored: backward regenerates it from the (seed, calls) ticket
    of its forward.

Routes
    native    csrc/tnn_dropout.hip: a one-thread ticket launch and ONE data launch per call.  Needs the entry points and
              float32 / float64 operands.
    composed  the keep mask from THIS module's generator, uploaded as booleans, then the existing scalar multiply, masked
              select and add.  What runs under the CPU test twin, what `fused=False` layers use, and the second
              implementation the GPU tests compare the kernels with.  Both routes give identical bits and leave the generator
              in the same state.
"""

import numpy as np

ROUNDS = 10               # TNN_RNG_ROUNDS
STATE_BYTES = 16          # TNN_RNG_STATE_BYTES: {uint64 seed, uint64 calls}; a ticket has the same layout
DRAW_BITS = 24            # TNN_RNG_DRAW_BITS: r = word >> (32 - DRAW_BITS)
THREADS = 256             # TNN_DROPOUT_THREADS
VEC = 16                  # TNN_DROPOUT_VEC: bytes per lane of a wide access
MAX_BLOCKS = 2048         # TNN_DROPOUT_MAX_BLOCKS: most workgroups of a data launch
ROUTES = ("native", "composed")

MUL0, MUL1 = 0xD2511F53, 0xCD9E8D57
KEY0, KEY1 = 0x9E3779B9, 0xBB67AE85
_MASK32 = 0xFFFFFFFF
_MASK64 = (1 << 64) - 1
_INT64_MAX = (1 << 63) - 1


class DropoutPlan(object):
    __slots__ = ("shape", "n", "p", "threshold", "scale", "first", "route")

    def grid(self):
        """Workgroups of the native data launch (0: no launch)."""
        if self.n == 0:
            return 0
        blocks = ((self.first + self.n - 1) >> 2) - (self.first >> 2) + 1
        return min((blocks + THREADS - 1) // THREADS, MAX_BLOCKS)

    def __repr__(self):
        return "DropoutPlan(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.__slots__)


def threshold_of(p):
    """T = round(p 2^24) for a rate 0 <= p < 1; an element is kept iff its 24-bit draw is >= T."""
    try:
        p = float(p)
    except (TypeError, ValueError):
        raise ValueError("dropout: p must be a number in [0, 1), got %r" % (p,))
    if not 0.0 <= p < 1.0:               # (NaN fails both comparisons)
        raise ValueError("dropout: p must be in [0, 1), got %r" % (p,))
    t = int(round(p * (1 << DRAW_BITS)))
    if t >= 1 << DRAW_BITS:
        raise ValueError("dropout: p = %r rounds to a threshold of 2^%d — nothing would be kept" % (p, DRAW_BITS))
    return t


def check_stream(first, n):
    first, n = int(first), int(n)
    if first < 0 or n < 0 or first + n > _INT64_MAX:
        raise ValueError("dropout: the stream slice needs first >= 0 and first + n <= 2^63 - 1, got first %d, n %d" % (first, n))
    return first, n


def plan_dropout(shape, p, dtype=np.float32, first=0, native=True, float_ok=True, route=None):
    """The plan of a dropout over an array of `shape` and `dtype`.  native: the library has the entry points; float_ok: the
    operand is (or will be made) float32 / float64; route: force one ("native" / "composed"), None picks."""
    if route is not None and route not in ROUTES:
        raise ValueError("route must be one of %s or None, got %r" % (ROUTES, route))
    plan = DropoutPlan()
    plan.threshold = threshold_of(p)     # (raises for anything that is not a rate in [0, 1))
    plan.p = float(p)
    dtype = np.dtype(dtype)
    is_float = dtype in (np.dtype(np.float32), np.dtype(np.float64))
    can = bool(native) and bool(float_ok) and is_float
    if route == "native" and not can:
        raise ValueError("the native dropout route needs libtnn_hip.so and float32 / float64 operands, got dtype %s" % dtype.name)
    plan.route = route or ("native" if can else "composed")
    plan.shape = tuple(int(s) for s in shape)
    plan.first, plan.n = check_stream(first, int(np.prod(plan.shape, dtype=np.int64)) if plan.shape else 1)
    plan.scale = 1.0 / (1.0 - plan.p)    # a double; each route rounds it ONCE to the operand dtype
    return plan


# ------------------------------------------------------------------------------------------------ the reference generator
def philox4x32_10(counter, key):
    """Philox4x32-10 over arrays of blocks: counter [..., 4] and key [..., 2] (anything that casts to uint32, broadcast
    against each other over the leading axes) -> uint32 [..., 4]."""
    counter = np.asarray(counter, dtype=np.uint64) & np.uint64(_MASK32)
    key = np.asarray(key, dtype=np.uint64) & np.uint64(_MASK32)
    if counter.shape[-1:] != (4,) or key.shape[-1:] != (2,):
        raise ValueError("philox4x32_10: counter [..., 4] and key [..., 2], got %s and %s" % (counter.shape, key.shape))
    lead = np.broadcast_shapes(counter.shape[:-1], key.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(counter[..., i], lead).copy() for i in range(4))
    k0, k1 = (np.broadcast_to(key[..., i], lead).copy() for i in range(2))
    m32, sh = np.uint64(_MASK32), np.uint64(32)
    for _ in range(ROUNDS):                     # (32 x 32 -> 64-bit products fit uint64 exactly)
        p0, p1 = np.uint64(MUL0) * c0, np.uint64(MUL1) * c2
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & m32, (p0 >> sh) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(KEY0)) & m32, (k1 + np.uint64(KEY1)) & m32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def stream_words(seed, calls, first, n):
    """The uint32 words of stream elements first .. first + n - 1 of the call that took the ticket (seed, calls)."""
    first, n = check_stream(first, n)
    seed, calls = int(seed) & _MASK64, int(calls) & _MASK64
    if n == 0:
        return np.zeros(0, dtype=np.uint32)
    blk0, blk1 = first >> 2, (first + n - 1) >> 2
    blocks = (np.uint64(blk0) + np.arange(blk1 - blk0 + 1, dtype=np.uint64))
    counter = np.empty((blocks.size, 4), dtype=np.uint64)
    counter[:, 0] = blocks & np.uint64(_MASK32)
    counter[:, 1] = blocks >> np.uint64(32)
    counter[:, 2] = calls & _MASK32
    counter[:, 3] = calls >> 32
    words = philox4x32_10(counter, np.array([seed & _MASK32, seed >> 32], dtype=np.uint64)).reshape(-1)
    lead = first - (blk0 << 2)
    return words[lead:lead + n]


def draws(seed, calls, first, n):
    """The 24-bit draws r = word >> 8 of the stream slice, uint32."""
    return stream_words(seed, calls, first, n) >> np.uint32(32 - DRAW_BITS)


def keep_mask(seed, calls, first, n, threshold):
    """bool [n]: True where dropout with this integer threshold KEEPS the element."""
    threshold = int(threshold)
    if not 0 <= threshold < 1 << DRAW_BITS:
        raise ValueError("dropout: threshold must be in [0, 2^%d), got %d" % (DRAW_BITS, threshold))
    return draws(seed, calls, first, n) >= np.uint32(threshold)


def uniform(seed, calls, first, n, dtype=np.float32):
    """The uniform numbers r 2^-24 of the stream slice in `dtype` (float32 / float64: exact), in [0, 1)."""
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError("uniform: float32 or float64, got %s" % dtype.name)
    return draws(seed, calls, first, n).astype(dtype) * dtype.type(2.0 ** -DRAW_BITS)


def reference(x, seed, calls, p, residual=None, first=0):
    """The specified result of one dropout call in numpy: keep ? x * s : +0, plus the residual when there is one (product and
    sum rounded separately), in x's dtype."""
    x = np.asarray(x)
    plan = plan_dropout(x.shape, p, x.dtype, first=first, native=False)
    keep = keep_mask(seed, calls, first, x.size, plan.threshold).reshape(x.shape)
    with np.errstate(all="ignore"):
        y = np.where(keep, x * x.dtype.type(plan.scale), x.dtype.type(0))
        if residual is not None:
            y = np.asarray(residual, dtype=x.dtype) + y
    return y
