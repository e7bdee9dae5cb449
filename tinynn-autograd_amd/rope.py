"""Host planner of the rotary position embedding (numpy only, no device import): from operand shapes and options to ONE
plan, in the style of gqa.py and norm.py, plus the host tables and the numpy evaluation of the rotation.

    contract    x viewed as [B, T, H, D], rotary width R (even, 2 <= R <= D), table length P.  cos_t[p, i], sin_t[p, i]
                (0 <= p < P, 0 <= i < R / 2) are the cosine and sine of p * base^(-2 i / R), dense [P, R / 2] in the operand
                dtype: computed HERE, in numpy.longdouble (the angle included), and rounded once — the device evaluates no
                trigonometric function.  Pairing "half": element i pairs with i + R / 2; "interleaved": 2 i with 2 i + 1.
                For a pair (x_lo, x_hi) at position p:  y_lo = x_lo c - x_hi s,  y_hi = x_hi c + x_lo s;  elements [R, D)
                are copied.  inverse: s -> -s; the vjp of the rotation is the inverse rotation of the gradient.
    positions   row (b, t) sits at offset + t (a host integer), or at positions[b], a device int64 [B] array read by the
                kernel (T == 1 and offset == 0 then; a position outside [0, P) gives a row of zeros).
    layouts     "bthd": [B, T, H, D] (what a [B T, H D] projection reshapes to) or "bhtd": [B, H, T, D]; the kernel takes
                strides, nothing is transposed.  Up to two tensors (q and k: equal B, T and D, any head counts) per call.

Routes
    native    csrc/tnn_rope.hip: ONE tnn_rope_apply launch for both tensors.  Needs the entry point and float32 / float64.
    composed  slice reads, products and slice assignments on the array operations that exist; the device-position form reads
              the host mirror of the positions per sequence and cannot be captured.  What runs under the CPU test twin and
              the second, independent implementation the GPU tests compare the kernel with.

Wide or element accesses (include/tnn_rope.h states the rule; `wide_access` is its one Python copy): every base address
VEC-byte aligned, every stride a multiple of V = VEC / itemsize, and R / 2 (interleaved: R) a multiple of V.

Out of scope: position interpolation and NTK / YaRN scaling, bf16, fusing the rotation into the attention kernels, growing a
Rotary's tables after first use.
"""

import math

import numpy as np

VEC = 16                  # TNN_ROPE_VEC
THREADS = 256             # TNN_ROPE_THREADS
MAX_BLOCKS = 2048         # TNN_ROPE_MAX_BLOCKS
PAIRINGS = ("half", "interleaved")            # TNN_ROPE_HALF, TNN_ROPE_INTERLEAVED: the index is the code
LAYOUTS = ("bthd", "bhtd")
ROUTES = ("native", "composed")


def default_rotary_dim(D):
    """The largest even number <= D."""
    return int(D) - int(D) % 2


def check_rotary_dim(R, D=None, what="rope"):
    R = int(R)
    if R < 2 or R % 2 or (D is not None and R > int(D)):
        raise ValueError("%s: the rotary width must be even with 2 <= R%s, got %d"
                         % (what, "" if D is None else " <= D = %d" % int(D), R))
    return R


def tables(max_len, rotary_dim, base=10000.0, dtype=np.float32):
    """(cos_t, sin_t), dense [max_len, rotary_dim / 2] in `dtype`: the frequencies base^(-2 i / R), the angles p * frequency
    and their cosine and sine all in numpy.longdouble, rounded to `dtype` once."""
    P, R = int(max_len), check_rotary_dim(rotary_dim, what="rope.tables")
    if P < 1:
        raise ValueError("rope.tables: max_len must be >= 1, got %d" % P)
    if not float(base) > 0.0 or not np.isfinite(float(base)):
        raise ValueError("rope.tables: base must be a positive finite number, got %r" % (base,))
    ld = np.longdouble
    i = np.arange(R // 2).astype(ld)
    freq = np.power(ld(base), -(2 * i) / ld(R))
    angle = np.arange(P).astype(ld)[:, None] * freq[None, :]
    dtype = np.dtype(dtype)
    return np.ascontiguousarray(np.cos(angle).astype(dtype)), np.ascontiguousarray(np.sin(angle).astype(dtype))


def view_strides(layout, shape):
    """The (b, t, h) element strides of a dense array of `shape` in `layout`."""
    if layout == "bthd":
        _, t, h, d = shape
        return (t * h * d, h * d, d)
    _, h, t, d = shape
    return (h * t * d, d, t * d)


def wide_access(pairing, R, itemsize, strides, addresses):
    """include/tnn_rope.h's rule: True when the kernel takes 16-byte accesses.  addresses: the base addresses that exist."""
    v = VEC // int(itemsize)
    if (R // 2 if pairing == "half" else R) % v:
        return False
    return all(int(s) % v == 0 for s in strides) and all(int(a) % VEC == 0 for a in addresses)


def choose_blocks(items):
    """The library's choice of workgroups for `items` work items (blocks == 0)."""
    return max(1, min(-(-int(items) // THREADS), MAX_BLOCKS))


class RopePlan(object):
    __slots__ = ("B", "T", "Ha", "Hb", "D", "R", "P", "offset", "device_positions", "layout", "pairing", "inverse", "blocks",
                 "a_strides", "b_strides", "a_shape", "b_shape", "in_place", "wide", "items", "grid", "route")

    def geometry(self):
        """B, T, Ha, Hb, D, R, P in the order tnn_rope_apply's geometry array holds them."""
        return (self.B, self.T, self.Ha, self.Hb, self.D, self.R, self.P)

    def strides(self):
        """The twelve (b, t, h) element strides of xa, ya, xb, yb (outputs are dense arrays of the inputs' shapes)."""
        return self.a_strides * 2 + self.b_strides * 2

    def pairing_code(self):
        return PAIRINGS.index(self.pairing)

    def empty(self):
        return self.B * self.T * (self.Ha + self.Hb) == 0

    def __repr__(self):
        return "RopePlan(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.__slots__)


def _split(layout, shape):
    if layout == "bthd":
        b, t, h, d = shape
    else:
        b, h, t, d = shape
    return b, t, h, d


def _overlap(a, b):
    return a is not None and b is not None and a[0] < b[0] + b[1] and b[0] < a[0] + a[1]


def plan_rope(a_shape, b_shape=None, rotary_dim=None, max_len=None, offset=0, positions_shape=None, layout="bthd",
              pairing="half", inverse=False, blocks=0, itemsize=4, addresses=None, native=True, float_ok=True, route=None):
    """The plan of rope(xa[, xb]).  Shapes: [B, T, H, D] ("bthd") or [B, H, T, D] ("bhtd"); the two tensors agree in B, T and
    D.  rotary_dim None: the largest even number <= D.  max_len: the table length P.  positions_shape: the shape of the
    device positions (then T == 1 and offset == 0), None for `offset`.  blocks: 0 (the library's choice) or 1 .. MAX_BLOCKS.
    addresses: None, or the base addresses (xa, ya, xb, yb, cos_t, sin_t) — None for one that does not exist yet (a fresh
    output: disjoint and aligned); ya may equal xa (in place), every other overlap of an output raises.  Every check runs
    before any launch."""
    what = "rope"
    if layout not in LAYOUTS:
        raise ValueError("%s: layout must be one of %s, got %r" % (what, LAYOUTS, layout))
    if pairing not in PAIRINGS:
        raise ValueError("%s: pairing must be one of %s, got %r" % (what, PAIRINGS, pairing))
    a_shape = tuple(int(s) for s in a_shape)
    b_shape = None if b_shape is None else tuple(int(s) for s in b_shape)
    if len(a_shape) != 4 or (b_shape is not None and len(b_shape) != 4):
        raise ValueError("%s: the operands are [B, T, H, D] (layout \"bthd\") or [B, H, T, D] (\"bhtd\"), got shapes %s and %s"
                         % (what, a_shape, b_shape))
    p = RopePlan()
    p.layout, p.pairing, p.inverse = layout, pairing, bool(inverse)
    p.B, p.T, p.Ha, p.D = _split(layout, a_shape)
    p.Hb = 0
    if b_shape is not None:
        bb, tb, p.Hb, db = _split(layout, b_shape)
        if (bb, tb, db) != (p.B, p.T, p.D):
            raise ValueError("%s: the two tensors must agree in B, T and D, got shapes %s and %s (layout %r)"
                             % (what, a_shape, b_shape, layout))
    if p.D < 1:
        raise ValueError("%s: the head dimension must be >= 1, got shape %s" % (what, a_shape))
    p.R = check_rotary_dim(default_rotary_dim(p.D) if rotary_dim is None else rotary_dim, p.D, what)
    if max_len is None or int(max_len) < 1:
        raise ValueError("%s: the table length max_len must be >= 1, got %r" % (what, max_len))
    p.P = int(max_len)
    p.offset = int(offset)
    p.device_positions = positions_shape is not None
    if p.device_positions:
        if p.T != 1 or p.offset != 0:
            raise ValueError("%s: device positions need T == 1 and offset == 0, got T = %d and offset = %d"
                             % (what, p.T, p.offset))
        if tuple(int(s) for s in positions_shape) != (p.B,):
            raise ValueError("%s: positions must hold one position per sequence, shape (%d,), got %s"
                             % (what, p.B, tuple(positions_shape)))
    elif p.offset < 0 or p.offset + p.T > p.P:
        raise ValueError("%s: positions %d .. %d lie outside the table's max_len %d" % (what, p.offset, p.offset + p.T - 1, p.P))
    p.blocks = int(blocks)
    if not 0 <= p.blocks <= MAX_BLOCKS:
        raise ValueError("%s: blocks must be 0 (the library's choice) or 1 .. %d, got %d" % (what, MAX_BLOCKS, p.blocks))
    p.a_shape, p.b_shape = a_shape, b_shape
    p.a_strides = view_strides(layout, a_shape)
    p.b_strides = view_strides(layout, b_shape) if b_shape is not None else (0, 0, 0)
    # overlap: an output may be exactly its own input, nothing else may share bytes with an output
    p.in_place = (False, False)
    known = []
    if addresses is not None:
        xa, ya, xb, yb, ct, st = (None if a is None else int(a) for a in addresses)
        na = math.prod(a_shape) * itemsize
        nb = 0 if b_shape is None else math.prod(b_shape) * itemsize
        nt = p.P * (p.R // 2) * itemsize
        span = lambda addr, n: None if addr is None or n == 0 else (addr, n)
        sxa, sya, sxb, syb, sct, sst = span(xa, na), span(ya, na), span(xb, nb), span(yb, nb), span(ct, nt), span(st, nt)
        p.in_place = (sya is not None and ya == xa, syb is not None and yb == xb)
        if _overlap(sya, sxa) and not p.in_place[0] or _overlap(syb, sxb) and not p.in_place[1]:
            raise ValueError("%s: an output overlaps its input without being it (in place means the same array)" % what)
        if _overlap(sya, sxb) or _overlap(sya, syb) or _overlap(syb, sxa):
            raise ValueError("%s: the two tensors overlap" % what)
        if any(_overlap(o, t) for o in (sya, syb) for t in (sct, sst)):
            raise ValueError("%s: an output overlaps the tables" % what)
        known = [s[0] for s in (sxa, sya, sxb, syb, sct, sst) if s is not None]
    strides = p.a_strides + (p.b_strides if p.Hb else ())
    p.wide = wide_access(pairing, p.R, itemsize, strides, known)
    v = VEC // itemsize if p.wide else 1
    rot = p.R // v if (p.wide and pairing == "interleaved") else p.R // 2 // v
    tail = -(-(p.D - p.R) // v)
    p.items = 0
    for heads, in_place in ((p.Ha, p.in_place[0]), (p.Hb, p.in_place[1])):
        p.items += p.B * p.T * heads * (rot + (0 if in_place and not p.device_positions else tail))
    p.grid = p.blocks or choose_blocks(p.items)
    ok = bool(native) and bool(float_ok)
    if route is not None:
        if route not in ROUTES:
            raise ValueError("route must be one of %s or None, got %r" % (ROUTES, route))
        if route == "native" and not ok:
            raise ValueError("the native rotary embedding route needs libtnn_hip.so and float32 / float64 operands")
        p.route = route
    else:
        p.route = "native" if ok else "composed"
    return p


def rope_host(x, cos_t, sin_t, offset=0, positions=None, layout="bthd", pairing="half", inverse=False):
    """The rotation in numpy, in x's dtype, with one rounding per arithmetic operation (two products and a sum per output):
    what the composed route computes.  cos_t / sin_t: [P, R / 2]; positions: host integers [B] (T == 1) or None."""
    x = np.asarray(x)
    ct, st = np.asarray(cos_t, dtype=x.dtype), np.asarray(sin_t, dtype=x.dtype)
    P, half = ct.shape
    R = 2 * half
    xv = x if layout == "bthd" else x.transpose(0, 2, 1, 3)              # [B, T, H, D] view
    B, T = xv.shape[:2]
    out = np.array(xv, copy=True)
    if positions is None:
        pos = np.broadcast_to(int(offset) + np.arange(T), (B, T))
    else:
        pos = np.asarray(positions, dtype=np.int64).reshape(B, 1)
    valid = (pos >= 0) & (pos < P)
    safe = np.where(valid, pos, 0)
    c, s = ct[safe][:, :, None, :], st[safe][:, :, None, :]                # [B, T, 1, R / 2]
    if inverse:
        s = -s
    lo, hi = (slice(0, half), slice(half, R)) if pairing == "half" else (slice(0, R, 2), slice(1, R, 2))
    x_lo, x_hi = xv[..., lo], xv[..., hi]
    out[..., lo] = x_lo * c - x_hi * s
    out[..., hi] = x_hi * c + x_lo * s
    out[~valid] = 0
    return out if layout == "bthd" else np.ascontiguousarray(out.transpose(0, 2, 1, 3))


class Rotary(object):
    """The rotary tables of a model: Rotary(max_len, rotary_dim=None, base=10000.0, pairing="half").  Holds the host tables
    per (rotary width, dtype) and the device copies, which are made ONCE, at first use, by device_array.rope and never
    reallocated — a captured step sees fixed addresses.  rotary_dim None: the largest even number <= the head dimension it is
    used with.  One Rotary may be shared by every block of a model."""

    def __init__(self, max_len, rotary_dim=None, base=10000.0, pairing="half"):
        self.max_len = int(max_len)
        if self.max_len < 1:
            raise ValueError("Rotary: max_len must be >= 1, got %r" % (max_len,))
        self.rotary_dim = None if rotary_dim is None else check_rotary_dim(rotary_dim, what="Rotary")
        self.base = float(base)
        if not self.base > 0.0 or not np.isfinite(self.base):
            raise ValueError("Rotary: base must be a positive finite number, got %r" % (base,))
        if pairing not in PAIRINGS:
            raise ValueError("Rotary: pairing must be one of %s, got %r" % (PAIRINGS, pairing))
        self.pairing = pairing
        self._host, self._device = {}, {}

    def width(self, D):
        """The rotary width used with head dimension D."""
        return check_rotary_dim(default_rotary_dim(D) if self.rotary_dim is None else self.rotary_dim, D, "Rotary")

    def host_tables(self, R, dtype):
        key = (int(R), np.dtype(dtype))
        if key not in self._host:
            self._host[key] = tables(self.max_len, key[0], self.base, key[1])
        return self._host[key]

    def device_tables(self, R, dtype, upload):
        """The device copies for (R, dtype); upload(host array) -> device array is called once per table, at first use."""
        key = (int(R), np.dtype(dtype))
        if key not in self._device:
            cos_t, sin_t = self.host_tables(*key)
            self._device[key] = (upload(cos_t), upload(sin_t))
        return self._device[key]
