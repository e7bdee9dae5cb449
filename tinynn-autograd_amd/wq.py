"""Host planner of the int8 weight-only linear layer (numpy only, no device import): the format, stated in numpy, and from
operand shapes and options to ONE plan per call — validated extents, the row form, the lane group, the split over K, the
workspace size, the route.

The format (include/tnn_wq.h).  For a float32 weight w [K, N] ([num_in, num_out], as Dense stores it), symmetric, per OUTPUT
COLUMN:

    scale[n] = absmax_k |w[k, n]| / 127        code[k, n] = clamp(rne(w[k, n] / scale[n]), -127, 127)        w^ = code * scale

in float32, with the residual step of the cache format (kvq.quantize_host): |w - code scale| <= scale / 2 for every element.
A column of zeros has scale 0 and codes 0; non-finite weights are out of scope.  The codes are int8 two's-complement bytes in
a uint8 array [K / 4, N, 4]: element [kb, n, j] is the code of w[4 kb + j, n], so one 16-byte access holds 4 consecutive
columns by 4 consecutive k and consecutive lanes continue along n.  K and N must be multiples of 4 (fits()); a weight that
does not fit keeps its float values and its layer the float path.  K N + 4 N bytes instead of 4 K N.

Routes
    native    csrc/tnn_wq.hip.  M <= MAX_ROWS rows: tnn_wq_linear (kernel "linear"), the row form the next of ROW_FORMS, K cut
              over `splits` workgroups per 256-column panel.  More rows (the prefill): tnn_wq_dequantize into a scratch
              weight and the ordinary float32 GEMM (kernel "dequant_gemm"), which is compute-bound there.
    composed  dequantize (on the host under the CPU test twin, by dequantize_host) and the ordinary product.  The second,
              independent implementation the GPU tests compare the kernel with.

SLOWER_RULES lists the regions in which the probe (tools/probes/wq_ab.py, profiles/wq_vs_float.txt) found tnn_wq_linear
SLOWER than the float32 ops.dense_ of the same shape — the weights still take a quarter of the memory there; expect_slower()
tells a caller who quantizes for speed alone.  Out of scope: group-wise scales along K, int4 / fp8 codes, float64, a backward
pass.
"""

import numpy as np

from . import kvq as _kq

VEC = 16                  # TNN_WQ_VEC: bytes per lane and access (4 columns by 4 k)
MAX_ROWS = 16             # TNN_WQ_MAX_ROWS
ROW_FORMS = (1, 2, 4, 8, 16)
PANEL = 256               # TNN_WQ_PANEL: columns per workgroup
UNROLL = 4                # TNN_WQ_UNROLL: packs a lane has in flight per round
WAVES = 4                 # TNN_WQ_WAVES
STAGE = 768               # TNN_WQ_STAGE: k values of x staged in LDS at a time
MAX_SPLITS = 64           # TNN_WQ_MAX_SPLITS
ROUTES = ("native", "composed")
QUANTS = ("int8",)
CUS = 256                 # compute units of one MI355X: what choose_splits fills
WORKGROUPS_PER_CU = 2     # ... and how many workgroups per unit it aims at
ROUNDS_PER_SPLIT = 4      # ... each with at least this many rounds of k-blocks
SMALL_WEIGHT = 1 << 20    # codes below which K is not split over workgroups: one launch instead of two
# (most K N, most M): ops.dense_wq_ with K N <= the first and M <= the second is SLOWER than the float32 ops.dense_ —
# profiles/wq_vs_float.txt, section (a): at 512 x 512 the call takes 0.21x .. 0.47x the float call's speed for every M (a quarter
# of a MiB of codes: both calls are launch and host time, and the float GEMM's host path is the shorter); at 4096 x 4096 it is
# level (1.01x .. 1.09x), from 4096 x 16384 on 1.6x .. 4.4x faster.  Nothing between 512 x 512 and 4096 x 4096 was measured.
SLOWER_RULES = ((512 * 512, MAX_ROWS),)


def expect_slower(M, K, N):
    """Whether SLOWER_RULES marks the shape: the int8 product then costs more time than the float32 one (it still saves
    memory)."""
    return any(K * N <= most_kn and M <= most_m for most_kn, most_m in SLOWER_RULES)


# ---------------------------------------------------------------------- the format
def fits(K, N):
    return K >= 4 and N >= 4 and K % 4 == 0 and N % 4 == 0


def codes_shape(K, N):
    if not fits(K, N):
        raise ValueError("wq: K %d, N %d (the code layout [K / 4, N, 4] needs multiples of 4)" % (K, N))
    return (K // 4, N, 4)


def weight_shape(codes_shape_):
    """(K, N) of a code array's shape."""
    sh = tuple(int(s) for s in codes_shape_)
    if len(sh) != 3 or sh[2] != 4 or sh[1] % 4 != 0:
        raise ValueError("wq: the codes must be [K / 4, N, 4] with N a multiple of 4, got shape %s" % (sh,))
    return 4 * sh[0], sh[1]


def quantize_host(w):
    """w float32 [K, N] -> (codes uint8 [K / 4, N, 4] holding int8 bytes, scales float32 [N]): the rule of the module's head
    (a column of w is a row of the cache format)."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    if w.ndim != 2:
        raise ValueError("wq.quantize_host: w must be [K, N], got shape %s" % (w.shape,))
    K, N = w.shape
    shape = codes_shape(K, N)
    by_column, scales = _kq.quantize_host(w.T)                               # [N, K], [N]
    return np.ascontiguousarray(by_column.T.reshape(shape[0], 4, N).transpose(0, 2, 1)), scales


def unpack_codes(codes):
    """codes uint8 [K / 4, N, 4] -> int8 [K, N]."""
    K, N = weight_shape(np.shape(codes))
    return np.ascontiguousarray(codes, dtype=np.uint8).view(np.int8).transpose(0, 2, 1).reshape(K, N)


def dequantize_host(codes, scales, dtype=np.float64):
    """code * scale in `dtype` (float64: exact) -> [K, N]."""
    return unpack_codes(codes).astype(dtype) * np.asarray(scales, dtype=np.float32).astype(dtype)[None, :]


# ---------------------------------------------------------------------- the geometry of tnn_wq_linear
def lane_group(N):
    """G = min(64, pow2ceil(N / 4)): the lanes that read one k-block of a panel."""
    g = 1
    while g < 64 and g < N // 4:
        g <<= 1
    return g


def pass_blocks(N):
    """The k-blocks one workgroup takes per round: waves x unroll x the lane groups of a wave."""
    return WAVES * UNROLL * (64 // lane_group(N))


def most_splits(K):
    return max(1, min(K // 4, MAX_SPLITS))


def choose_splits(M, K, N):
    """Workgroups per column panel: enough to put WORKGROUPS_PER_CU on every unit, each with at least ROUNDS_PER_SPLIT rounds
    of k-blocks, and ONE below SMALL_WEIGHT codes, where the combine launch costs more than the split saves; a pure function
    of the extents, so a repeated call adds in the same order.  Tuned from profiles/wq_vs_float.txt, section (b): the best of
    1 .. 64 was 1 at 512 x 512, 16 at 4096 x 4096 and 8 at 4096 x 16384, which is what this gives."""
    if K * N < SMALL_WEIGHT:
        return 1
    panels = -(-N // PANEL)
    want = -(-CUS * WORKGROUPS_PER_CU // panels)
    return max(1, min(want, (K // 4) // (ROUNDS_PER_SPLIT * pass_blocks(N)), most_splits(K)))


def split_range(K, splits, s):
    """The k-blocks [first, stop) of split s."""
    nb = K // 4
    return s * nb // splits, (s + 1) * nb // splits


def workspace_bytes(M, N, splits):
    """What tnn_wq_linear_workspace returns."""
    return 0 if splits == 1 else -(-splits * M * N * 4 // 16) * 16


class LinearPlan(object):
    __slots__ = ("M", "K", "N", "route", "kernel", "rows", "group", "panels", "splits", "bias", "out_shape")

    def empty(self):
        return self.M * self.N == 0

    def workspace_bytes(self):
        return workspace_bytes(self.M, self.N, self.splits) if self.kernel == "linear" else 0

    def __repr__(self):
        return "LinearPlan(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.__slots__)


def plan_linear(x_shape, codes_shape_, scales_shape, b_shape=None, splits=None, native=True, float_ok=True, aligned=True,
                route=None):
    """The plan of wq_linear: x [M, K] over codes [K / 4, N, 4] and scales [N], b [N] (or [1, N]) or None."""
    what = "wq_linear"
    p = LinearPlan()
    p.K, p.N = weight_shape(codes_shape_)
    x_shape = tuple(int(s) for s in x_shape)
    if len(x_shape) != 2 or x_shape[1] != p.K:
        raise ValueError("%s: x must be [M, K] = [M, %d], got shape %s" % (what, p.K, x_shape))
    if int(np.prod(scales_shape)) != p.N or (b_shape is not None and int(np.prod(b_shape)) != p.N):
        raise ValueError("%s: scales and b must hold N = %d elements, got shapes %s and %s" % (what, p.N, tuple(scales_shape), b_shape))
    p.M, p.bias, p.out_shape = x_shape[0], b_shape is not None, (x_shape[0], p.N)
    ok = native and float_ok and aligned and fits(p.K, p.N)
    if route is not None and route not in ROUTES:
        raise ValueError("route must be one of %s or None, got %r" % (ROUTES, route))
    if route == "native" and not ok:
        raise ValueError("the native int8 linear route needs libtnn_hip.so, float32 operands and 16-byte aligned operands")
    p.route = route or ("native" if ok else "composed")
    p.kernel = "linear" if p.route == "native" and 1 <= p.M <= MAX_ROWS else "dequant_gemm"
    p.rows = next((r for r in ROW_FORMS if r >= p.M), None) if p.kernel == "linear" else None
    p.group, p.panels = lane_group(p.N), -(-p.N // PANEL)
    if splits is None:
        p.splits = choose_splits(p.M, p.K, p.N) if p.kernel == "linear" else 1
    else:
        p.splits = int(splits)
        if not 1 <= p.splits <= most_splits(p.K):
            raise ValueError("%s: splits %d outside [1, %d] (%d k-blocks)" % (what, p.splits, most_splits(p.K), p.K // 4))
    return p


def plan_weight(shape):
    """What quantize_weights does with a parameter of this shape: "int8", or "float" when the format does not fit."""
    shape = tuple(int(s) for s in shape)
    return "int8" if len(shape) == 2 and fits(*shape) else "float"
