"""Host planner of 2-D convolution and max pooling (numpy only, no device import): from shapes, stride and padding to ONE
plan — validated extents, output shape, the route that executes it and the geometry of the native kernels.

Layout: activations NCHW, filters [F, C, KH, KW], bias [F].  `stride` (>= 1) and `padding` (>= 0, zeros; -inf for pooling)
are an integer or a (height, width) pair.  No dilation, no groups.  Output extent per axis: (H + 2 p - K) // s + 1.

Routes
    native    csrc/tnn_conv.hip: one launch per product (forward, data gradient, filter + bias gradient, pool forward /
              backward).  Taken whenever the library has the entry points and the operands are float32 / float64.
    composed  the same mathematics on the array operations that already exist, one round per filter tap: a stepped slice of
              the padded input, a product over the channel axis, an add (pooling: a fold of `maximum` over the shifted
              slices in row-major tap order).  What runs under the CPU test twin, what `fused=False` layers use, and the
              second, independent implementation the GPU tests compare the kernels with.
"""

import math

FORM_AUTO, FORM_TILE, FORM_SMALL = 0, 1, 2      # TNN_CONV_FORM_*
TILE_ELEMS = 4096                               # TNN_CONV_TILE_ELEMS
SMALL_MAX_ROWS = 32                             # AUTO: the 16-row geometry up to this many rows (channels) of the GEMM view
MAX_SPLITS = 256
K_TILE = 16                                     # contraction depth of one LDS tile
ROUTES = ("native", "composed")


class ConvPlan(object):
    __slots__ = ("N", "C", "H", "W", "F", "KH", "KW", "sh", "sw", "ph", "pw", "OH", "OW", "out_shape", "route")

    def geometry(self):
        """The eleven extents every native entry point takes, in its argument order."""
        return (self.N, self.C, self.H, self.W, self.F, self.KH, self.KW, self.sh, self.sw, self.ph, self.pw)

    def __repr__(self):
        return "ConvPlan(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.__slots__)


class PoolPlan(object):
    __slots__ = ("N", "C", "H", "W", "KH", "KW", "sh", "sw", "ph", "pw", "OH", "OW", "out_shape", "route")

    def geometry(self):
        return (self.N * self.C, self.H, self.W, self.KH, self.KW, self.sh, self.sw, self.ph, self.pw)

    def __repr__(self):
        return "PoolPlan(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.__slots__)


def pair(value, name, minimum):
    """An integer or a pair of integers -> (height, width), each >= minimum."""
    if isinstance(value, (tuple, list)):
        if len(value) != 2:
            raise ValueError("%s must be an integer or a pair, got %r" % (name, value))
        a, b = value
    else:
        a = b = value
    for v in (a, b):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError("%s must be integral, got %r" % (name, value))
    a, b = int(a), int(b)
    if a < minimum or b < minimum:
        raise ValueError("%s must be >= %d, got %r" % (name, minimum, value))
    return a, b


def out_extent(size, kernel, stride, padding):
    """(size + 2 padding - kernel) // stride + 1; raises when the padded input is smaller than the kernel."""
    if size + 2 * padding < kernel:
        raise ValueError("input extent %d (+ 2 x %d padding) is smaller than the kernel extent %d" % (size, padding, kernel))
    return (size + 2 * padding - kernel) // stride + 1


def _route(native, dtype_kind_ok, route):
    if route is not None:
        if route not in ROUTES:
            raise ValueError("route must be one of %s or None, got %r" % (ROUTES, route))
        if route == "native" and not (native and dtype_kind_ok):
            raise ValueError("the native convolution route needs libtnn_hip.so and float32 / float64 operands")
        return route
    return "native" if native and dtype_kind_ok else "composed"


def plan_conv2d(x_shape, w_shape, b_shape=None, stride=1, padding=0, dilation=1, groups=1, native=True, float_ok=True,
                route=None):
    """The plan of conv2d(x, w, b).  native: the library has the entry points; float_ok: every operand is (or will be made)
    float32 / float64 of one kind; route: force one ("native" / "composed"), None picks."""
    if pair(dilation, "dilation", 1) != (1, 1):
        raise ValueError("conv2d: dilation is not supported")
    if groups != 1:
        raise ValueError("conv2d: groups are not supported")
    x_shape, w_shape = tuple(int(s) for s in x_shape), tuple(int(s) for s in w_shape)
    if len(x_shape) != 4:
        raise ValueError("conv2d: the input must be [N, C, H, W], got shape %s" % (x_shape,))
    if len(w_shape) != 4:
        raise ValueError("conv2d: the filters must be [F, C, KH, KW], got shape %s" % (w_shape,))
    p = ConvPlan()
    p.N, p.C, p.H, p.W = x_shape
    p.F, wc, p.KH, p.KW = w_shape
    if wc != p.C:
        raise ValueError("conv2d: the input has %d channels, the filters expect %d" % (p.C, wc))
    if min(p.C, p.H, p.W, p.F, p.KH, p.KW) < 1:
        raise ValueError("conv2d: empty channel, image or filter extent (x %s, w %s)" % (x_shape, w_shape))
    if b_shape is not None and math.prod(int(s) for s in b_shape) != p.F:
        raise ValueError("conv2d: the bias must hold %d elements, got shape %s" % (p.F, tuple(b_shape)))
    p.sh, p.sw = pair(stride, "stride", 1)
    p.ph, p.pw = pair(padding, "padding", 0)
    p.OH = out_extent(p.H, p.KH, p.sh, p.ph)
    p.OW = out_extent(p.W, p.KW, p.sw, p.pw)
    p.out_shape = (p.N, p.F, p.OH, p.OW)
    p.route = _route(native, float_ok, route)
    return p


def plan_pool2d(x_shape, kernel, stride=None, padding=0, native=True, float_ok=True, route=None):
    """The plan of max_pool2d(x, kernel, stride, padding); stride None = the kernel (windows that tile the image)."""
    x_shape = tuple(int(s) for s in x_shape)
    if len(x_shape) != 4:
        raise ValueError("max_pool2d: the input must be [N, C, H, W], got shape %s" % (x_shape,))
    p = PoolPlan()
    p.N, p.C, p.H, p.W = x_shape
    if min(p.H, p.W) < 1:
        raise ValueError("max_pool2d: empty image extent %s" % (x_shape,))
    p.KH, p.KW = pair(kernel, "kernel", 1)
    p.sh, p.sw = (p.KH, p.KW) if stride is None else pair(stride, "stride", 1)
    p.ph, p.pw = pair(padding, "padding", 0)
    if p.ph > p.KH // 2 or p.pw > p.KW // 2:
        raise ValueError("max_pool2d: padding %s is larger than half the window %s (a window could be all padding)"
                         % ((p.ph, p.pw), (p.KH, p.KW)))
    p.OH = out_extent(p.H, p.KH, p.sh, p.ph)
    p.OW = out_extent(p.W, p.KW, p.sw, p.pw)
    p.out_shape = (p.N, p.C, p.OH, p.OW)
    p.route = _route(native, float_ok, route)
    return p


# ---------------------------------------------------------------------- geometry of the native float32 kernels
def form_for(rows, form=FORM_AUTO):
    """The geometry the library uses for a GEMM view with `rows` channel rows: FORM_SMALL (16 x 256) or FORM_TILE (64 x 64)."""
    if form == FORM_AUTO:
        return FORM_SMALL if rows <= SMALL_MAX_ROWS else FORM_TILE
    if form not in (FORM_TILE, FORM_SMALL):
        raise ValueError("form %r" % (form,))
    return form


def tiles(rows, cols, form=FORM_AUTO):
    tm, tp = (16, 256) if form_for(rows, form) == FORM_SMALL else (64, 64)
    return -(-rows // tm) * -(-cols // tp)


def filter_splits(plan, with_db, form=FORM_AUTO, cus=256):
    """How many ranges the filter gradient cuts its N OH OW contraction into: the GEMM view has F x (C KH KW [+ 1]) outputs,
    a handful of tiles, so the contraction is spread until about two workgroups per compute unit exist; every range keeps at
    least four K-tiles.  1 = no workspace, no reduction."""
    k = plan.N * plan.OH * plan.OW
    t = tiles(plan.F, plan.C * plan.KH * plan.KW + (1 if with_db else 0), form)
    want = (2 * cus) // t
    most = k // (4 * K_TILE)
    return int(max(1, min(want, most, MAX_SPLITS)))


def filter_workspace_bytes(plan, with_db, form, splits):
    """Bytes of the workspace tnn_conv2d_bwd_filter needs (mirrors tnn_conv2d_bwd_filter_workspace): arrival counters, then
    the partial tiles."""
    if splits <= 1:
        return 0
    t = tiles(plan.F, plan.C * plan.KH * plan.KW + (1 if with_db else 0), form)
    return (t * 4 + 255) // 256 * 256 + splits * t * TILE_ELEMS * 4


def taps(plan):
    """[(kh, kw, row slice, column slice)] of the padded input, row-major tap order (the composed route)."""
    out = []
    for kh in range(plan.KH):
        for kw in range(plan.KW):
            out.append((kh, kw, slice(kh, kh + (plan.OH - 1) * plan.sh + 1, plan.sh),
                        slice(kw, kw + (plan.OW - 1) * plan.sw + 1, plan.sw)))
    return out
