"""Host planner of the row normalisations (numpy only, no device import): from operand shapes and options to ONE plan —
validated extents, the shape of the row statistics, the kernel form and the route.

    layer   y = (x - mean) * rstd * gamma + beta     mean, biased variance over the LAST axis; rstd = 1 / sqrt(var + eps)
    rms     y = x * rstd * gamma                     rstd = 1 / sqrt(mean(x^2) + eps); no mean, no beta

x is viewed as [M, N]: the last axis is normalised, every leading axis folds into M.  gamma and beta are absent or hold
exactly N elements (shape [N] or [1, N]).

Forms (csrc/tnn_norm.hip)
    "wave"    N <= WAVE_MAX_N: one wave owns a row in registers and reduces it without LDS; ROWS_PER_BLOCK rows per workgroup
    "block"   N <= BLOCK_MAX_N: the whole workgroup owns a row, the waves' sums meet in LDS

Routes
    native    csrc/tnn_norm.hip: one launch forward (y, rstd and mean), one backward call for dx, dgamma and dbeta.  Needs
              the entry points, float32 / float64 operands and N <= BLOCK_MAX_N.
    composed  the same mathematics on the array operations that already exist (sums, products, sqrt).  What runs under the
              CPU test twin and for wider rows, what `fused=False` layers use, and the second, independent implementation
              the GPU tests compare the kernels with.
"""

import math

WAVE_MAX_N = 1024         # TNN_NORM_WAVE_MAX_N: widest row one wave keeps in registers
BLOCK_MAX_N = 4096        # TNN_NORM_BLOCK_MAX_N: widest row one workgroup keeps in registers
ROWS_PER_BLOCK = 4        # TNN_NORM_ROWS_PER_BLOCK: waves (rows in flight) per workgroup of the wave form
VEC = 16                  # TNN_NORM_VEC: bytes per lane of a wide access
MAX_PARTIALS = 1024       # TNN_NORM_MAX_PARTIALS: most partial rows of the parameter gradients
ROUTES = ("native", "composed")
KINDS = ("layer", "rms")
KIND_CODE = {"layer": 0, "rms": 1}            # TNN_NORM_LAYER, TNN_NORM_RMS
GELU_FORMS = ("none", "tanh")                 # `approximate`: the exact erf form, the tanh form
GELU_CODE = {"none": 0, "tanh": 1}


class NormPlan(object):
    __slots__ = ("M", "N", "kind", "eps", "stats_shape", "x_shape", "form", "route", "has_gamma", "has_beta")

    def empty(self):
        return self.M == 0

    def rows_per_block(self):
        return ROWS_PER_BLOCK if self.form == "wave" else 1

    def partials(self):
        """Workgroups of the backward launch when it computes a parameter gradient = partial rows it leaves."""
        rows = self.rows_per_block()
        return max(1, min((self.M + rows - 1) // rows, MAX_PARTIALS))

    def workspace_bytes(self, itemsize, with_dgamma, with_dbeta):
        if self.empty():
            return 0
        return (int(bool(with_dgamma)) + int(bool(with_dbeta))) * self.partials() * self.N * itemsize

    def __repr__(self):
        return "NormPlan(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.__slots__)


def _route(native, float_ok, fits, route):
    if route is not None:
        if route not in ROUTES:
            raise ValueError("route must be one of %s or None, got %r" % (ROUTES, route))
        if route == "native" and not (native and float_ok and fits):
            raise ValueError("the native normalisation route needs libtnn_hip.so, float32 / float64 operands and rows of at "
                             "most %d elements" % BLOCK_MAX_N)
        return route
    return "native" if native and float_ok and fits else "composed"


def _param(shape, n, what):
    if shape is None:
        return False
    shape = tuple(int(s) for s in shape)
    if shape not in ((n,), (1, n)):
        raise ValueError("norm: %s must hold the %d elements of the last axis as [%d] or [1, %d], got shape %s"
                         % (what, n, n, n, shape))
    return True


def plan_norm(x_shape, gamma_shape=None, beta_shape=None, kind="layer", eps=1e-5, native=True, float_ok=True, route=None):
    """The plan of a normalisation of x over its last axis.  native: the library has the entry points; float_ok: every
    operand is (or will be made) float32 / float64 of one kind; route: force one ("native" / "composed"), None picks."""
    if kind not in KINDS:
        raise ValueError("norm: kind must be one of %s, got %r" % (KINDS, kind))
    x_shape = tuple(int(s) for s in x_shape)
    if len(x_shape) < 1:
        raise ValueError("norm: the input needs at least one axis, got a scalar")
    p = NormPlan()
    p.N = x_shape[-1]
    if p.N < 1:
        raise ValueError("norm: the normalised axis is empty (x %s)" % (x_shape,))
    p.has_gamma = _param(gamma_shape, p.N, "gamma")
    if kind == "rms" and beta_shape is not None:
        raise ValueError("norm: RMS norm takes no beta")
    p.has_beta = _param(beta_shape, p.N, "beta")
    try:
        eps = float(eps)
    except (TypeError, ValueError):
        raise ValueError("norm: eps must be a finite number >= 0, got %r" % (eps,))
    if not (math.isfinite(eps) and eps >= 0.0):
        raise ValueError("norm: eps must be a finite number >= 0, got %r" % (eps,))
    p.kind, p.eps = kind, eps
    p.x_shape, p.stats_shape = x_shape, x_shape[:-1]
    p.M = math.prod(p.stats_shape)
    p.form = "wave" if p.N <= WAVE_MAX_N else "block"
    p.route = _route(native, float_ok, p.N <= BLOCK_MAX_N, route)
    return p


def gelu_form(approximate):
    if approximate not in GELU_FORMS:
        raise ValueError("gelu: approximate must be one of %s, got %r" % (GELU_FORMS, approximate))
    return approximate


def gelu_route(approximate, native=True, float_ok=True, route=None):
    """"native" or "composed" for GELU.  The composed route exists for the tanh form only: there is no erf among the
    existing elementwise operations."""
    gelu_form(approximate)
    if route is not None and route not in ROUTES:
        raise ValueError("route must be one of %s or None, got %r" % (ROUTES, route))
    can = native and float_ok
    if route == "native" and not can:
        raise ValueError("the native GELU route needs libtnn_hip.so and float32 / float64 operands")
    if route == "composed" or not can:
        if approximate == "none":
            raise ValueError("the exact (erf) GELU needs the native route of libtnn_hip.so; only approximate=\"tanh\" has a "
                             "composed form")
        return "composed"
    return "native"
