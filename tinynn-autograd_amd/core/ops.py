"""Differentiable ops on device-backed Tensors (reference: core/ops.py:12-384).

Every public name of the reference module exists here with the same signature and the same vjp
semantics (tie rules of maximum_/minimum_/max_/min_, inclusive clip mask, un-broadcast rule, saved
inputs held by reference in the closures).  Forward values and vjps are DeviceArray expressions, i.e.
HIP kernels behind the C-ABI; nothing is computed on the host.  Cited line numbers point at the
reference expression each piece replaces.

Extra fused nodes used by this package's own layers/losses (parity-tested against the generic chain):
`dense_` (GEMM + bias epilogue), `sigmoid_`, `softmax_nll_` (whole-batch softmax NLL), `conv2d_` / `max_pool2d_` (NCHW
convolution and max pooling, csrc/tnn_conv.hip; the reference has neither), `attention_` (fused scaled-dot-product attention,
csrc/tnn_attn.hip; likewise), `layer_norm_` / `rms_norm_` / `gelu_` (csrc/tnn_norm.hip; likewise), `embedding_` /
`cross_entropy_` (csrc/tnn_token.hip; likewise — `embedding_` is the gather whose vjp ACCUMULATES over repeated ids, which
`getitem_`'s does not), `dropout_` (csrc/tnn_dropout.hip; likewise — its mask comes from the device random generator of rng.py
and is regenerated, not stored, for the vjp), `gated_` / `silu_` (csrc/tnn_gated.hip; likewise — SwiGLU / GEGLU, both gradients
from one launch).
"""

import math
import weakref

import numpy as np

from .. import _lib
from .. import device_array as da


_AS_TENSOR = None


def as_tensor(obj):
    global _AS_TENSOR
    if _AS_TENSOR is None:
        from .tensor import as_tensor as _as_tensor   # lazy: tensor imports ops (resolved once, not on every call)
        _AS_TENSOR = _as_tensor
    return _AS_TENSOR(obj)


# ---------------------------------------------------------------------- graph construction
def build_binary_ops_tensor(ts1, ts2, grad_fn_ts1, grad_fn_ts2, values):
    """reference: core/ops.py:12-20"""
    parents = [(ts1, grad_fn_ts1), (ts2, grad_fn_ts2)]
    return _make_node(ts1.__class__, values, parents)


def build_unary_ops_tensor(ts, grad_fn, values):
    """reference: core/ops.py:23-29"""
    return _make_node(ts.__class__, values, [(ts, grad_fn)])


def _make_node(cls, values, parents):
    # only inputs that require grad become edges, so e.g. dX of the first Dense layer is never computed
    edges = [dict(tensor=t, grad_fn=fn) for t, fn in parents if t.requires_grad]
    return cls(values, bool(edges), edges)


def _unbroadcast(grad, shape):
    """Undo numpy broadcasting of an operand of `shape` (core/ops.py:41-46): sum away the leading axes
    the operand did not have, then sum (keepdims) over the axes where it had extent 1."""
    grad = da.asarray(grad)
    if grad.shape == tuple(shape):
        return grad
    extra = grad.ndim - len(shape)
    if extra > 0:
        grad = grad.sum(axis=tuple(range(extra)))
    for axis, dim in enumerate(shape):
        if dim == 1 and grad.shape[axis] != 1:
            grad = grad.sum(axis=axis, keepdims=True)
    return grad


# ---------------------------------------------------------------------- arithmetic
def add_(ts1, ts2):
    """reference: core/ops.py:32-58"""
    values = ts1.values + ts2.values
    return build_binary_ops_tensor(
        ts1, ts2,
        lambda g: _unbroadcast(g, ts1.shape),
        lambda g: _unbroadcast(g, ts2.shape),
        values)


def sub_(ts1, ts2):
    """reference: core/ops.py:61-62 (a + (-b)); one node here, same values and vjps."""
    values = ts1.values - ts2.values
    return build_binary_ops_tensor(
        ts1, ts2,
        lambda g: _unbroadcast(g, ts1.shape),
        lambda g: _unbroadcast(-da.asarray(g), ts2.shape),
        values)


def mul_(ts1, ts2):
    """reference: core/ops.py:65-90"""
    values = ts1.values * ts2.values
    return build_binary_ops_tensor(
        ts1, ts2,
        lambda g: _unbroadcast(g * ts2.values, ts1.shape),
        lambda g: _unbroadcast(g * ts1.values, ts2.shape),
        values)


def div_(ts1, ts2):
    """reference: core/ops.py:93-118"""
    values = ts1.values / ts2.values
    return build_binary_ops_tensor(
        ts1, ts2,
        lambda g: _unbroadcast(g / ts2.values, ts1.shape),
        lambda g: _unbroadcast(-da.asarray(g) * ts1.values / ts2.values ** 2, ts2.shape),
        values)


def pow_(ts1, ts2):
    """reference: core/ops.py:121-147"""
    values = ts1.values ** ts2.values

    def grad_base(g):
        return _unbroadcast(g * ts2.values * ts1.values ** (ts2.values - 1), ts1.shape)

    def grad_exponent(g):
        return _unbroadcast(g * (da.log(ts1.values) * values), ts2.shape)

    return build_binary_ops_tensor(ts1, ts2, grad_base, grad_exponent, values)


def dot_(ts1, ts2):
    """reference: core/ops.py:150-163.  `.T` is a lazy flag, so the vjps run as NT / TN GEMMs.

    2-D @ 2-D is the reference's pair of calls.  For every other form numpy's matmul admits (stacks of matrices, broadcast
    batch dimensions, 1-D operands) the reference's backward raises or mis-shapes (`.T` reverses ALL axes), so the vjps
    follow the mathematics: dA = unbroadcast(G @ swap(B), A.shape), dB = unbroadcast(swap(A) @ G, B.shape), swap = the
    last two axes, handed to the batched product as transpose flags and never copied; 1-D operands are promoted as
    numpy promotes them."""
    a, b = ts1.values, ts2.values
    values = a @ b
    if a.ndim == 2 and b.ndim == 2:
        return build_binary_ops_tensor(
            ts1, ts2,
            lambda g: da.asarray(g) @ ts2.values.T,
            lambda g: ts1.values.T @ da.asarray(g),
            values)
    grad_a, grad_b = _dot_vjps_nd(ts1, ts2)
    return build_binary_ops_tensor(ts1, ts2, grad_a, grad_b, values)


def _dot_vjps_nd(ts1, ts2):
    """The two vjps of `a @ b` when an operand is 1-D or N-d (saved inputs are read at backward time, like everywhere)."""
    a_shape, b_shape = tuple(ts1.values.shape), tuple(ts2.values.shape)
    a2_shape = (1,) + a_shape if len(a_shape) == 1 else a_shape          # numpy's promotion: a row ...
    b2_shape = b_shape + (1,) if len(b_shape) == 1 else b_shape          # ... and a column
    K, N = b2_shape[-2], b2_shape[-1]

    def promoted(g):
        """g in the shape of the promoted product [batch..., M, N]"""
        g = da.asarray(g)
        shape = list(g.shape)
        if len(b_shape) == 1:
            shape.append(1)
        if len(a_shape) == 1:
            shape.insert(len(shape) - 1, 1)
        return g.reshape(shape)

    def grad_a(g):
        b2 = da.asarray(ts2.values).reshape(b2_shape)
        ga = da.matmul(promoted(g), b2, swap_b=True)                     # [batch..., M, K]
        return _unbroadcast(ga, a2_shape).reshape(a_shape)

    def grad_b(g):
        a2 = da.asarray(ts1.values).reshape(a2_shape)
        g = promoted(g)
        if len(b2_shape) == 2 and len(a2_shape) > 2:
            # X[..., M, K] @ W[K, N]: dW is ONE long-K TN product over all the rows — no [batch, K, N] temporary, no
            # reduction pass
            gb = a2.reshape(-1, K).T @ g.reshape(-1, N)
        else:
            gb = _unbroadcast(da.matmul(a2, g, swap_a=True), b2_shape)   # [batch..., K, N]
        return gb.reshape(b_shape)

    return grad_a, grad_b


def maximum_(ts1, ts2):
    """reference: core/ops.py:166-188 — ties send the gradient to ts1 (>=)."""
    values = da.maximum(ts1.values, ts2.values)
    return build_binary_ops_tensor(
        ts1, ts2,
        lambda g: _unbroadcast(da.mul_mask(g, ts1.values >= ts2.values), ts1.shape),
        lambda g: _unbroadcast(da.mul_mask(g, ts2.values > ts1.values), ts2.shape),
        values)


def minimum_(ts1, ts2):
    """reference: core/ops.py:191-213 — ties send the gradient to ts1 (<=)."""
    values = da.minimum(ts1.values, ts2.values)
    return build_binary_ops_tensor(
        ts1, ts2,
        lambda g: _unbroadcast(da.mul_mask(g, ts1.values <= ts2.values), ts1.shape),
        lambda g: _unbroadcast(da.mul_mask(g, ts2.values < ts1.values), ts2.shape),
        values)


# ---------------------------------------------------------------------- unary
def exp_(ts):
    """reference: core/ops.py:216-222 (the vjp reuses the saved output)"""
    values = da.exp(ts.values)
    return build_unary_ops_tensor(ts, lambda g: values * g, values)


def log_(ts):
    """reference: core/ops.py:243-249"""
    values = da.log(ts.values)
    return build_unary_ops_tensor(ts, lambda g: g / ts.values, values)


def neg_(ts):
    """reference: core/ops.py:293-299"""
    return build_unary_ops_tensor(ts, lambda g: -da.asarray(g), -ts.values)


def _extreme(ts, axis, rmax):
    x = ts.values
    values = x.max(axis=axis) if rmax else x.min(axis=axis)

    def grad_fn(g):
        # every element equal to the extreme receives the full gradient (core/ops.py:229,238)
        ext = x.max(axis=axis, keepdims=True) if rmax else x.min(axis=axis, keepdims=True)
        return da.mul_mask(g, ext == x)

    return build_unary_ops_tensor(ts, grad_fn, values)


def max_(ts, axis=None):
    """reference: core/ops.py:225-231"""
    return _extreme(ts, axis, True)


def min_(ts, axis=None):
    """reference: core/ops.py:234-240"""
    return _extreme(ts, axis, False)


def sum_(ts, axis):
    """reference: core/ops.py:252-265"""
    x = ts.values
    values = x.sum(axis=axis)

    def grad_fn(g):
        g = da.asarray(g)
        if axis is None:
            if g.ndim > x.ndim:
                raise ValueError("gradient of a full sum must be broadcastable to the input")
            return g._as_float(x.dtype if x.dtype.kind == "f" else None)._broadcast_to(x.shape)
        return np.expand_dims(g._contig(), axis)._broadcast_to(x.shape)

    return build_unary_ops_tensor(ts, grad_fn, values)


def transpose_(ts, axes=None):
    """reference: core/ops.py:268-279"""
    values = ts.values.transpose(axes)
    perm = list(reversed(range(ts.values.ndim))) if axes is None else [int(a) for a in axes]
    inverse = [int(i) for i in np.argsort(perm)]
    return build_unary_ops_tensor(ts, lambda g: da.asarray(g).transpose(inverse), values)


def getitem_(ts, key):
    """reference: core/ops.py:282-290 (slice = view, 1-D integer array = row gather kernel, any other numpy key = one
    gather of csrc/tnn_index.hip).  The vjp assigns, as the reference's `recover_grad[key] = grad` does: where the key repeats
    an index the LAST gradient wins (deterministic scatter) — not the sum np.add.at would give."""
    x = ts.values
    if isinstance(key, ts.__class__):
        key = key.values
    key = da.expand_masks(key)         # a device mask is counted once: forward and vjp share its coordinates
    values = x[key]

    def grad_fn(g):
        recovered = da.zeros(x.shape, x.dtype if x.dtype.kind == "f" else None)
        recovered[key] = g
        return recovered

    return build_unary_ops_tensor(ts, grad_fn, values)


def reshape_(ts, newshape):
    """reference: core/ops.py:302-309"""
    shape = ts.values.shape
    return build_unary_ops_tensor(ts, lambda g: da.asarray(g).reshape(shape), ts.values.reshape(newshape))


def pad_(ts, pad_width, mode):
    """reference: core/ops.py:312-321"""
    values = np.pad(ts.values, pad_width=pad_width, mode=mode)
    window = tuple(slice(int(before), int(size - after))
                   for size, (before, after) in zip(values.shape, pad_width))
    return build_unary_ops_tensor(ts, lambda g: da.asarray(g)[window], values)


def flatten_(ts):
    """reference: core/ops.py:324-330"""
    shape = ts.shape
    return build_unary_ops_tensor(ts, lambda g: da.asarray(g).reshape(shape), ts.values.ravel())


def clip_(ts, min, max):
    """reference: core/ops.py:333-344.  The inclusive mask (x >= min) & (x <= max) is recomputed from the
    saved input inside the vjp kernel instead of being stored as a bool array."""
    x = ts.values
    values = da.clip(x, min, max)
    return build_unary_ops_tensor(ts, lambda g: da.clip_bwd(g, x, min, max), values)


# ---------------------------------------------------------------------- fused nodes (this package's own)
class _DenseVjp(object):
    """The vjps of one ops.dense_ node (see dense_): per-edge forms for schedulers that ask edge by edge (the reference's
    own recursion), `fused_vjp` for Tensor.backward, which offers all edges at once."""
    __slots__ = ("b", "xv", "wv", "bv", "out", "m", "k", "n", "dt", "relu", "x_relu", "edges", "shared")

    def __init__(self, b, xv, wv, bv, out, m, k, n, dt, relu, x_relu):
        # arrays, not the input tensors (only the bias tensor, a leaf, for its arena view): a vjp that held its node's input
        # TENSOR closed a reference cycle through the speculative head (x -> its wrapped vjp -> the classifier's vjp -> x)
        self.b, self.xv, self.wv, self.bv, self.out = b, xv, wv, bv, out
        self.m, self.k, self.n, self.dt, self.relu, self.x_relu = m, k, n, dt, relu, x_relu
        self.edges = ()
        self.shared = []              # [(g object, db)] computed together with dW, waiting for the bias vjp

    def dz_of(self, g_in):
        """Gradient w.r.t. the pre-activation: g itself, or g * [z >= 0] for the fused ReLU unless a consumer's dX
        launch applied that mask already."""
        g = da.asarray(g_in)
        if not self.relu or g._tag is self.out:
            return g
        return da.mul_signmask(g, self.out)

    def d_x(self, g):
        return self.dz_of(g) @ self.wv.T

    def _dw_db(self, g_in, dest):
        m, k, n, dt, b = self.m, self.k, self.n, self.dt, self.b
        g = self.dz_of(g_in)
        if g.shape != (m, n) or g.dtype != dt or g._hv is not None or not g.size:
            return None
        g = g._contig()
        dw = dest if dest is not None else da.empty((k, n), dt)
        db = None
        if b.requires_grad:
            home = getattr(b, "_grad_home", None)
            if (home is not None and b._grad is None and b._grad_zero and not getattr(b, "_home_lent", False)
                    and home.size == n and home.dtype == dt):
                db = home                            # the bias' own arena view: lent out once per backward
                b._home_lent = True
            else:
                db = da.empty(tuple(b.shape), dt)
        _lib.get().gemm_tn_colsum(k, n, m, self.xv._ptr, k, g._ptr, n, dw._ptr, n, db._ptr if db is not None else None,
                                  dw._code())
        if db is not None:
            del self.shared[:]
            self.shared.append((g_in, db))
        return dw

    def d_w(self, g):
        dw = self._dw_db(g, None)
        return dw if dw is not None else self.xv.T @ self.dz_of(g)

    def d_w_into(self, g, dest):
        if dest.shape != (self.k, self.n) or dest.dtype != self.dt or dest._t or dest._hv is not None:
            return self.d_w(g)
        dw = self._dw_db(g, dest)
        return dw if dw is not None else self.d_w(g)

    d_w.into = d_w_into               # Tensor.backward: the first contribution of a lazily-zero leaf goes to its arena view

    def d_b(self, g):
        if self.shared and self.shared[0][0] is g:
            return self.shared.pop()[1]
        return _unbroadcast(self.dz_of(g), self.b.shape)

    def fused_vjp(self, g_in, homes):
        """All edges from ONE tnn_dense_bwd launch.  homes[i]: the arena view of edge i's tensor when the scheduler
        lends it (first contribution of a lazily-zero leaf), else None.  Returns None to decline (odd gradients)."""
        m, k, n, dt, edges = self.m, self.k, self.n, self.dt, self.edges
        g = da.asarray(g_in)
        if g.shape != (m, n) or g.dtype != dt or g._hv is not None or g._t or not g.size:
            return None
        if "x" in edges and not self.x_relu:
            return None                               # dX without a mask epilogue: the per-edge GEMMs
        g = self.dz_of(g)._contig()
        xv = self.xv
        res = {}
        dw = db = dx = None
        for name, home in zip(edges, homes):
            if name == "w":
                ok = home is not None and home.shape == (k, n) and home.dtype == dt and not home._t and home._hv is None
                dw = home if ok else da.empty((k, n), dt)
                res["w"] = dw
            elif name == "b":
                ok = home is not None and home.size == n and home.dtype == dt and not home._t and home._hv is None
                db = home if ok else da.empty(tuple(self.b.shape), dt)
                res["b"] = db
            else:
                dx = da.empty((m, k), dt)
                dx._tag = xv                          # already multiplied by x's ReLU mask
                res["x"] = dx
        if dw is None:
            dw = da.empty((k, n), dt)                 # w frozen: the launch still needs somewhere to write
        if dx is None and edges == ["w", "b"] and type(dw) is da.LazyArray and type(db) is da.LazyArray:
            # the model's FIRST layer writing into its arena views: the launch can wait for the optimizer (core/model.py)
            owner = getattr(self.b, "_defer_first", None)
            owner = owner() if owner is not None else None
            if owner is not None and owner._defer_first_backward(xv, g, self.wv, dw, db, m, k, n):
                return [dw, db]
        _lib.get().dense_bwd(m, k, n, xv._ptr, g._ptr, self.wv._ptr, dw._ptr, db._ptr if db is not None else None,
                             dx._ptr if dx is not None else None, xv._ptr if dx is not None else None, dw._code())
        return [res[name] for name in edges]


def dense_(x, w, b, relu=False, head_w=None, lazy=False, head_b=None):
    """x @ w + b as ONE GEMM with a bias epilogue (core/layers.py:49); the vjps are the NT / TN GEMMs of
    dot_ (core/ops.py:156-160) and the column-sum of add_'s un-broadcast (:49-55).

    relu=True (Net.forward fuses a Dense that is directly followed by a ReLU layer): the epilogue also applies
    clip(., 0) (core/layers.py:97-98) and keeps the vjp mask z >= 0 (core/ops.py:338, gradient 1 AT zero) in the sign
    bit of zero — z < 0 is stored as -0.0, z >= 0 as |z| — so no pre-activation and no mask array exist.

    Backward is ONE launch per layer whenever the scheduler (Tensor.backward) offers all edges at once
    (`_fused_vjp`): tnn_dense_bwd writes dW and db (straight into the parameters' arena views when they are lent)
    and, if x is itself a sign-encoded ReLU output, dX = (g W^T) * [z_prev >= 0] from the same launch.  That dX is
    tagged as already masked for x's producer, whose own vjp then skips its mask pass; a gradient that reaches a ReLU
    node untagged (several consumers were summed, or a foreign consumer) is masked there — masking twice is harmless
    (the mask is idempotent), so the rule never changes a value.

    head_w (Net.forward, hidden layer in front of a classifier head): the launch also emits the NEXT layer's logits as
    per-tile partial sums (tnn_dense_fwd_head_partials) — they ride on the output array (`_aux`) for the loss node.  More than
    128 rows (head_b, the classifier's bias, is then needed too): the row-panel launch instead (tnn_dense_fwd_rows_head_stats:
    whole logits without the bias + one {max, sum-exp} pair per 16 rows).
    lazy (Net.forward, the classifier layer itself in TRAIN mode): the GEMM is deferred until the logits are first used
    (device_array.LazyArray); softmax_nll_ then produces them together with the loss and this layer's backward."""
    xv, wv, bv = x.values, w.values, b.values
    if xv.ndim != 2 or wv.ndim != 2 or xv.shape[1] != wv.shape[0] or bv.size != wv.shape[1]:
        raise ValueError("dense_: shapes %s @ %s + %s do not line up" % (xv.shape, wv.shape, bv.shape))
    m, k = xv.shape
    n = wv.shape[1]
    dt = da._float_result_dtype(xv, wv)
    x_relu = xv._tag is da.RELU_SIGN and xv.dtype == dt and not xv._t and xv._hv is None
    xc = xv._as_float(dt)._contig()
    x_relu = x_relu and xc is xv                      # the sign bits must be the producer's own buffer
    xv, wv, bv = xc, wv._as_float(dt)._contig(), bv._as_float(dt)._contig()
    code = da._CODE[dt]
    if lazy and not relu and m and n and dt == np.float32:
        def produce(arr, xv=xv, wv=wv, bv=bv):
            _lib.get().gemm_bias_act(0, 0, m, n, k, xv._ptr, k, wv._ptr, n, bv._ptr, _lib.ACT_NONE, 0,
                                     da.DeviceArray._ptr.__get__(arr, da.DeviceArray), n, code)
        out = da.LazyArray.deferred((m, n), dt, produce)
    else:
        lazy = False
        out = da.empty((m, n), dt)
        hw = head_w.values if head_w is not None else None
        hb = head_b.values if head_b is not None else None
        if (hw is not None and 128 < m <= 1024 and relu and n == 128 and k % 4 == 0 and dt == np.float32 and hw.dtype == dt
                and hw.shape == (128, 10) and not hw._t and hw._hv is None and hb is not None and hb.dtype == dt
                and hb.size == 10 and not hb._t and hb._hv is None):
            zfull, pairs = da.empty((m, 10), dt), da.empty(((m + 15) // 16, 2), dt)
            _lib.get().dense_fwd_rows_head_stats(m, n, k, xv._ptr, k, wv._ptr, n, bv._ptr, _lib.ACT_RELU, 1, out._ptr, n,
                                                 hw._ptr, 10, zfull._ptr, hb._ptr, pairs._ptr, code)
            out._aux = (zfull, hw, pairs, hb)         # valid for the classifier weights / bias as they are NOW
        elif (hw is not None and out.size and m <= 128 and dt == np.float32 and hw.dtype == dt and hw.ndim == 2 and hw.shape[0] == n
                and hw.shape[1] <= 16 and not hw._t and hw._hv is None):
            zpart = da.empty(((n + 15) // 16, m, hw.shape[1]), dt)
            _lib.get().dense_fwd_head_partials(m, n, k, xv._ptr, k, wv._ptr, n, bv._ptr, _lib.ACT_RELU if relu else _lib.ACT_NONE,
                                               1 if relu else 0, out._ptr, n, hw._ptr, hw.shape[1], zpart._ptr, code)
            out._aux = (zpart, hw)                    # valid for the classifier weights `hw` as they are NOW
        elif out.size:
            _lib.get().gemm_bias_act(0, 0, m, n, k, xv._ptr, k, wv._ptr, n, bv._ptr,
                                     _lib.ACT_RELU if relu else _lib.ACT_NONE, 1 if relu else 0, out._ptr, n, code)
    if relu:
        out._tag = da.RELU_SIGN

    # the vjps live on ONE context object (bound methods) instead of eight closures per call: the op-level step is host-bound
    ctx = _DenseVjp(b, xv, wv, bv, out, m, k, n, dt, relu, x_relu)
    node = _make_node(x.__class__, out, [(x, ctx.d_x), (w, ctx.d_w), (b, ctx.d_b)])
    edges = ctx.edges = [name for name, t in (("x", x), ("w", w), ("b", b)) if t.requires_grad]
    fused_vjp = ctx.fused_vjp
    node._fused_vjp = fused_vjp
    if lazy:
        node._head = (x, w, b, xv, wv, bv, edges)     # what softmax_nll_ needs to run the head in one launch
    elif relu:
        node._dense_ctx = (x, w, b, xv, wv, bv, edges, x_relu)   # ... and the hidden layer's backward with it
    return node


class _ConvVjp(object):
    """The vjps of one ops.conv2d_ node: `fused_vjp` for Tensor.backward (dw and db from ONE launch, written into the
    parameters' arena views when they are lent; dx only when x is an edge), per-edge forms for everybody else."""
    __slots__ = ("x", "w", "b", "out", "stride", "padding", "relu", "route", "edges")

    def __init__(self, x, w, b, out, stride, padding, relu, route):
        self.x, self.w, self.b, self.out = x, w, b, out       # saved inputs by reference, read at backward time
        self.stride, self.padding, self.relu, self.route = stride, padding, relu, route
        self.edges = ()

    def dz_of(self, g):
        g = da.asarray(g)
        if g._hv is not None or g.shape != self.out.shape:
            g = g._as_float(self.out.dtype)._broadcast_to(self.out.shape)
        return da.mul_signmask(g, self.out) if self.relu else g

    def d_x(self, g):
        return self.d_x_from(self.dz_of(g))

    def d_w(self, g):
        return da.conv2d_bwd_filter(self.x.values, self.dz_of(g), self.w.values.shape, self.stride, self.padding,
                                    with_db=False, route=self.route)[0]

    def d_b(self, g):
        return self.dz_of(g).sum(axis=(0, 2, 3)).reshape(self.b.shape)

    def fused_vjp(self, g, homes):
        edges = self.edges
        dz = self.dz_of(g)
        res = {}
        if "x" in edges:
            res["x"] = self.d_x_from(dz)
        if "w" in edges or "b" in edges:
            home = dict(zip(edges, homes))
            dw, db = da.conv2d_bwd_filter(self.x.values, dz, self.w.values.shape, self.stride, self.padding,
                                          with_db="b" in edges, dw_out=home.get("w"), db_out=home.get("b"),
                                          route=self.route)
            res["w"] = dw
            if db is not None:
                bhome = home.get("b")
                res["b"] = bhome if db is bhome else db.reshape(self.b.shape)
        return [res[name] for name in edges]

    def d_x_from(self, dz):
        return da.conv2d_bwd_data(dz, self.w.values, self.x.values.shape, self.stride, self.padding, route=self.route)


def conv2d_(x, w, b=None, stride=1, padding=0, relu=False, route=None):
    """2-D convolution node: x [N, C, H, W] (*) w [F, C, KH, KW] + b [F] -> [N, F, OH, OW], OH = (H + 2 p - KH) // s + 1
    (cross-correlation, zero padding, integer or pair stride / padding; no dilation, no groups).

    Forward is ONE tnn_conv2d_fwd launch (implicit GEMM on MFMA; relu=True adds the clip(., 0) epilogue and keeps the vjp
    mask z >= 0 in the sign bit of zero, like dense_).  Backward: dx = tnn_conv2d_bwd_data — not computed at all when x does
    not require a gradient (the first layer) — and dw together with db from ONE tnn_conv2d_bwd_filter launch.  Under the
    CPU test twin, and with route="composed" (or device_array.CONV_ROUTE), the same products run as a loop over the filter
    taps and relu=True is a clip followed by the same sign encoding."""
    xv, wv = x.values, w.values
    bv = None if b is None else b.values
    out = da.conv2d(xv, wv, bv, stride, padding, relu=relu, route=route)
    ctx = _ConvVjp(x, w, b, out, stride, padding, relu, route)
    parents = [(x, ctx.d_x), (w, ctx.d_w)] + ([(b, ctx.d_b)] if b is not None else [])
    node = _make_node(x.__class__, out, parents)
    ctx.edges = [name for name, t in (("x", x), ("w", w), ("b", b)) if t is not None and t.requires_grad]
    node._fused_vjp = ctx.fused_vjp
    return node


def max_pool2d_(x, kernel, stride=None, padding=0, route=None):
    """Max pooling node over kernel windows of every [H, W] plane of x [N, C, H, W]; stride None = the kernel; padding is
    -inf and must not exceed kernel // 2.  Tie rule: the FIRST maximum of the window in row-major order receives the whole
    gradient (numpy's argmax rule, the rule da.argmax follows and what a fold of maximum_ gives, whose ties go to the first
    operand).  NaN propagates like max.  The forward records the winner's offset; the vjp (one thread per input pixel, no
    atomics) sums the windows that recorded a pixel, so overlapping windows (stride < kernel) add up."""
    xv = x.values
    shape = tuple(xv.shape)
    values, idx = da.max_pool2d(xv, kernel, stride, padding, route=route)
    return build_unary_ops_tensor(
        x, lambda g: da.max_pool2d_bwd(da.asarray(g)._as_float(values.dtype)._broadcast_to(values.shape), idx, shape,
                                       kernel, stride, padding, route=route), values)


class _AttnVjp(object):
    """The vjps of one ops.attention_ / ops.attention_gqa_ node: `fused_vjp` for Tensor.backward (only the gradients whose
    edges require them: dq from ONE launch — which also produces delta — and dk + dv from ONE launch, written into arena views
    when they are lent), per-edge forms for everybody else.  bwd_q / bwd_kv: the two device_array functions of the node's form
    (grouped: dk and dv have the shapes of the Hkv-head k and v); opts: what they take besides operands, need_* and *_out."""
    __slots__ = ("q", "k", "v", "out", "lse", "bwd_q", "bwd_kv", "opts", "edges")

    def __init__(self, q, k, v, out, lse, bwd_q, bwd_kv, opts):
        self.q, self.k, self.v = q, k, v                       # saved inputs by reference, read at backward time
        self.out, self.lse = out, lse                          # the output and the per-row log-sum-exp: p is recomputed
        self.bwd_q, self.bwd_kv, self.opts = bwd_q, bwd_kv, opts
        self.edges = ()

    def _bwd_q(self, g, need_dq, dq_out=None):
        return self.bwd_q(self.q.values, self.k.values, self.v.values, self.out, g, self.lse, need_dq=need_dq, dq_out=dq_out,
                          **self.opts)

    def _bwd_kv(self, g, delta, need_dk, need_dv, dk_out=None, dv_out=None):
        return self.bwd_kv(self.q.values, self.k.values, self.v.values, g, self.lse, delta, need_dk=need_dk, need_dv=need_dv,
                           dk_out=dk_out, dv_out=dv_out, **self.opts)

    def d_q(self, g):
        return self._bwd_q(g, True)[0]

    def d_k(self, g):
        return self._bwd_kv(g, self._bwd_q(g, False)[1], True, False)[0]

    def d_v(self, g):
        return self._bwd_kv(g, self._bwd_q(g, False)[1], False, True)[1]

    def fused_vjp(self, g, homes):
        edges = self.edges
        home = dict(zip(edges, homes))
        res = {}
        kv = "k" in edges or "v" in edges
        dq, delta = self._bwd_q(g, "q" in edges, home.get("q"))
        if "q" in edges:
            res["q"] = dq
        if kv:
            res["k"], res["v"] = self._bwd_kv(g, delta, "k" in edges, "v" in edges, home.get("k"), home.get("v"))
        return [res[name] for name in edges]


def _lens_opt(lens):
    """lens= as an option of the node (saved for the vjps; never differentiated); None: the options are today's."""
    return {} if lens is None else {"lens": _raw_values(lens)}


def _attn_node(q, k, v, fwd, bwd_q, bwd_kv, **opts):
    """The node of attention_ / attention_gqa_: `fwd` with the options, and an _AttnVjp that hands them to the backward."""
    out, lse = fwd(q.values, k.values, v.values, **opts)
    ctx = _AttnVjp(q, k, v, out, lse, bwd_q, bwd_kv, opts)
    node = _make_node(q.__class__, out, [(q, ctx.d_q), (k, ctx.d_k), (v, ctx.d_v)])
    ctx.edges = [name for name, t in (("q", q), ("k", k), ("v", v)) if t.requires_grad]
    node._fused_vjp = ctx.fused_vjp
    return node


def attention_(q, k, v, causal=False, scale=None, layout="bhtd", route=None, lens=None, **unknown):
    """Scaled-dot-product attention node: softmax(scale q k^T) v, softmax over the key axis, scale = 1 / sqrt(D) by default.

    layout "bhtd": q [..., Tq, D], k [..., Tk, D], v [..., Tk, Dv] -> [..., Tq, Dv] (identical leading dimensions, no
    broadcasting); layout "bthd": q [B, Tq, H, D], k [B, Tk, H, D], v [B, Tk, H, Dv] -> [B, Tq, H, Dv], what a [B T, H D]
    projection reshapes to for free.  causal=True keeps key j for query i iff j <= i (top-left aligned for any Tq, Tk).
    float32 and float64; other dtypes are promoted the way matmul promotes them.  Out of scope: arbitrary masks, dropout,
    bf16 — unknown keyword arguments raise.

    lens (a ragged.Lengths or a dense int64 device array [B], not differentiable; Tq == Tk, layout "bthd" or three-axis
    "bhtd"): sequence b of a right-padded batch has lens[b] live tokens.  Live rows attend over live keys only; dead rows get
    o = +0 and dq = +0, dead keys dk = dv = +0; lens[b] == 0 is an all-zero sequence.  Forward and both backward launches are
    then tnn_varlen_* (include/tnn_varlen.h): the lengths are read on the device, whole 64-row blocks of padding are skipped
    and padding is never read.  A host sequence raises TypeError; a Lengths with a value outside [0, T] raises before any
    launch.  The composed route masks on the host (varlen.py).

    Forward is ONE tnn_attn_fwd launch (online softmax on MFMA; the [Tq, Tk] scores never reach memory) that also keeps the
    per-row log-sum-exp.  Backward recomputes the probabilities from it: dq from one launch (not computed when q does not
    require a gradient), dk + dv from one launch.  Under the CPU test twin, beyond head dimension 128 and with
    route="composed" (or device_array.ATTN_ROUTE) the same mathematics runs on batched products, exp and sums."""
    if unknown:
        raise TypeError("attention_: unsupported arguments %s (masks, dropout and bf16 are out of scope)" % sorted(unknown))
    return _attn_node(q, k, v, da.attention, da.attention_bwd_q, da.attention_bwd_kv, causal=causal, scale=scale, layout=layout,
                      route=route, **_lens_opt(lens))


def attention_gqa_(q, k, v, causal=False, scale=None, route=None, lens=None, **unknown):
    """Grouped-query attention node, layout "bthd": q [B, Tq, H, D], k [B, Tk, Hkv, D], v [B, Tk, Hkv, Dv] -> [B, Tq, H, Dv]
    with H a multiple of Hkv; query head h attends over key / value head h // (H / Hkv).  Hkv == 1 is multi-query attention,
    Hkv == H gives attention_'s result bit for bit.  The causal rule, the scale and the dtypes are attention_'s.

    Forward is ONE tnn_gqa_fwd launch — k and v are never expanded.  Backward: dq from one launch, dk + dv from one launch in
    which a workgroup owns a key block of ONE key / value head and adds its group's query heads in a fixed order (no atomics,
    dk and dv are written once, in the shapes of k and v), into lent arena views when there are any.  Under the CPU test
    twin, with route="composed" (or device_array.GQA_ROUTE), beyond head dimension 128 and for groups above 8, k and v are
    repeated over the group, the composed attention runs and dk / dv are summed over the group axis.  lens: per-sequence
    lengths of a right-padded batch, as attention_ (the same tnn_varlen_* launches, with the group).  Out of scope: masks,
    dropout, bf16, other layouts — unknown keyword arguments raise."""
    if unknown:
        raise TypeError("attention_gqa_: unsupported arguments %s (masks, dropout, bf16 and other layouts than \"bthd\" are out "
                        "of scope)" % sorted(unknown))
    return _attn_node(q, k, v, da.gqa_attention, da.gqa_attention_bwd_q, da.gqa_attention_bwd_kv, causal=causal, scale=scale,
                      route=route, **_lens_opt(lens))


def rope_(q, k=None, rotary=None, offset=0, positions=None, layout="bthd", inverse=False, route=None, **unknown):
    """Rotary position embedding node(s): q alone -> one tensor, q and k -> a pair, rotated by ONE tnn_rope_apply launch.
    q [B, T, H, D] and k [B, T, Hkv, D] (layout "bthd") or [B, H, T, D] and [B, Hkv, T, D] ("bhtd"); rotary: a rope.Rotary
    (the host-computed cos / sin tables, the rotary width R <= D and the pairing).  Row (b, t) sits at position offset + t.
    For a pair (x_lo, x_hi) of a row at position p: y_lo = x_lo c - x_hi s, y_hi = x_hi c + x_lo s with c, s the table
    entries; elements [R, D) pass through.  inverse=True rotates back.  float32 and float64.

    Each output's vjp is the inverse rotation of its own gradient — one launch each, dq and dk arrive separately.
    positions (a ragged.Lengths or a dense int64 device array [B]; T == 1, offset == 0) is INFERENCE ONLY: every sequence's
    position is read on the device, so a captured decoding step keeps its arguments; the results are then LEAF tensors without
    a grad_fn.  Under the CPU test twin and with route="composed" (or device_array.ROPE_ROUTE) the rotation runs on slice
    reads, products and slice assignments.  Out of scope: frequency scaling (NTK / YaRN), bf16 — unknown keyword arguments
    raise."""
    if unknown:
        raise TypeError("rope_: unsupported arguments %s (frequency scaling and bf16 are out of scope)" % sorted(unknown))
    opts = dict(rotary=rotary, offset=offset, layout=layout, route=route)
    out = da.rope(q.values, None if k is None else k.values, positions=_raw_values(positions), inverse=inverse, **opts)
    outs = (out,) if k is None else out
    if positions is not None:
        res = tuple(q.__class__(o, False, []) for o in outs)
        return res[0] if k is None else res

    def node(ts, values):
        def vjp(g):
            g = da.asarray(g)._as_float(values.dtype)._broadcast_to(values.shape)
            return da.rope(g, None, inverse=not inverse, **opts)
        return build_unary_ops_tensor(ts, vjp, values)

    if k is None:
        return node(q, outs[0])
    return node(q, outs[0]), node(k, outs[1])


class _NormVjp(object):
    """The vjps of one ops.layer_norm_ / ops.rms_norm_ node: `fused_vjp` for Tensor.backward (ONE tnn_norm_bwd call for
    whichever of x, gamma, beta require gradients, written into arena views when they are lent), per-edge forms for
    everybody else."""
    __slots__ = ("x", "gamma", "beta", "mean", "rstd", "kind", "route", "edges")

    def __init__(self, x, gamma, beta, mean, rstd, kind, route):
        self.x, self.gamma, self.beta = x, gamma, beta         # saved inputs by reference, read at backward time
        self.mean, self.rstd = mean, rstd                      # the row statistics of the forward launch
        self.kind, self.route = kind, route
        self.edges = ()

    def _bwd(self, g, names, home=None):
        home = home or {}
        dx, dgamma, dbeta = da.norm_bwd(self.x.values, g, None if self.gamma is None else self.gamma.values, self.mean,
                                        self.rstd, kind=self.kind, route=self.route, need_dx="x" in names,
                                        need_dgamma="gamma" in names, need_dbeta="beta" in names, dx_out=home.get("x"),
                                        dgamma_out=home.get("gamma"), dbeta_out=home.get("beta"))
        if dgamma is not None and dgamma is not home.get("gamma"):
            dgamma = dgamma.reshape(self.gamma.shape)
        if dbeta is not None and dbeta is not home.get("beta"):
            dbeta = dbeta.reshape(self.beta.shape)
        return {"x": dx, "gamma": dgamma, "beta": dbeta}

    def d_x(self, g):
        return self._bwd(g, ("x",))["x"]

    def d_gamma(self, g):
        return self._bwd(g, ("gamma",))["gamma"]

    def d_beta(self, g):
        return self._bwd(g, ("beta",))["beta"]

    def fused_vjp(self, g, homes):
        edges = self.edges
        res = self._bwd(g, edges, dict(zip(edges, homes)))
        return [res[name] for name in edges]


def _norm_node(kind, x, gamma, beta, eps, route):
    gv = None if gamma is None else gamma.values
    if kind == "layer":
        out, mean, rstd = da.layer_norm(x.values, gv, None if beta is None else beta.values, eps=eps, route=route)
    else:
        mean = None
        out, rstd = da.rms_norm(x.values, gv, eps=eps, route=route)
    ctx = _NormVjp(x, gamma, beta, mean, rstd, kind, route)
    named = [("x", x, ctx.d_x), ("gamma", gamma, ctx.d_gamma), ("beta", beta, ctx.d_beta)]
    node = _make_node(x.__class__, out, [(t, fn) for _, t, fn in named if t is not None])
    ctx.edges = [name for name, t, _ in named if t is not None and t.requires_grad]
    node._fused_vjp = ctx.fused_vjp
    return node


def layer_norm_(x, gamma=None, beta=None, eps=1e-5, route=None, **unknown):
    """Layer normalisation node over the LAST axis of x (any rank >= 1): (x - mean) * rstd * gamma + beta with the biased
    variance and rstd = 1 / sqrt(var + eps).  gamma / beta: [N] or [1, N] tensors, or None (1 and 0).  float32 and float64.

    Forward is ONE tnn_norm_fwd launch that reads x once, writes y once and keeps the row statistics; backward is ONE
    tnn_norm_bwd call for whichever of x, gamma, beta require gradients (one pass over x and dy, the parameter gradients
    reduced in a fixed order).  Under the CPU test twin, for rows wider than norm.BLOCK_MAX_N and with route="composed" (or
    device_array.NORM_ROUTE) the same mathematics runs on sums, products and a square root.  Out of scope: bf16, a fused
    residual add, dropout — unknown keyword arguments raise."""
    if unknown:
        raise TypeError("layer_norm_: unsupported arguments %s" % sorted(unknown))
    return _norm_node("layer", x, gamma, beta, eps, route)


def rms_norm_(x, gamma=None, eps=1e-5, route=None, **unknown):
    """RMS normalisation node over the LAST axis of x: x * rstd * gamma with rstd = 1 / sqrt(mean(x^2) + eps); no mean and no
    beta.  Launches and routes: layer_norm_.  Unknown keyword arguments raise."""
    if unknown:
        raise TypeError("rms_norm_: unsupported arguments %s (RMS norm takes no beta)" % sorted(unknown))
    return _norm_node("rms", x, gamma, None, eps, route)


def gelu_(x, approximate="none", route=None, **unknown):
    """GELU node.  approximate="none": 0.5 x (1 + erf(x / sqrt(2))); "tanh": 0.5 x (1 + tanh(sqrt(2 / pi) (x + 0.044715
    x^3))).  One launch forward, one backward (the slope is recomputed from x).  The composed route (CPU test twin,
    route="composed") exists for the tanh form only; the exact form raises there.  Unknown keyword arguments raise."""
    if unknown:
        raise TypeError("gelu_: unsupported arguments %s" % sorted(unknown))
    xv = x.values
    out = da.gelu(xv, approximate=approximate, route=route)
    return build_unary_ops_tensor(x, lambda g: da.gelu_bwd(xv, g, approximate=approximate, route=route), out)


def gated_(gate, up=None, act="silu", packed=False, route=None, **unknown):
    """Gated activation node: act(gate) * up elementwise over tensors [.., F] — SwiGLU with act="silu", GEGLU with
    "gelu_tanh" or "gelu" (the exact form, native route only); up=None: act(gate) alone.  packed=True: `gate` is ONE tensor
    [.., 2 F], the gate columns followed by the up columns (what one Dense(2 F) produces); both halves are read in place.
    float32 and float64.

    Forward is ONE tnn_gated_fwd launch.  Backward is ONE tnn_gated_bwd launch: the packed node's vjp writes dz [.., 2 F]
    (dgate columns, then dup columns), so the Dense backward behind it is one GEMM; the two-tensor node gets dgate and dup from
    the same launch, and a side that does not require a gradient is not computed.  Under the CPU test twin and with
    route="composed" (or device_array.GATED_ROUTE) the same mathematics runs on sigmoid / tanh and products.  Out of scope:
    bf16, a GEMM-epilogue form — unknown keyword arguments raise."""
    if unknown:
        raise TypeError("gated_: unsupported arguments %s (bf16 and GEMM-epilogue fusion are out of scope)" % sorted(unknown))
    gv = gate.values
    if packed and up is not None:
        raise ValueError("gated_: packed=True takes ONE array [.., 2 F] (gate columns, then up columns), not gate and up")
    if packed or up is None:
        out = da.gated(gv, None, act=act, packed=packed, route=route)
        if packed:
            return build_unary_ops_tensor(gate, lambda g: da.gated_bwd(gv, None, g, act=act, packed=True, route=route), out)
        return build_unary_ops_tensor(gate, lambda g: da.gated_bwd(gv, None, g, act=act, route=route)[0], out)
    uv = up.values
    out = da.gated(gv, uv, act=act, route=route)

    def both(g, need_dgate, need_dup):
        return da.gated_bwd(gv, uv, g, act=act, route=route, need_dgate=need_dgate, need_dup=need_dup)

    node = build_binary_ops_tensor(gate, up, lambda g: both(g, True, False)[0], lambda g: both(g, False, True)[1], out)
    needs = (gate.requires_grad, up.requires_grad)
    node._fused_vjp = lambda g, homes: [d for d, need in zip(both(g, *needs), needs) if need]
    return node


def silu_(x, route=None, **unknown):
    """SiLU node: x * sigmoid(x) in the overflow-free form of include/tnn_gated.h — gated_ without `up`: one launch forward,
    one backward.  Unknown keyword arguments raise."""
    if unknown:
        raise TypeError("silu_: unsupported arguments %s" % sorted(unknown))
    return gated_(x, None, act="silu", route=route)


def dropout_(x, p, residual=None, generator=None, route=None, first=0, **unknown):
    """Dropout node: keep ? x / (1 - p) : 0 elementwise, plus `residual` (a tensor of x's shape) when there is one — the fused
    residual form, in which ONE launch replaces a block's residual add.  The keep decision of an element is the 24-bit draw of
    its stream index (first + its row-major position) of ONE call of `generator` (rng.Generator; None: rng.default_generator)
    against round(p 2^24): dropout.py states the generator exactly.  float32 and float64.

    p == 0 returns x itself (or x + residual through add_) without any new launch and without consuming a call.  Otherwise
    forward is a one-thread ticket launch and ONE tnn_dropout_fwd launch, backward ONE tnn_dropout_bwd launch that regenerates
    the mask from the forward's ticket — so it is right after later draws and inside a replayed graph; the residual's gradient
    is the incoming gradient itself.  Under the CPU test twin and with route="composed" (or device_array.DROPOUT_ROUTE) the
    mask is drawn on the host with the planner's generator and applied by the existing multiply, masked select and add; that
    route raises inside an open graph capture.  This node applies dropout whenever it is called: the TRAIN / TEST decision
    belongs to the layers.  Out of scope: bf16, per-sample or ragged masks — unknown keyword arguments raise."""
    if unknown:
        raise TypeError("dropout_: unsupported arguments %s" % sorted(unknown))
    from ..dropout import threshold_of
    if threshold_of(p) == 0 and float(p) == 0.0:
        return x if residual is None else add_(residual, x)
    out, mask = da.dropout(x.values, p, None if residual is None else residual.values, generator=generator, route=route,
                           first=first)

    def d_x(g):
        return da.dropout_bwd(g, mask)

    if residual is None:
        return build_unary_ops_tensor(x, d_x, out)
    return build_binary_ops_tensor(x, residual, d_x, lambda g: da.asarray(g), out)


def _index_values(obj, limit, what, also=None):
    """ids / targets given as a Tensor, a DeviceArray or numpy -> a dense int64 device array; host values are range-checked
    once, here (IndexError); they never require a gradient."""
    obj = getattr(obj, "values", obj) if hasattr(obj, "requires_grad") else obj
    return da._token_ids(obj, limit, what, also)[0]


class _EmbedVjp(object):
    """The vjps of one ops.embedding_ node: `fused_vjp` for Tensor.backward (ONE tnn_embed_bwd call for whichever of table /
    pos require gradients, written into arena views when they are lent), per-edge forms for everybody else."""
    __slots__ = ("table", "pos", "ids", "padding_idx", "route", "edges")

    def __init__(self, table, pos, ids, padding_idx, route):
        self.table, self.pos, self.ids = table, pos, ids
        self.padding_idx, self.route = padding_idx, route
        self.edges = ()

    def _bwd(self, g, names, home=None):
        home = home or {}
        dtable, dpos = da.embedding_bwd(g, self.ids, self.table.shape, None if self.pos is None else self.pos.shape,
                                        self.padding_idx, need_dtable="table" in names, need_dpos="pos" in names,
                                        dtable_out=home.get("table"), dpos_out=home.get("pos"), route=self.route)
        return {"table": dtable, "pos": dpos}

    def d_table(self, g):
        return self._bwd(g, ("table",))["table"]

    def d_pos(self, g):
        return self._bwd(g, ("pos",))["pos"]

    def fused_vjp(self, g, homes):
        edges = self.edges
        res = self._bwd(g, edges, dict(zip(edges, homes)))
        return [res[name] for name in edges]


def embedding_(table, ids, pos=None, padding_idx=None, route=None, **unknown):
    """Token embedding node: out[..., :] = table[ids[...], :] (+ pos[t, :], t the index along the last axis of ids).  table
    [V, E] and pos [T', E] (T' >= the last extent of ids) are tensors; ids — a Tensor, a DeviceArray or numpy, integers of any
    shape — never require a gradient.  Host ids outside [0, V) raise IndexError; device-resident ones are not read back and
    give a zero token row.  The vjp w.r.t. the table is a scatter-ADD: a token that occurs n times receives the sum of its n
    gradients (`table[ids]` through getitem_ keeps only the last one); padding_idx, when given, receives none.

    Forward is ONE tnn_embed_fwd launch, backward ONE tnn_embed_bwd call for whichever of table / pos require gradients — a
    deterministic sort-and-segment sum without floating-point atomics.  Under the CPU test twin and with route="composed" (or
    device_array.TOKEN_ROUTE) the same mathematics runs on a row gather and a one-hot product, whose backward reads the ids
    on the host and therefore cannot be captured.  Out of scope: bf16, max_norm, sparse gradients — unknown keyword arguments
    raise."""
    if unknown:
        raise TypeError("embedding_: unsupported arguments %s" % sorted(unknown))
    idd = _index_values(ids, int(table.shape[0]), "embedding")
    if padding_idx is not None and not 0 <= int(padding_idx) < int(table.shape[0]):
        raise ValueError("embedding: padding_idx %d outside [0, %d)" % (int(padding_idx), int(table.shape[0])))
    out = da.embedding(table.values, idd, None if pos is None else pos.values, route=route)
    ctx = _EmbedVjp(table, pos, idd, padding_idx, route)
    named = [("table", table, ctx.d_table), ("pos", pos, ctx.d_pos)]
    node = _make_node(table.__class__, out, [(t, fn) for _, t, fn in named if t is not None])
    ctx.edges = [name for name, t, _ in named if t is not None and t.requires_grad]
    node._fused_vjp = ctx.fused_vjp
    return node


def _raw_values(obj):
    return obj.values if hasattr(obj, "requires_grad") else obj


def attention_decode_(q, k_cache, v_cache, length, k_new=None, v_new=None, scale=None, layout="bthd", route=None, splits=None,
                      **unknown):
    """One decoding step of attention, INFERENCE ONLY: o [B, H, Dv] = softmax(scale q k^T) v for one query per (batch, head)
    over the live rows of a key / value cache; with k_new / v_new the step's own row is first written into cache row `length`
    (the caches — DeviceArrays or Tensors — are modified in place).  q [B, H, D]; `length` is a host integer shared by the
    batch; layout "bthd" (caches [B, Tmax, H, D]) or "bhtd" ([B, H, Tmax, D]).  No mask: a decoding step sees every cached key.

    The result is a LEAF tensor without a grad_fn — nothing here is differentiable, and the operands' graphs are not
    extended.  ONE tnn_decode_attn call, whose keys are split over enough workgroups to cover the machine (decoding.py);
    under the CPU test twin and with route="composed" (or device_array.DECODE_ROUTE) a slice assignment and the composed
    attention.  A ragged batch — every sequence at its own length — takes attention_decode_ragged_, grouped-query heads
    attention_decode_gqa_, T > 1 new rows over a filled cache (chunked prefill) attention_extend_.  Out of scope: bf16 —
    unknown keyword arguments raise."""
    if unknown:
        raise TypeError("attention_decode_: unsupported arguments %s (bf16 is out of scope; a ragged batch takes "
                        "attention_decode_ragged_, grouped-query heads attention_decode_gqa_)" % sorted(unknown))
    out = da.attention_decode(q.values, _raw_values(k_cache), _raw_values(v_cache), length,
                              None if k_new is None else k_new.values, None if v_new is None else v_new.values, scale=scale,
                              layout=layout, route=route, splits=splits)
    return q.__class__(out, False, [])


def sample_rows_(logits, u=None, temperature=1.0, top_k=None, route=None, **unknown):
    """The next token of every row, INFERENCE ONLY: ids int64 [M] (a leaf tensor on the device, no grad_fn) from logits [M, V]
    and one uniform number per row, u [M] in [0, 1) — a Tensor, a DeviceArray or numpy; not needed at temperature 0, which is
    the first index of the row maximum.  Otherwise the inverse CDF of softmax(logits / temperature) restricted to the top_k
    largest (None: all; ties at the threshold go to the lowest indices).  ONE tnn_sample_rows launch that reads nothing back:
    the ids can feed embedding_ as they are.  The composed route (CPU test twin, route="composed") reads the logits back and
    cannot be captured.  Out of scope: top-p, a device random generator, bf16 — unknown keyword arguments raise."""
    if unknown:
        raise TypeError("sample_rows_: unsupported arguments %s (top-p is out of scope)" % sorted(unknown))
    ids = da.sample_rows(logits.values, None if u is None else _raw_values(u), temperature=temperature, top_k=top_k, route=route)
    return logits.__class__(ids, False, [])


def attention_decode_ragged_(q, k_cache, v_cache, lens, k_new, v_new, scale=None, layout="bthd", route=None, splits=None,
                             **unknown):
    """attention_decode_ with the append for a RAGGED batch, INFERENCE ONLY: sequence b writes its new row into cache row
    lens[b] and attends over keys [0, lens[b]].  lens: a ragged.Lengths (device int64 [B] and its host mirror) or a dense int64
    device array — it is read ON THE DEVICE, so the call's arguments do not change from step to step and a token step can be
    captured into a graph.  ONE tnn_ragged_decode_attn call whose grid depends on the shapes alone (ragged.py); under the CPU
    test twin and with route="composed" (or device_array.RAGGED_ROUTE) a loop over the sequences with the host lengths.
    The result is a LEAF tensor without a grad_fn.  Grouped-query heads take attention_decode_ragged_gqa_.  Out of scope: bf16 —
    unknown keyword arguments raise."""
    if unknown:
        raise TypeError("attention_decode_ragged_: unsupported arguments %s (bf16 is out of scope; grouped-query heads take "
                        "attention_decode_ragged_gqa_)"
                        % sorted(unknown))
    out = da.attention_decode_ragged(q.values, _raw_values(k_cache), _raw_values(v_cache), _raw_values(lens), k_new.values,
                                     v_new.values, scale=scale, layout=layout, route=route, splits=splits)
    return q.__class__(out, False, [])


def attention_decode_gqa_(q, k_cache, v_cache, length, k_new=None, v_new=None, scale=None, layout="bthd", route=None,
                          splits=None, **unknown):
    """attention_decode_ for grouped-query heads, INFERENCE ONLY: q [B, H, D] over caches that hold Hkv heads ("bthd":
    [B, Tmax, Hkv, D]; "bhtd": [B, Hkv, Tmax, D]), k_new [B, Hkv, D], v_new [B, Hkv, Dv]; query head h reads key / value head
    h // (H / Hkv).  ONE tnn_gqa_decode_attn call in which a workgroup serves all H / Hkv queries of a key / value head from
    one read of each cached row — the cache and the bytes of a step are H / Hkv times smaller than with repeated heads.
    Composed route (CPU test twin, route="composed" or device_array.GQA_ROUTE, groups above 8): the append by a slice
    assignment and the composed attention over the live prefix repeated over the group.  The result is a LEAF tensor without
    a grad_fn.  T > 1 new rows over a filled cache (chunked prefill) take attention_extend_.  Out of scope: bf16 — unknown
    keyword arguments raise."""
    if unknown:
        raise TypeError("attention_decode_gqa_: unsupported arguments %s (bf16 is out of scope; a ragged batch takes "
                        "attention_decode_ragged_gqa_)" % sorted(unknown))
    out = da.gqa_decode(q.values, _raw_values(k_cache), _raw_values(v_cache), length,
                        None if k_new is None else k_new.values, None if v_new is None else v_new.values, scale=scale,
                        layout=layout, route=route, splits=splits)
    return q.__class__(out, False, [])


def attention_decode_ragged_gqa_(q, k_cache, v_cache, lens, k_new, v_new, scale=None, layout="bthd", route=None, splits=None,
                                 **unknown):
    """attention_decode_ragged_ for grouped-query heads, INFERENCE ONLY: the operands of attention_decode_gqa_ with lens (a
    ragged.Lengths or a dense int64 device array [B]) read ON THE DEVICE.  ONE tnn_gqa_ragged_decode_attn call whose arguments
    are fixed by the shapes, so a token step can be captured into a graph; the composed route loops over the sequences with
    the host lengths and raises inside an open capture.  The result is a LEAF tensor without a grad_fn — unknown keyword
    arguments raise."""
    if unknown:
        raise TypeError("attention_decode_ragged_gqa_: unsupported arguments %s (bf16 is out of scope)" % sorted(unknown))
    out = da.gqa_decode(q.values, _raw_values(k_cache), _raw_values(v_cache), None, k_new.values, v_new.values,
                        lens=_raw_values(lens), scale=scale, layout=layout, route=route, splits=splits)
    return q.__class__(out, False, [])


def attention_extend_(q, k_cache, v_cache, length, k_new, v_new, scale=None, layout="bthd", route=None, **unknown):
    """Attention of T NEW rows per sequence over a key / value cache and over themselves, with the append, INFERENCE ONLY —
    chunked prefill, the continuation of a cached sequence, the verification of drafted tokens.  layout "bthd": q [B, T, H, D],
    k_new [B, T, Hkv, D], v_new [B, T, Hkv, Dv], caches [B, Tmax, Hkv, D | Dv] -> o [B, T, H, Dv] ("bhtd": heads before rows);
    query row i sits at position length + i and sees the keys j <= length + i (the bottom-right causal rule), query head h
    reads key / value head h // (H / Hkv) — Hkv == H is plain multi-head attention.  The caches (DeviceArrays or Tensors)
    are modified in place: rows [length, length + T) become k_new / v_new.  `length` is a host integer shared by the batch.

    The result is a LEAF tensor without a grad_fn.  ONE tnn_extend_attn call whose rows do not depend on how they are cut into
    calls (include/tnn_extend.h); under the CPU test twin and with route="composed" (or device_array.EXTEND_ROUTE) a slice
    assignment and the composed attention with an offset mask.  Out of scope: lengths read on the device (ragged chunks),
    bf16 — unknown keyword arguments raise."""
    if unknown:
        raise TypeError("attention_extend_: unsupported arguments %s (ragged chunks and bf16 are out of scope)" % sorted(unknown))
    out = da.attention_extend(q.values, _raw_values(k_cache), _raw_values(v_cache), length, k_new.values, v_new.values,
                              scale=scale, layout=layout, route=route)
    return q.__class__(out, False, [])


def embedding_at_(table, ids, positions, pos=None, route=None, **unknown):
    """The embedding of a ragged decoding step, INFERENCE ONLY: out[..., :] = table[ids[...], :] + pos[positions[...], :] —
    every id sits at its own position.  table [V, E] and pos [Tpos, E] (or None) are tensors; ids (a Tensor or a DeviceArray,
    int64 on the device) and positions (likewise, or a ragged.Lengths) are read on the device and never on the host: an id
    outside [0, V) gives a zero token row, a position outside [0, Tpos) a zero position row.  ONE tnn_ragged_embed_fwd launch;
    composed route: two row gathers and an addition.  The result is a LEAF tensor without a grad_fn — unknown keyword
    arguments raise."""
    if unknown:
        raise TypeError("embedding_at_: unsupported arguments %s" % sorted(unknown))
    out = da.embedding_at(table.values, _raw_values(ids), _raw_values(positions), None if pos is None else pos.values, route=route)
    return table.__class__(out, False, [])


def cross_entropy_(logits, targets, ignore_index=None, reduction="mean", route=None, **unknown):
    """Per-row softmax cross-entropy node over the LAST axis of logits [..., V] with integer targets [...] (a Tensor, a
    DeviceArray or numpy; never a gradient): the sum ("sum") or the mean over the counted rows ("mean") of
    log sum exp(x) - x[target].  Rows whose target equals ignore_index are not counted and get no gradient; when nothing is
    counted the loss is 0 and every gradient is zero.  Host targets that are neither in [0, V) nor ignore_index raise
    IndexError; device-resident ones are not read back (out-of-range rows are not counted).

    Forward is ONE tnn_xent_fwd call that reads every logit once and keeps the per-row log-sum-exp; backward ONE tnn_xent_bwd
    launch that takes the upstream gradient and the row count as device scalars (nothing is read on the host).  Composed
    route: as for embedding_.  Out of scope: label smoothing, class weights, bf16 — unknown keyword arguments raise."""
    if unknown:
        raise TypeError("cross_entropy_: unsupported arguments %s" % sorted(unknown))
    tg = _index_values(targets, int(logits.shape[-1]), "cross_entropy", also=ignore_index)
    loss, _, lse, count = da.cross_entropy(logits.values, tg, ignore_index=ignore_index, reduction=reduction, route=route)

    def grad_fn(g, out=None):
        return da.cross_entropy_bwd(logits.values, tg, lse, count, g, ignore_index=ignore_index, reduction=reduction,
                                    route=route, dlogits_out=out)
    node = build_unary_ops_tensor(logits, grad_fn, loss)
    node._fused_vjp = lambda g, homes: [grad_fn(g, homes[0])]
    return node


def _softmax_head(logits, labels):
    """The classifier head as ONE launch when the logits are still pending (dense_(lazy=True)) and the shapes are the ones
    tnn_mlp_head_tick takes: last Dense forward (core/layers.py:49) + whole-batch softmax NLL (core/losses.py:24-32) + the last
    Dense's backward (core/ops.py:156-160, :52-54, ReLU mask :342-343), i.e. three of the op-level step's launches.  The
    backward part is SPECULATIVE: its results are handed over when backward() reaches the Dense node with the loss node's own
    dz (the default seed 1.0); any other seed, a second backward or a foreign consumer recomputes through the ordinary vjps.
    Returns None when the fusion does not apply."""
    head = getattr(logits, "_head", None)
    z = logits._values
    if head is None or type(z) is not da.LazyArray or not z.pending:
        return None
    x, w, b, xv, wv, bv, edges = head
    y = as_tensor(labels).values
    m, c = z.shape
    hdim = wv.shape[0]
    aux = xv._aux
    # more than 128 rows: only with what the row-panel forward left behind (whole logits + panel statistics for THESE weights)
    rows_form = (m > 128 and aux is not None and len(aux) == 4 and aux[1] is wv and aux[3] is bv
                 and aux[0].shape == (m, c) and hdim == 128 and c == 10)
    if (y.shape != z.shape or xv._tag is not da.RELU_SIGN or xv._t or xv._hv is not None or wv._t or bv._t
            or not (rows_form or (m <= 128 and _head_fits(m, hdim, c)))):
        return None
    dt = np.dtype(np.float32)
    y = y._as_float(dt)._contig()
    lib = _lib.get()
    stats, loss, dz = da.empty((2,), dt), da.empty((), dt), da.empty((m, c), dt)

    # Speculative results may be written straight into a parameter's arena view, but a LATER loss evaluation (second forward +
    # loss before this one's backward) would write ITS results into the same view: every view written here is stamped with this
    # call's token on its tensor, and the hand-over below adopts a view only while the stamp is still this call's.
    owner = object()

    def dest(t, shape):
        """The tensor's arena view when its gradient is lazily zero (what the scheduler would lend), else a fresh buffer."""
        home = getattr(t, "_grad_home", None)
        if (t.requires_grad and home is not None and t._grad is None and t._grad_zero and not t.dependency
                and home.size == math.prod(shape) and home.dtype == dt and not home._t and home._hv is None):
            t._spec_owner = owner
            return home, True
        return da.empty(shape, dt), False
    dw, dw_home = dest(w, (hdim, c))
    db, db_home = dest(b, tuple(b.shape))
    zpart = None
    if rows_form:
        zpart = aux[0]
    elif aux is not None and aux[1] is wv and aux[0].shape == (hdim // 16, m, c):
        zpart = aux[0]
    generic = logits._fused_vjp

    # ---- with the hidden layer's backward in the same launch (tnn_mlp_head_bwd_tick: the 4-launch trainer's third launch)
    # when that layer is a fused Dense+ReLU node whose own input carries a ReLU mask: its dz is derived inside the tiles and
    # never stored, so the gradient handed to the hidden activation is a DEFERRED array (computed by the ordinary vjp only
    # if somebody reads that intermediate .grad) which the hidden node recognises and answers with the precomputed results
    hid = getattr(x, "_dense_ctx", None)
    if (hid is not None and zpart is not None and x.requires_grad and len(x.dependency) == len(hid[6])
            and hid[7] and hid[3].shape[1] % 16 == 0 and hid[4].dtype == dt and not hid[4]._t and "x" in hid[6]):
        x0, w1, b1, x0v, w1v, b1v, edges1, _ = hid
        n_in = x0v.shape[1]
        dw1, dw1_home = dest(w1, (n_in, hdim))
        db1, db1_home = dest(b1, tuple(b1.shape))
        dx0 = da.empty((m, n_in), dt)
        dx0._tag = x0v
        # Adam's bias-correction powers for the coming step are advanced by one thread of this launch when the classifier's
        # parameters belong to a Model whose optimizer asks for it (once per optimizer step: Adam.take_tick)
        opt = getattr(w, "_tick_optimizer", None)
        opt = opt() if opt is not None else None
        tick = opt.take_tick() if opt is not None else None
        pows, tb1, tb2 = tick if tick is not None else (None, 0.0, 0.0)
        if rows_form:
            pairs = aux[2]
            lib.mlp_head_bwd_tick_ext(m, m, n_in, hdim, c, x0v._ptr, w1v._ptr, xv._ptr, wv._ptr, bv._ptr, y._ptr, zpart._ptr,
                                      pairs._ptr, -pairs.shape[0], z.fulfilled_ptr(), dz._ptr, stats._ptr, loss._ptr, dw._ptr,
                                      db._ptr, dw1._ptr, db1._ptr, dx0._ptr, _lib.F32, pows, tb1, tb2)
        else:
            lib.mlp_head_bwd_tick(m, n_in, hdim, c, x0v._ptr, w1v._ptr, xv._ptr, wv._ptr, bv._ptr, y._ptr, zpart._ptr,
                                  z.fulfilled_ptr(), dz._ptr, stats._ptr, loss._ptr, dw._ptr, db._ptr, dw1._ptr, db1._ptr,
                                  dx0._ptr, _lib.F32, pows, tb1, tb2)

        def hidden_dz(arr, dz=dz, wv=wv, xv=xv):     # only if the intermediate gradient is actually looked at
            val = da.mul_signmask(dz @ wv.T, xv)
            _lib.get().memcpy_d2d(da.DeviceArray._ptr.__get__(arr, da.DeviceArray), val._ptr, val.nbytes)
        dx = da.LazyArray.deferred((m, hdim), dt, hidden_dz)
        dx._tag = xv
        pre1 = {"x": (dx0, False), "w": (dw1, dw1_home), "b": (db1, db1_home)}
        stamped1 = {"w": w1, "b": b1}
        generic1 = x._fused_vjp

        x_ref = weakref.ref(x)                        # not x itself: x._fused_vjp -> this closure -> x would be a cycle that
                                                      # keeps the whole step's graph (and its buffers) alive until the cycle GC

        def hidden_vjp(g_in, homes):
            x = x_ref()
            state = x._head_pre
            x._head_pre = None
            if state is not None and g_in is dx:
                out = []
                for name, home in zip(edges1, homes):
                    arr, wrote_home = pre1[name]
                    if wrote_home and (home is not arr or getattr(stamped1[name], "_spec_owner", None) is not owner):
                        out = None                    # not this tensor's to adopt, or overwritten by a later loss evaluation
                        break
                    out.append(arr)
                if out is not None:
                    return out
            return generic1(g_in, homes)
        x._head_pre = True
        x._fused_vjp = hidden_vjp
    elif rows_form:
        return None                                   # the one-launch head without the hidden backward exists for <= 128 rows only
    else:
        dx = da.empty((m, hdim), dt) if x.requires_grad else None
        lib.mlp_head_tick(m, hdim, c, xv._ptr, wv._ptr, bv._ptr, y._ptr, None if zpart is None else zpart._ptr,
                          z.fulfilled_ptr(), dz._ptr, stats._ptr, loss._ptr, dw._ptr, db._ptr, None if dx is None else dx._ptr,
                          _lib.F32, None, 0.0, 0.0)
        if dx is not None:
            dx._tag = xv                              # already multiplied by x's ReLU mask
    pre = {"x": (dx, False), "w": (dw, dw_home), "b": (db, db_home)}
    stamped = {"w": w, "b": b}

    logits_ref = weakref.ref(logits)                  # see x_ref above

    def fused_vjp(g_in, homes):
        logits = logits_ref()
        state = logits._head_pre
        logits._head_pre = None                       # one hand-over; whatever comes later is recomputed
        if state is not None and g_in is dz:
            out = []
            for name, home in zip(edges, homes):
                arr, wrote_home = pre[name]
                if wrote_home and (home is not arr or getattr(stamped[name], "_spec_owner", None) is not owner):
                    out = None                        # the arena view is no longer this tensor's to adopt, or a later loss
                    break                             # evaluation has overwritten it
                out.append(arr)
            if out is not None:
                return out
        return generic(g_in, homes)
    logits._head_pre = True
    logits._fused_vjp = fused_vjp

    def d_logits(g):
        g = da.asarray(g)
        if g._hv is not None and float(g._hv) == 1.0:
            return dz
        return g * dz
    return build_unary_ops_tensor(logits, d_logits, loss)


_HEAD_FITS = {}


def _head_fits(m, hdim, c):
    key = (m, hdim, c)
    if key not in _HEAD_FITS:
        import ctypes
        fits = ctypes.c_int(0)
        _lib.get().mlp_head_fits(m, hdim, c, _lib.F32, ctypes.byref(fits))
        _HEAD_FITS[key] = bool(fits.value)
    return _HEAD_FITS[key]


def sigmoid_(ts):
    """1 / (1 + exp(-x)) in one kernel; vjp g * s * (1 - s) (closed form; the reference's Sigmoid raises,
    SURVEY F7)."""
    s = da.sigmoid(ts.values)
    return build_unary_ops_tensor(ts, lambda g: g * (s * (1.0 - s)), s)


def softmax_nll_(logits, labels, comm=None):
    """core/losses.py:24-32 as one node: whole-batch max / sum-exp, loss and dz = p - (e*y/q)/m.

    With a communicator the {max, sum-exp} pair of every shard is all-gathered and merged, m is the GLOBAL
    batch size, and the returned loss is this shard's share (the shares add up to the global loss)."""
    if comm is None or comm.world == 1:
        fused = _softmax_head(logits, labels)
        if fused is not None:
            return fused
    z, y = logits.values, as_tensor(labels).values
    dt = z.dtype if z.dtype.kind == "f" else da.get_default_float()
    z, y = z._as_float(dt)._contig(), y._as_float(dt)._contig()
    if z.ndim != 2 or y.shape != z.shape:
        raise ValueError("softmax_nll_: logits %s and labels %s must be equal 2-D shapes" % (z.shape, y.shape))
    m, c = z.shape
    lib = _lib.get()
    stats = da.empty((2,), dt)
    loss = da.empty((), dt)
    dz = da.empty((m, c), dt)
    if comm is None or comm.world == 1:
        # one launch (stats + loss + dz); batches that do not fit one workgroup take the multi-launch form inside
        lib.softmax_nll_fused(z._ptr, y._ptr, m, c, stats._ptr, loss._ptr, dz._ptr, z._code())
    else:
        lib.softmax_nll_stats(z._ptr, m, c, stats._ptr, stats._code())
        stats = comm.merge_softmax_stats(stats)
        lib.softmax_nll_fwd_bwd(z._ptr, y._ptr, m, c, m * comm.world, stats._ptr, loss._ptr, dz._ptr, z._code())
    def d_logits(g):
        g = da.asarray(g)
        if g._hv is not None and float(g._hv) == 1.0:       # the default seed of loss.backward(): no scaling launch
            return dz
        return g * dz
    return build_unary_ops_tensor(logits, d_logits, loss)


# ---------------------------------------------------------------------- anything-in wrappers
def max(obj, axis=None):
    return max_(as_tensor(obj), axis=axis)


def min(obj, axis=None):
    """not in the reference's wrapper list (it only has min_); added for symmetry with max"""
    return min_(as_tensor(obj), axis=axis)


def maximum(obj1, obj2):
    return maximum_(as_tensor(obj1), as_tensor(obj2))


def minimum(obj1, obj2):
    return minimum_(as_tensor(obj1), as_tensor(obj2))


def exp(obj):
    return exp_(as_tensor(obj))


def sum(obj, axis=None):
    return sum_(as_tensor(obj), axis=axis)


def log(obj):
    return log_(as_tensor(obj))


def reshape(obj, newshape):
    return reshape_(as_tensor(obj), newshape)


def pad(obj, pad_width, mode="constant"):
    return pad_(as_tensor(obj), pad_width, mode=mode)


def flatten(obj):
    return flatten_(as_tensor(obj))


def clip(obj, min=None, max=None):
    return clip_(as_tensor(obj), min, max)


def conv2d(obj, w, b=None, stride=1, padding=0, dilation=1, groups=1):
    """not in the reference: see conv2d_ (dilation / groups other than 1 raise ValueError)"""
    if dilation not in (1, (1, 1)) or groups != 1:
        raise ValueError("conv2d: dilation and groups are not supported")
    return conv2d_(as_tensor(obj), as_tensor(w), None if b is None else as_tensor(b), stride, padding)


def max_pool2d(obj, kernel, stride=None, padding=0):
    """not in the reference: see max_pool2d_"""
    return max_pool2d_(as_tensor(obj), kernel, stride=stride, padding=padding)


def attention(obj, k, v, causal=False, scale=None, layout="bhtd", lens=None, **unknown):
    """not in the reference: see attention_ (masks, dropout and bf16 are out of scope: unknown keyword arguments raise)"""
    if unknown:
        raise TypeError("attention: unsupported arguments %s (masks, dropout and bf16 are out of scope)" % sorted(unknown))
    return attention_(as_tensor(obj), as_tensor(k), as_tensor(v), causal=causal, scale=scale, layout=layout, lens=lens)


def _opt_tensor(obj):
    return None if obj is None else as_tensor(obj)


def layer_norm(obj, gamma=None, beta=None, eps=1e-5, **unknown):
    """not in the reference: see layer_norm_ (unknown keyword arguments raise)"""
    if unknown:
        raise TypeError("layer_norm: unsupported arguments %s" % sorted(unknown))
    return layer_norm_(as_tensor(obj), _opt_tensor(gamma), _opt_tensor(beta), eps=eps)


def rms_norm(obj, gamma=None, eps=1e-5, **unknown):
    """not in the reference: see rms_norm_ (unknown keyword arguments raise)"""
    if unknown:
        raise TypeError("rms_norm: unsupported arguments %s (RMS norm takes no beta)" % sorted(unknown))
    return rms_norm_(as_tensor(obj), _opt_tensor(gamma), eps=eps)


def gelu(obj, approximate="none", **unknown):
    """not in the reference: see gelu_ (unknown keyword arguments raise)"""
    if unknown:
        raise TypeError("gelu: unsupported arguments %s" % sorted(unknown))
    return gelu_(as_tensor(obj), approximate=approximate)


def gated(obj, up=None, act="silu", packed=False, **unknown):
    """not in the reference: see gated_ (SwiGLU / GEGLU; unknown keyword arguments raise)"""
    if unknown:
        raise TypeError("gated: unsupported arguments %s (bf16 and GEMM-epilogue fusion are out of scope)" % sorted(unknown))
    return gated_(as_tensor(obj), _opt_tensor(up), act=act, packed=packed)


def silu(obj, **unknown):
    """not in the reference: see silu_ (unknown keyword arguments raise)"""
    if unknown:
        raise TypeError("silu: unsupported arguments %s" % sorted(unknown))
    return silu_(as_tensor(obj))


def dropout(obj, p=0.5, residual=None, generator=None, **unknown):
    """not in the reference: see dropout_ (unknown keyword arguments raise)"""
    if unknown:
        raise TypeError("dropout: unsupported arguments %s" % sorted(unknown))
    return dropout_(as_tensor(obj), p, _opt_tensor(residual), generator=generator)


def embedding(obj, ids, pos=None, padding_idx=None, **unknown):
    """not in the reference: see embedding_ (unknown keyword arguments raise)"""
    if unknown:
        raise TypeError("embedding: unsupported arguments %s" % sorted(unknown))
    return embedding_(as_tensor(obj), ids, _opt_tensor(pos), padding_idx=padding_idx)


def cross_entropy(obj, targets, ignore_index=None, reduction="mean", **unknown):
    """not in the reference: see cross_entropy_ (unknown keyword arguments raise)"""
    if unknown:
        raise TypeError("cross_entropy: unsupported arguments %s" % sorted(unknown))
    return cross_entropy_(as_tensor(obj), targets, ignore_index=ignore_index, reduction=reduction)


def attention_gqa(obj, k, v, causal=False, scale=None, lens=None, **unknown):
    """not in the reference: see attention_gqa_ (grouped-query heads, layout "bthd"; unknown keyword arguments raise)"""
    if unknown:
        raise TypeError("attention_gqa: unsupported arguments %s (masks, dropout and bf16 are out of scope)" % sorted(unknown))
    return attention_gqa_(as_tensor(obj), as_tensor(k), as_tensor(v), causal=causal, scale=scale, lens=lens)


def rope(obj, k=None, rotary=None, offset=0, positions=None, layout="bthd", inverse=False, **unknown):
    """not in the reference: see rope_ (rotary position embedding of one tensor or of a q / k pair; unknown keyword arguments
    raise)"""
    if unknown:
        raise TypeError("rope: unsupported arguments %s (frequency scaling and bf16 are out of scope)" % sorted(unknown))
    return rope_(as_tensor(obj), _opt_tensor(k), rotary=rotary, offset=offset, positions=positions, layout=layout,
                 inverse=inverse)


def attention_decode_gqa(obj, k_cache, v_cache, length=None, k_new=None, v_new=None, lens=None, scale=None, layout="bthd",
                         **unknown):
    """not in the reference: see attention_decode_gqa_ (length=) and attention_decode_ragged_gqa_ (lens=); inference only;
    unknown keyword arguments raise"""
    if unknown:
        raise TypeError("attention_decode_gqa: unsupported arguments %s" % sorted(unknown))
    if (length is None) == (lens is None):
        raise ValueError("attention_decode_gqa: give length= (a host integer shared by the batch) or lens= (one per sequence)")
    if lens is not None:
        return attention_decode_ragged_gqa_(as_tensor(obj), k_cache, v_cache, lens, as_tensor(k_new), as_tensor(v_new),
                                            scale=scale, layout=layout)
    return attention_decode_gqa_(as_tensor(obj), k_cache, v_cache, length, _opt_tensor(k_new), _opt_tensor(v_new), scale=scale,
                                 layout=layout)


def attention_decode(obj, k_cache, v_cache, length, k_new=None, v_new=None, scale=None, layout="bthd", **unknown):
    """not in the reference: see attention_decode_ (inference only; unknown keyword arguments raise)"""
    if unknown:
        raise TypeError("attention_decode: unsupported arguments %s" % sorted(unknown))
    return attention_decode_(as_tensor(obj), k_cache, v_cache, length, _opt_tensor(k_new), _opt_tensor(v_new), scale=scale,
                             layout=layout)


def sample_rows(obj, u=None, temperature=1.0, top_k=None, **unknown):
    """not in the reference: see sample_rows_ (inference only; unknown keyword arguments raise)"""
    if unknown:
        raise TypeError("sample_rows: unsupported arguments %s (top-p is out of scope)" % sorted(unknown))
    return sample_rows_(as_tensor(obj), u, temperature=temperature, top_k=top_k)
