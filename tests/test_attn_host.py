"""Attention above the kernels — device_array routes, graph node, wrapper, MultiHeadAttention, Model — on the backend of the
session (the CPU test twin runs the composed route): forward and all three gradients against the float64 oracle inside the
derived bounds, both dtypes and layouts, causal and not, q without a gradient, the hand-written chain of existing ops, empty
results, rejected arguments, parameter order, lazy fan-in and one Adam step against the float64 replica."""

import numpy as np
import pytest

import attn_oracle as ao
import tinynn_autograd_amd as tn
from tinynn_autograd_amd import _lib, device_array as da
from tinynn_autograd_amd.core import ops
from tinynn_autograd_amd.core.layers import Dense, MultiHeadAttention, MHA_PARAM_ORDER, PARAM_ORDER
from tinynn_autograd_amd.core.losses import SquaredErrorLoss
from tinynn_autograd_amd.core.model import Model
from tinynn_autograd_amd.core.nn import Net
from tinynn_autograd_amd.core.optimizer import Adam
from tinynn_autograd_amd.core.tensor import Tensor


def leaf(a):
    t = Tensor(a, requires_grad=True)
    t.zero_grad()
    return t


def test_the_session_route():
    lib = _lib.get()
    plan = da._attn_plan(tn.ones((1, 2, 3)), tn.ones((1, 4, 3)), tn.ones((1, 4, 5)), False, None, "bhtd", None)
    assert plan.route == ("native" if lib.has_attn else "composed")
    if tn.backend_name() != "hip-gfx950":
        assert plan.route == "composed"
    assert da.ATTN_ROUTE is None


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("layout", ["bhtd", "bthd"])
@pytest.mark.parametrize("causal", [False, True])
def test_node_forward_and_gradients(dtype, layout, causal):
    tn.set_default_float(dtype)
    rs = np.random.RandomState(11 + causal)
    q, k, v, do = ao.make_inputs(rs, layout, 2, 3, 9, 12, 5, 7, dtype)
    res = ao.reference(q, k, v, do, causal, None, layout, dtype)
    qt, kt, vt = leaf(q), leaf(k), leaf(v)
    out = ops.attention(qt, kt, vt, causal=causal, layout=layout)
    assert out.values.dtype == dtype and out.shape == do.shape and out.requires_grad
    out.backward(do)
    for t in (qt, kt, vt):
        assert t.grad.shape == t.shape and t.grad.dtype == dtype
    ao.check(dict(o=out.values, dq=qt.grad, dk=kt.grad, dv=vt.grad), res, "%s causal %d" % (layout, causal))
    out.backward(do)                                       # repeatable, and Tensor.backward accumulates
    for t, name in ((qt, "dq"), (kt, "dk"), (vt, "dv")):
        ao.assert_within(t.grad, 2 * res.values[name], 2 * res.bounds[name] + ao.unit(dtype) * np.abs(2 * res.values[name]),
                         name + " twice")


def arena_leaves(q, k, v):
    """q, k, v as leaves whose gradients have pinned views of ONE flat arena as their home (what a Model's optimizer
    gives its parameters): (tensors, arena)."""
    arena = tn.zeros((q.size + k.size + v.size,))
    leaves, off = [], 0
    for a in (q, k, v):
        t = Tensor(a, requires_grad=True)
        t._grad_home = arena[off:off + a.size].reshape(a.shape)
        t.zero_grad()
        leaves.append(t)
        off += a.size
    return leaves, arena


@pytest.mark.parametrize("layout", ["bhtd", "bthd"])
def test_gradients_land_in_arena_views(layout):
    """First contribution of lazily-zero, arena-backed leaves: the gradient IS the arena view (the fused vjp is offered the
    views; a route that cannot write them in place has its result copied there); a second backward accumulates on top."""
    rs = np.random.RandomState(31)
    q, k, v, do = ao.make_inputs(rs, layout, 2, 2, 9, 11, 4, 6)
    res = ao.reference(q, k, v, do, True, None, layout)
    (qt, kt, vt), arena = arena_leaves(q, k, v)
    out = ops.attention(qt, kt, vt, causal=True, layout=layout)
    out.backward(do)
    flat = np.asarray(arena)
    off = 0
    for t, name in ((qt, "dq"), (kt, "dk"), (vt, "dv")):
        assert t.grad is t._grad_home
        ao.assert_within(t.grad, res.values[name], res.bounds[name], name)
        np.testing.assert_array_equal(flat[off:off + t.grad.size].reshape(t.shape), np.asarray(t.grad))
        off += t.grad.size
    out.backward(do)
    for t, name in ((qt, "dq"), (kt, "dk"), (vt, "dv")):
        assert t.grad is t._grad_home
        ao.assert_within(t.grad, 2 * res.values[name], 2 * res.bounds[name] + ao.U32 * np.abs(2 * res.values[name]), name + " twice")


def test_q_without_a_gradient_and_per_edge_vjps():
    rs = np.random.RandomState(4)
    q, k, v, do = ao.make_inputs(rs, "bhtd", 1, 2, 6, 8, 4, 3)
    res = ao.reference(q, k, v, do, True, 0.4, "bhtd")
    kt, vt = leaf(k), leaf(v)
    out = ops.attention(Tensor(q), kt, vt, causal=True, scale=0.4)
    assert [d["tensor"] for d in out.dependency] == [kt, vt]
    out.backward(do)
    ao.check(dict(o=out.values, dk=kt.grad, dv=vt.grad), res, "q frozen")
    assert not ops.attention(Tensor(q), Tensor(k), Tensor(v)).requires_grad
    # one tensor on two edges: the scheduler asks edge by edge, the contributions add up
    x = (rs.randn(1, 5, 4) * 2).astype(np.float32)
    xt = leaf(x)
    g = rs.randn(1, 5, 4).astype(np.float32)
    ops.attention(xt, xt, xt).backward(g)
    self_res = ao.reference(x, x, x, g)
    want = sum(self_res.values[n] for n in ("dq", "dk", "dv"))
    bound = sum(self_res.bounds[n] for n in ("dq", "dk", "dv")) + 2 * ao.U32 * sum(np.abs(self_res.values[n]) for n in ("dq", "dk", "dv"))
    ao.assert_within(xt.grad, want, bound, "self-attention on one tensor")


def test_composed_route_equals_the_hand_written_chain():
    rs = np.random.RandomState(6)
    q, k, v, do = ao.make_inputs(rs, "bhtd", 2, 2, 10, 13, 8, 6)
    qt, kt, vt = leaf(q), leaf(k), leaf(v)
    out = ops.attention_(qt, kt, vt, route="composed")
    out.backward(do)
    q2, k2, v2 = leaf(q), leaf(k), leaf(v)
    s = (q2 @ ops.transpose_(k2, (0, 1, 3, 2))) * (1.0 / np.sqrt(8))
    # (the row maximum enters as a constant: a shift of a row's scores does not change the softmax, and the reference's
    # max_ vjp only handles the axes its own tests use)
    e = ops.exp(s - ops.reshape(ops.max(Tensor(s.values), axis=-1), (2, 2, 10, 1)))
    chain = (e / ops.reshape(ops.sum(e, axis=-1), (2, 2, 10, 1))) @ v2
    chain.backward(do)
    # forward: the same operations in the same order, up to how k's transpose reaches the product (a flag there, a copy
    # here) — at most a reordered dot product, 2 ulp of the largest element allowed
    scale = np.abs(np.asarray(chain.values)).max()
    np.testing.assert_allclose(np.asarray(out.values), np.asarray(chain.values), rtol=0, atol=2 * 2.0 ** -23 * scale)
    # backward: two formulations of the same sums.  The route rebuilds p = exp(s - lse), the chain keeps e / l: per term two
    # exp evaluations (X ulp each, attn_oracle.EXP_ULP), a log, a subtraction, a division and a product differ, (2 X + 4) u,
    # and the sums over the keys / queries may be ordered differently, max(Tq, Tk) u — first order, scaled by the largest
    # element of the gradient: (2 X + 4 + 13) u = 21 u, about 10 ulp
    tol = (2 * ao.EXP_ULP + 4 + 13) * ao.U32
    for a, b in ((qt, q2), (kt, k2), (vt, v2)):
        gmax = np.abs(np.asarray(b.grad)).max()
        np.testing.assert_allclose(np.asarray(a.grad), np.asarray(b.grad), rtol=0, atol=tol * gmax)


def test_dtype_promotion_and_empty_results():
    rs = np.random.RandomState(2)
    q, k, v, _ = ao.make_inputs(rs, "bhtd", 1, 1, 3, 4, 2, 2)
    mixed = da.attention(tn.asarray(q), tn.asarray(k, dtype=np.float64), tn.asarray(v))      # promoted as matmul promotes
    assert mixed[0].dtype == np.float64 and mixed[1].dtype == np.float64
    assert ops.attention(q, k, v).values.dtype == np.float32
    ints = ops.attention(np.ones((2, 3), dtype=np.int64), np.ones((4, 3), dtype=np.int64), np.arange(8).reshape(4, 2))
    assert ints.values.dtype == np.float32
    np.testing.assert_allclose(np.asarray(ints.values), np.broadcast_to([3.0, 4.0], (2, 2)), rtol=1e-6)
    for shapes in (((2, 0, 3), (2, 4, 3), (2, 4, 5)), ((0, 2, 3), (0, 4, 3), (0, 4, 5))):
        qt, kt, vt = (leaf(np.zeros(s, dtype=np.float32)) for s in shapes)
        out = ops.attention(qt, kt, vt)
        assert out.shape == shapes[0][:-1] + (5,)
        out.backward(np.zeros(out.shape, dtype=np.float32))
        assert kt.grad.shape == shapes[1] and not np.asarray(kt.grad).any()


def test_rejected_arguments():
    q, k, v = (Tensor(np.ones(s, dtype=np.float32)) for s in ((2, 3), (4, 3), (4, 2)))
    for kwargs in (dict(mask=np.ones((2, 4))), dict(dropout=0.1), dict(dtype="bf16")):
        with pytest.raises(TypeError, match="out of scope"):
            ops.attention(q, k, v, **kwargs)
        with pytest.raises(TypeError, match="out of scope"):
            ops.attention_(q, k, v, **kwargs)
    with pytest.raises(ValueError, match="no keys"):
        ops.attention(q, Tensor(np.ones((0, 3), dtype=np.float32)), Tensor(np.ones((0, 2), dtype=np.float32)))
    with pytest.raises(ValueError, match="head dimension"):
        ops.attention(q, Tensor(np.ones((4, 5), dtype=np.float32)), v)
    with pytest.raises(ValueError, match="layout"):
        ops.attention(q, k, v, layout="thd")
    with pytest.raises(ValueError, match="route must be"):
        ops.attention_(q, k, v, route="quick")


def test_layer_parameters_order_and_lazy_fan_in():
    assert PARAM_ORDER == ("w", "b")
    assert MHA_PARAM_ORDER == ("wq", "bq", "wk", "bk", "wv", "bv", "wo", "bo")
    np.random.seed(3)
    lazy = MultiHeadAttention(2)
    assert not lazy.is_init and list(lazy.params) == list(MHA_PARAM_ORDER) and all(p is None for p in lazy.params.values())
    np.random.seed(3)
    eager = MultiHeadAttention(2, num_in=8)
    assert eager.is_init and list(eager.params) == list(MHA_PARAM_ORDER)
    x = Tensor(np.random.RandomState(0).randn(2, 5, 8).astype(np.float32))
    np.random.seed(3)
    out = lazy.forward(x)
    assert lazy.is_init and out.shape == (2, 5, 8)
    for name in MHA_PARAM_ORDER:
        assert tuple(lazy.params[name].shape) == ((8, 8) if name[0] == "w" else (1, 8))
        np.testing.assert_array_equal(np.asarray(lazy.params[name].values), np.asarray(eager.params[name].values))
    net = Net([Dense(8, num_in=8), lazy])
    assert net.parameter_tensors()[2:] == [lazy.params[n] for n in MHA_PARAM_ORDER]
    with pytest.raises(ValueError, match="multiple of num_heads"):
        MultiHeadAttention(3, num_in=8)
    with pytest.raises(ValueError, match="multiple of num_heads"):
        MultiHeadAttention(3).forward(x)
    with pytest.raises(ValueError, match=r"\[B, T, E\]"):
        eager.forward(Tensor(np.ones((5, 8), dtype=np.float32)))


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("causal", [False, True])
def test_model_step_against_the_float64_replica(fused, causal):
    rs = np.random.RandomState(21)
    x, y = rs.randn(2, 5, 8).astype(np.float32), rs.randn(2, 5, 8).astype(np.float32)
    np.random.seed(5)
    layer = MultiHeadAttention(2, causal=causal, fused=fused)
    model = Model(net=Net([layer]), loss=SquaredErrorLoss(), optimizer=Adam(lr=1e-2))
    loss_layer = SquaredErrorLoss()
    model.zero_grad()
    loss = loss_layer.loss(model.forward(Tensor(x)), Tensor(y))
    ref = ao.MHA64([np.asarray(p.values) for p in model.net.parameter_tensors()], 2, causal=causal, lr=1e-2)
    loss.backward()
    model.step()
    after = float(loss_layer.loss(model.forward(Tensor(x)), Tensor(y)).values)
    loss64, _ = ref.step(x, y)
    after64 = ref.loss_and_grads(x, y)[0]
    assert after64 < loss64
    np.testing.assert_allclose(float(loss.values), loss64, rtol=1e-5)
    np.testing.assert_allclose(after, after64, rtol=1e-5)
    for name, p, p64 in zip(MHA_PARAM_ORDER, model.net.parameter_tensors(), ref.p):
        if name == "bk":
            continue      # its gradient is mathematically zero (a shift of a row's scores): Adam normalises rounding noise,
                          # and the output does not depend on it
        np.testing.assert_allclose(np.asarray(p.values), p64, rtol=0, atol=1e-5)
