"""N-d `a @ b` through the Python layers — planner, dispatcher, vjps, un-broadcast — on the `gemm2d` and `loop` routes (the
only ones the CPU test twin has; forced here so the same calls are made where the product library is loaded).  Forward
values against the fixture recorded from the reference, gradients against the float64 closed form (the reference's N-d
backward raises, tests/gen_bmm_golden.py); both exact on the fixture's integer data."""

import contextlib

import numpy as np
import pytest

import gen_bmm_golden as G
import op_cases
from helpers import load_op_cases

import tinynn_autograd_amd as tn
from tinynn_autograd_amd import _lib
from tinynn_autograd_amd import device_array as da
from tinynn_autograd_amd.core import ops
from tinynn_autograd_amd.core.tensor import Tensor


@pytest.fixture(autouse=True)
def _loop_route():
    old = da.BMM_ROUTE
    da.BMM_ROUTE = "loop"
    yield
    da.BMM_ROUTE = old


@contextlib.contextmanager
def recorded_calls():
    """Every tnn_gemm / tnn_gemm_batched call of the block: [(name, transA, transB, M, N, K)]"""
    lib = _lib.get()
    calls = []
    saved = {name: getattr(lib, name) for name in ("gemm", "gemm_batched")}

    def spy(name):
        def call(*args):
            calls.append((name,) + tuple(args[:5]))
            return saved[name](*args)
        return call

    for name in saved:
        setattr(lib, name, spy(name))
    try:
        yield calls
    finally:
        for name, fn in saved.items():
            setattr(lib, name, fn)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", list(G.CASES))
def test_fixture_forward_and_gradients(name, dtype):
    tn.set_default_float(dtype)
    stored = G.load()
    a, b, g = G.case_input(name)
    ta, tb = Tensor(a.astype(dtype), requires_grad=True), Tensor(b.astype(dtype), requires_grad=True)
    with recorded_calls() as calls:
        out = ops.dot_(ta, tb)
    assert not any(c[0] == "gemm_batched" for c in calls)
    got = np.asarray(out.values)
    assert got.dtype == dtype and got.shape == stored[name + "/fwd"].shape
    np.testing.assert_array_equal(got, stored[name + "/fwd"].astype(dtype))      # bit for bit: integers
    out.backward(tn.asarray(g.astype(dtype)))
    ga, gb = G.closed_form_grads(a, b, g)
    assert np.asarray(ta.grad).shape == a.shape and np.asarray(tb.grad).shape == b.shape
    np.testing.assert_array_equal(np.asarray(ta.grad, dtype=np.float64), ga)
    np.testing.assert_array_equal(np.asarray(tb.grad, dtype=np.float64), gb)


def test_backward_accumulates_repeats_and_prunes():
    a, b, g = G.case_input("broadcast_4d")
    ta, tb = Tensor(a, requires_grad=True), Tensor(b, requires_grad=False)
    out = ta @ tb
    with recorded_calls() as calls:
        out.backward(tn.asarray(g))
        out.backward(tn.asarray(g))
    ga, _ = G.closed_form_grads(a, b, g)
    np.testing.assert_array_equal(np.asarray(ta.grad, dtype=np.float64), 2 * ga)      # accumulates until zero_grad
    assert tb.grad is None or not np.asarray(tb.grad).any()                          # no edge to an input without grad
    per_backward = len(calls) // 2
    assert per_backward == 8                          # one product per batch element for dA, none for dB
    ta.zero_grad()
    out.backward(tn.asarray(g))
    np.testing.assert_array_equal(np.asarray(ta.grad, dtype=np.float64), ga)


def test_dense_form_is_single_gemms():
    """X[..., M, K] @ W[K, N]: forward one (rows, K) @ (K, N), dX one NT product over all rows, dW ONE long-K TN product."""
    a, b, g = G.case_input("dense_form")
    ta, tb = Tensor(a, requires_grad=True), Tensor(b, requires_grad=True)
    with recorded_calls() as calls:
        out = ta @ tb
        out.backward(tn.asarray(g))
    assert calls == [("gemm", 0, 0, 600, 30, 70), ("gemm", 0, 1, 600, 70, 30), ("gemm", 1, 0, 70, 30, 600)]
    assert np.asarray(out.values).shape == (3, 200, 30)


def test_2d_dot_is_todays_calls():
    """The 2-D `dot` case of tests/golden/op_cases.json: the same three GEMMs as ever, the same values and gradients (its
    operands are integer lists, which the float cast makes dense before the product); on float operands the vjps are the NT
    and TN kernels through the lazy `.T`, no transpose is materialised."""
    want = load_op_cases()["dot"]
    with recorded_calls() as calls:
        got = op_cases.case_dot(Tensor, ops)
    assert [(c[0],) + c[3:] for c in calls] == [("gemm", 2, 4, 3), ("gemm", 2, 3, 4), ("gemm", 3, 4, 2)]
    for k in want:
        np.testing.assert_array_equal(np.asarray(got[k], dtype=np.float64), want[k])
    a, b, g = G.case_input("plain_2d")
    ta, tb = Tensor(a, requires_grad=True), Tensor(b, requires_grad=True)
    with recorded_calls() as calls:
        (ta @ tb).backward(tn.asarray(g))
    assert calls == [("gemm", 0, 0, 7, 3, 5), ("gemm", 0, 1, 7, 5, 3), ("gemm", 1, 0, 5, 3, 7)]


def test_strided_views_and_lazy_transposes():
    rs = np.random.RandomState(5)
    a = rs.randint(-3, 4, size=(6, 4, 5)).astype(np.float32)
    b = rs.randint(-3, 4, size=(3, 5)).astype(np.float32)
    da_, db_ = tn.asarray(a), tn.asarray(b)
    np.testing.assert_array_equal(np.asarray(da_[1:4] @ db_.T), a[1:4] @ b.T)               # leading-axis view, lazy .T
    np.testing.assert_array_equal(np.asarray(db_ @ da_.swapaxes(1, 2)), b @ a.swapaxes(1, 2))
    np.testing.assert_array_equal(np.asarray(np.matmul(da_.transpose(1, 0, 2), db_.T)), a.transpose(1, 0, 2) @ b.T)
    np.testing.assert_array_equal(np.asarray(np.swapaxes(da_, 0, 2)), np.swapaxes(a, 0, 2))
    np.testing.assert_array_equal(np.asarray(db_.swapaxes(0, 1) @ db_), b.T @ b)
    np.testing.assert_array_equal(np.asarray(da_.swapaxes(-1, -1)), a)
    with pytest.raises(np.exceptions.AxisError):
        da_.swapaxes(0, 3)


def test_empty_and_k0():
    z = tn.asarray(np.zeros((0, 3, 4), dtype=np.float32)) @ tn.asarray(np.zeros((0, 4, 2), dtype=np.float32))
    assert z.shape == (0, 3, 2)
    z = tn.asarray(np.ones((2, 3, 0), dtype=np.float32)) @ tn.asarray(np.ones((2, 0, 5), dtype=np.float32))
    np.testing.assert_array_equal(np.asarray(z), np.zeros((2, 3, 5), dtype=np.float32))
    z = tn.asarray(np.ones((2, 3, 4), dtype=np.float32)) @ tn.asarray(np.ones((4, 0), dtype=np.float32))
    assert z.shape == (2, 3, 0)


def test_refusals():
    a = tn.asarray(np.ones((2, 3, 4), dtype=np.float32))
    with pytest.raises(ValueError, match="core dimension 0"):
        a @ tn.asarray(np.ones((2, 5, 4), dtype=np.float32))
    with pytest.raises(ValueError, match="broadcast"):
        a @ tn.asarray(np.ones((3, 4, 4), dtype=np.float32))
    with pytest.raises(TypeError, match="not matmul"):             # numpy's N-d dot is another contraction
        np.dot(a, tn.asarray(np.ones((2, 4, 3), dtype=np.float32)))
    with pytest.raises(TypeError, match="not matmul"):
        a.dot(tn.asarray(np.ones((4, 3), dtype=np.float32)))
    m = tn.asarray(np.arange(6.0).reshape(2, 3))
    np.testing.assert_array_equal(np.asarray(np.dot(m, m.T)), np.arange(6.0).reshape(2, 3) @ np.arange(6.0).reshape(2, 3).T)
