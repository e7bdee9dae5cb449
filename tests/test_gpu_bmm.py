"""tnn_gemm_batched (csrc/tnn_bmm.hip) on the MI355X: the fixture recorded from the reference bit for bit through the BATCHED
route in float32 and float64, a seeded fuzz against float64 numpy under the textbook dot-product bound, gradients through
Tensor.backward, graph capture, empty / K = 0 and swapaxes.

Bound (float32): |C - C64| <= (K + 1) u (|A| @ |B|) elementwise, u = 2**-24 — the forward error of a length-K dot product
summed in any order, with or without FMA (gamma_K = K u to first order; the inputs are exact float32 values, so there is
no input term).  float64: 2 (K + 1) 2**-53, since numpy's own result errs as well.
"""

import ctypes

import numpy as np
import pytest

import gen_bmm_golden as G

import tinynn_autograd_amd as tn
from tinynn_autograd_amd import _lib
from tinynn_autograd_amd import batching
from tinynn_autograd_amd import device_array as da
from tinynn_autograd_amd._bmm_signatures import FORM_AUTO, FORM_SMALL, FORM_TILE
from tinynn_autograd_amd.core.tensor import Tensor

pytestmark = pytest.mark.gpu

U32, U64 = 2.0 ** -24, 2.0 ** -53


@pytest.fixture(autouse=True)
def _restore_switches():
    old = da.BMM_ROUTE, da.BMM_FORM
    yield
    da.BMM_ROUTE, da.BMM_FORM = old


def bound(a, b, K, dtype):
    u = U32 if np.dtype(dtype) == np.float32 else 2 * U64
    return (K + 1) * u * np.matmul(np.abs(a.astype(np.float64)), np.abs(b.astype(np.float64)))


def check(got, a, b, dtype, what):
    want = np.matmul(a.astype(np.float64), b.astype(np.float64))
    got = np.asarray(got)
    assert got.shape == want.shape and got.dtype == dtype, what
    K = a.shape[-1]
    err = np.abs(got.astype(np.float64) - want)
    lim = bound(a, b, K, dtype)
    assert np.all(err <= lim), "%s: worst excess %g at bound %g" % (what, float((err - lim).max()), float(lim.max()))


def raw_batched(ta, tb, M, N, K, a_dev, lda, b_dev, ldb, batch, a_bs, b_bs, dtype, form):
    """tnn_gemm_batched itself, on device arrays: returns C [batch..., M, N]"""
    out = tn.empty(tuple(batch) + (M, N), dtype=dtype)
    arr = lambda v: (ctypes.c_int64 * max(len(v), 1))(*v)                   # noqa: E731
    _lib.get().gemm_batched(ta, tb, M, N, K, a_dev._ptr, lda, b_dev._ptr, ldb, out._ptr, len(batch),
                            arr(batch), arr(a_bs), arr(b_bs), da._CODE[np.dtype(dtype)], form)
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("form", [FORM_AUTO, FORM_TILE, FORM_SMALL])
def test_fixture_bit_exact_through_the_batched_route(dtype, form):
    tn.set_default_float(dtype)
    da.BMM_ROUTE, da.BMM_FORM = "batched", form
    stored = G.load()
    lib = _lib.get()
    assert lib.has_bmm and tn.backend_name() == "hip-gfx950"
    for name in G.CASES:
        a, b, _ = G.case_input(name)
        got = np.asarray(tn.asarray(a.astype(dtype)) @ tn.asarray(b.astype(dtype)))
        assert got.dtype == dtype, name
        np.testing.assert_array_equal(got, stored[name + "/fwd"].astype(dtype), err_msg=name)


def test_fixture_takes_the_expected_routes():
    """Without forcing: the batched kernel for stacks, one GEMM for the Dense form."""
    for name, want in (("stack", "batched"), ("broadcast_5d", "batched"), ("thousand_4x4", "batched"),
                       ("dense_form", "gemm2d"), ("stack_by_matrix", "gemm2d"), ("plain_2d", "gemm2d")):
        sa, sb = G.CASES[name]
        assert batching.plan_matmul(sa, sb, native=_lib.get().has_bmm).route == want, name


def _fuzz_case(rs, i):
    """One raw call: shapes covering both geometries and their edges, all four transpose combinations, row strides wider
    than the rows, broadcast and multi-dimensional batches, unaligned bases."""
    sizes = [1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 70, 96, 127, 128, 129, 200]
    M, N = int(rs.choice(sizes)), int(rs.choice(sizes))
    K = int(rs.choice([1, 2, 3, 4, 5, 8, 15, 16, 17, 31, 32, 33, 64, 100, 257]))
    ta, tb = i & 1, (i >> 1) & 1
    nbd = int(rs.randint(0, 4))
    batch = [int(rs.choice([1, 2, 3, 5])) for _ in range(nbd)]
    if i % 7 == 0:
        batch = [int(rs.choice([40, 130]))]
    pad_a, pad_b = int(rs.choice([0, 0, 1, 4])), int(rs.choice([0, 0, 3, 4]))
    a_rows, a_cols = (K, M) if ta else (M, K)
    b_rows, b_cols = (N, K) if tb else (K, N)
    lda, ldb = a_cols + pad_a, b_cols + pad_b
    a_bc = [bool(rs.rand() < 0.25) for _ in batch]                       # broadcast along this dimension
    b_bc = [bool(rs.rand() < 0.25) for _ in batch]
    a_store = [1 if bc else n for n, bc in zip(batch, a_bc)]
    b_store = [1 if bc else n for n, bc in zip(batch, b_bc)]
    off_a, off_b = int(rs.choice([0, 0, 1, 4])), int(rs.choice([0, 0, 2, 4]))
    return dict(M=M, N=N, K=K, ta=ta, tb=tb, batch=batch, lda=lda, ldb=ldb, a_store=a_store, b_store=b_store,
                a_bc=a_bc, b_bc=b_bc, a_rows=a_rows, a_cols=a_cols, b_rows=b_rows, b_cols=b_cols, off_a=off_a, off_b=off_b)


def _run_fuzz(dtype, n_cases, seed):
    rs = np.random.RandomState(seed)
    forms_seen = set()
    for i in range(n_cases):
        c = _fuzz_case(rs, i)
        form = (FORM_AUTO, FORM_TILE, FORM_SMALL)[i % 3]
        a_buf = rs.standard_normal(c["off_a"] + int(np.prod(c["a_store"] + [c["a_rows"], c["lda"]]))).astype(dtype)
        b_buf = rs.standard_normal(c["off_b"] + int(np.prod(c["b_store"] + [c["b_rows"], c["ldb"]]))).astype(dtype)
        a_host = a_buf[c["off_a"]:].reshape(c["a_store"] + [c["a_rows"], c["lda"]])[..., :c["a_cols"]]
        b_host = b_buf[c["off_b"]:].reshape(c["b_store"] + [c["b_rows"], c["ldb"]])[..., :c["b_cols"]]
        a_log = np.swapaxes(a_host, -1, -2) if c["ta"] else a_host
        b_log = np.swapaxes(b_host, -1, -2) if c["tb"] else b_host
        a_log = np.broadcast_to(a_log, tuple(c["batch"]) + a_log.shape[-2:])
        b_log = np.broadcast_to(b_log, tuple(c["batch"]) + b_log.shape[-2:])
        dense = lambda store, rows, ld: list(batching.dense_strides(store + [rows, ld])[:-2])     # noqa: E731
        a_bs = [0 if bc else s for bc, s in zip(c["a_bc"], dense(c["a_store"], c["a_rows"], c["lda"]))]
        b_bs = [0 if bc else s for bc, s in zip(c["b_bc"], dense(c["b_store"], c["b_rows"], c["ldb"]))]
        # (dtype given: asarray would otherwise store float64 host data as the default float32, half the bytes the raw call reads)
        a_dev, b_dev = tn.asarray(a_buf, dtype=dtype), tn.asarray(b_buf, dtype=dtype)
        assert a_dev.dtype == dtype and a_dev.size == a_buf.size and b_dev.dtype == dtype and b_dev.size == b_buf.size
        got = raw_batched(c["ta"], c["tb"], c["M"], c["N"], c["K"], a_dev[c["off_a"]:], c["lda"], b_dev[c["off_b"]:],
                          c["ldb"], c["batch"], a_bs, b_bs, dtype, form)
        check(got, a_log, b_log, dtype, "case %d %r form %d" % (i, c, form))
        forms_seen.add((form, c["M"] <= 32 and c["N"] <= 32))
    return forms_seen


def test_fuzz_float32():
    seen = _run_fuzz(np.float32, 240, 31)
    assert {(FORM_TILE, True), (FORM_TILE, False), (FORM_SMALL, True), (FORM_SMALL, False)} <= seen


def test_fuzz_float64():
    tn.set_default_float(np.float64)
    _run_fuzz(np.float64, 60, 32)


def test_fuzz_through_the_array_interface():
    """a @ b on device arrays: N-d views, lazy transposes and swapped batch axes, whatever route the planner takes."""
    rs = np.random.RandomState(33)
    for i in range(40):
        nb = int(rs.randint(1, 4))
        batch = [int(rs.choice([1, 2, 3, 6])) for _ in range(nb)]
        M, K, N = (int(rs.choice([1, 3, 16, 20, 33, 64, 70])) for _ in range(3))
        a = rs.standard_normal(batch + [M, K]).astype(np.float32)
        b_batch = [1 if rs.rand() < 0.3 else n for n in batch][int(rs.randint(0, nb + 1)):]
        b = rs.standard_normal(b_batch + [K, N]).astype(np.float32)
        da_, db_ = tn.asarray(a), tn.asarray(b)
        if i % 4 == 1:
            a, da_ = a[1:], da_[1:]
            b, db_ = (b[1:], db_[1:]) if b.ndim == a.ndim and b.shape[0] == a.shape[0] + 1 else (b, db_)
        if i % 4 == 2 and b.ndim == 2:
            bt = np.ascontiguousarray(b.T)
            db_ = tn.asarray(bt).T
        if i % 4 == 3:
            a, da_ = np.swapaxes(a, -1, -2), da_.swapaxes(-1, -2)
            b2 = rs.standard_normal(b.shape[:-2] + (M, N)).astype(np.float32)
            b, db_ = b2, tn.asarray(b2)
        check(da_ @ db_, a, b, np.float32, "case %d %s @ %s" % (i, a.shape, b.shape))


def _grad_check(a, b, g, route=None):
    da.BMM_ROUTE = route
    ta, tb = Tensor(a, requires_grad=True), Tensor(b, requires_grad=True)
    out = ta @ tb
    out.backward(tn.asarray(g))
    ga, gb = G.closed_form_grads(a, b, g)
    a64, b64, g64 = (np.asarray(v, dtype=np.float64) for v in (a, b, g))
    a2 = a64[None, :] if a64.ndim == 1 else a64
    b2 = b64[:, None] if b64.ndim == 1 else b64
    batch = np.broadcast_shapes(a2.shape[:-2], b2.shape[:-2])
    g2 = np.abs(g64.reshape(batch + (a2.shape[-2], b2.shape[-1])))
    # the bound of the vjp products, summed over everything that un-broadcasting adds up: the number of terms per output
    # element is the contraction length times the broadcast multiplicity
    lim_a = np.einsum("...mn,...kn->...mk", g2, np.broadcast_to(np.abs(b2), batch + b2.shape[-2:]))
    lim_b = np.einsum("...mk,...mn->...kn", np.broadcast_to(np.abs(a2), batch + a2.shape[-2:]), g2)

    def fold(x, shape):
        x = x.sum(axis=tuple(range(x.ndim - len(shape)))) if x.ndim > len(shape) else x
        for i, d in enumerate(shape):
            if d == 1 and x.shape[i] != 1:
                x = x.sum(axis=i, keepdims=True)
        return x

    terms_a = b2.shape[-1] * int(np.prod(batch)) // max(int(np.prod(a2.shape[:-2])), 1)
    terms_b = a2.shape[-2] * int(np.prod(batch)) // max(int(np.prod(b2.shape[:-2])), 1)
    lim_a = (terms_a + 1) * U32 * fold(lim_a, a2.shape).reshape(a64.shape)
    lim_b = (terms_b + 1) * U32 * fold(lim_b, b2.shape).reshape(b64.shape)
    got_a, got_b = np.asarray(ta.grad, dtype=np.float64), np.asarray(tb.grad, dtype=np.float64)
    assert got_a.shape == a.shape and got_b.shape == b.shape
    assert np.all(np.abs(got_a - ga) <= lim_a), float(np.abs(got_a - ga).max())
    assert np.all(np.abs(got_b - gb) <= lim_b), float(np.abs(got_b - gb).max())
    return out


@pytest.mark.parametrize("shapes", [((2, 1, 33, 20), (1, 3, 20, 17)), ((5, 16, 8), (5, 8, 16)), ((3, 70), (4, 70, 9)),
                                    ((6,), (4, 6, 5)), ((4, 7, 6), (6,)), ((4, 65, 40), (1, 40, 66))])
def test_gradients_batched(shapes):
    rs = np.random.RandomState(sum(shapes[0]) + 7 * sum(shapes[1]))
    a = rs.standard_normal(shapes[0]).astype(np.float32)
    b = rs.standard_normal(shapes[1]).astype(np.float32)
    g = rs.standard_normal(np.matmul(a, b).shape).astype(np.float32)
    _grad_check(a, b, g, route="batched")
    _grad_check(a, b, g, route=None)


def test_gradients_dense_form_is_the_single_gemm_collapse():
    rs = np.random.RandomState(9)
    a = rs.standard_normal((3, 200, 70)).astype(np.float32)
    b = rs.standard_normal((70, 30)).astype(np.float32)
    g = rs.standard_normal((3, 200, 30)).astype(np.float32)
    lib = _lib.get()
    calls = []
    saved = {name: getattr(lib, name) for name in ("gemm", "gemm_batched")}
    for name in saved:
        setattr(lib, name, (lambda n: lambda *args: (calls.append((n,) + tuple(args[:5])), saved[n](*args))[1])(name))
    try:
        _grad_check(a, b, g)
    finally:
        for name, fn in saved.items():
            setattr(lib, name, fn)
    assert calls == [("gemm", 0, 0, 600, 30, 70), ("gemm", 0, 1, 600, 70, 30), ("gemm", 1, 0, 70, 30, 600)]


def test_capture_and_replay():
    """A batched product inside tn.capture, replayed three times on changing inputs (same buffers, new contents)."""
    rs = np.random.RandomState(12)
    a = tn.asarray(rs.standard_normal((6, 20, 12)).astype(np.float32))
    b = tn.asarray(rs.standard_normal((1, 12, 33)).astype(np.float32))
    da.BMM_ROUTE = "batched"
    replay = tn.capture(lambda: a @ b, warmup=1)
    for step in range(3):
        an = rs.standard_normal((6, 20, 12)).astype(np.float32)
        bn = rs.standard_normal((1, 12, 33)).astype(np.float32)
        a[...] = tn.asarray(an)
        b[...] = tn.asarray(bn)
        out = replay()
        check(out, an, bn, np.float32, "replay %d" % step)


def test_empty_batch_and_k0():
    da.BMM_ROUTE = "batched"
    z = tn.asarray(np.zeros((0, 3, 4), dtype=np.float32)) @ tn.asarray(np.zeros((0, 4, 2), dtype=np.float32))
    assert z.shape == (0, 3, 2)
    a, b = tn.asarray(np.ones((3, 5, 4), dtype=np.float32)), tn.asarray(np.ones((3, 4, 7), dtype=np.float32))
    for form in (FORM_TILE, FORM_SMALL):
        out = da.full((3, 5, 7), 9.0, dtype=np.float32)
        arr = lambda v: (ctypes.c_int64 * len(v))(*v)                       # noqa: E731
        _lib.get().gemm_batched(0, 0, 5, 7, 0, a._ptr, 4, b._ptr, 7, out._ptr, 1, arr([3]), arr([20]), arr([28]), 0, form)
        np.testing.assert_array_equal(np.asarray(out), np.zeros((3, 5, 7), dtype=np.float32))     # K = 0 writes zeros
    out = da.full((3, 5, 7), 9.0, dtype=np.float64)
    a64, b64 = tn.asarray(np.ones((3, 5, 4)), dtype=np.float64), tn.asarray(np.ones((3, 4, 7)), dtype=np.float64)
    arr = lambda v: (ctypes.c_int64 * len(v))(*v)                           # noqa: E731
    _lib.get().gemm_batched(0, 0, 5, 7, 0, a64._ptr, 4, b64._ptr, 7, out._ptr, 1, arr([3]), arr([20]), arr([28]), 1, 0)
    np.testing.assert_array_equal(np.asarray(out), np.zeros((3, 5, 7)))
    z = tn.asarray(np.ones((2, 3, 0), dtype=np.float32)) @ tn.asarray(np.ones((2, 0, 5), dtype=np.float32))
    np.testing.assert_array_equal(np.asarray(z), np.zeros((2, 3, 5), dtype=np.float32))
    with pytest.raises(_lib.TnnError, match="batch dimensions"):
        _lib.get().gemm_batched(0, 0, 5, 7, 4, a._ptr, 4, b._ptr, 7, out._ptr, 5, arr([1] * 5), arr([0] * 5),
                                arr([0] * 5), 0, 0)


def test_swapaxes():
    rs = np.random.RandomState(3)
    x = rs.standard_normal((3, 4, 5)).astype(np.float32)
    d = tn.asarray(x)
    for a1, a2 in ((0, 1), (1, 2), (0, 2), (-1, -2), (1, 1)):
        np.testing.assert_array_equal(np.asarray(d.swapaxes(a1, a2)), np.swapaxes(x, a1, a2))
        np.testing.assert_array_equal(np.asarray(np.swapaxes(d, a1, a2)), np.swapaxes(x, a1, a2))
    q, k = rs.standard_normal((2, 4, 10, 8)).astype(np.float32), rs.standard_normal((2, 4, 10, 8)).astype(np.float32)
    check(tn.asarray(q) @ tn.asarray(k).swapaxes(-1, -2), q, np.swapaxes(k, -1, -2), np.float32, "q @ k^T")
