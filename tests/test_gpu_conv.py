"""csrc/tnn_conv.hip on the MI355X against the float64 oracle (tests/conv_oracle.py) under the DERIVED bound

    |y - y64| <= (K + 2) u (|x| (*) |w| + |b|),   u = 2**-24 (float32) or 2 * 2**-53 (float64),

K the contraction length of the product (C KH KW forward, F KH KW for dx, N OH OW for dw and db): the forward-error bound of
a length-K dot product in any summation order plus one rounding for the bias.  Pooling is exact (bit for bit) except for the
backward of overlapping windows, which adds at most ceil(k / s) ** 2 terms.

The one tolerance that is measured instead of derived is the LeNet trajectory: the native route must stay within
TRAJECTORY_FACTOR x the deviation of the COMPOSED route (existing kernels only) from the float64 fixture, measured in the
same test run and recorded in profiles/conv_lenet_trajectory.txt."""

import ctypes

import numpy as np
import pytest

import conv_oracle as co
import lenet_helpers as lh
import tinynn_autograd_amd as tn
from tinynn_autograd_amd import _lib, conv as cv
from tinynn_autograd_amd import device_array as da
from tinynn_autograd_amd.core import ops
from tinynn_autograd_amd.core.tensor import Tensor

pytestmark = pytest.mark.gpu

TRAJECTORY_FACTOR = 4.0        # profiles/conv_lenet_trajectory.txt: both routes are float32 evaluations of the same sums
FORMS = (cv.FORM_AUTO, cv.FORM_TILE, cv.FORM_SMALL)


@pytest.fixture(scope="module")
def golden():
    return lh.load_golden()


@pytest.fixture(autouse=True)
def _switches():
    yield
    da.CONV_ROUTE, da.CONV_FORM, da.CONV_SPLITS = None, 0, None


def dev(a, dtype, unaligned=False):
    """The array on the device in `dtype`; unaligned: at an address that is only element-aligned."""
    a = np.ascontiguousarray(a, dtype=dtype)
    if not unaligned:
        return tn.asarray(a, dtype=dtype)
    buf = tn.empty((a.size + 1,), dtype)
    view = buf[1:].reshape(a.shape)
    view[...] = tn.asarray(a, dtype=dtype)
    return view


def check_conv(x, w, b, dy, stride, padding, dtype, form, what, unaligned=False, splits=None, want=None):
    da.CONV_ROUTE, da.CONV_FORM, da.CONV_SPLITS = "native", form, splits
    xd, wd, bd, dyd = (dev(a, dtype, unaligned) for a in (x, w, b, dy))
    y = da.conv2d(xd, wd, bd, stride, padding)
    dx = da.conv2d_bwd_data(dyd, wd, x.shape, stride, padding)
    dw, db = da.conv2d_bwd_filter(xd, dyd, w.shape, stride, padding)
    want = want or (co.conv2d(x, w, b, stride, padding), co.conv2d_dx(dy, w, x.shape, stride, padding),
                    co.conv2d_dw(x, dy, w.shape, stride, padding), co.conv2d_db(dy))
    co.assert_within(y, want[0], co.fwd_bound(x, w, b, stride, padding, dtype), what + " y")
    co.assert_within(dx, want[1], co.dx_bound(dy, w, x.shape, stride, padding, dtype), what + " dx")
    co.assert_within(dw, want[2], co.dw_bound(x, dy, w.shape, stride, padding, dtype), what + " dw")
    co.assert_within(db, want[3], co.db_bound(dy, dtype), what + " db")


def test_backend_and_entry_points():
    lib = _lib.get()
    assert tn.backend_name() == "hip-gfx950"
    assert lib.has_conv
    assert cv.plan_conv2d((1, 1, 4, 4), (1, 1, 3, 3), native=lib.has_conv).route == "native"


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_fixture_cases(golden, dtype):
    for name, (xs, ws, stride, padding) in co.CONV_CASES.items():
        x, w, b, dy = co.conv_case_input(name)
        want = tuple(golden["%s.%s" % (name, k)] for k in ("y", "dx", "dw", "db"))
        for form in (FORMS if dtype == np.float32 else (cv.FORM_AUTO,)):
            check_conv(x, w, b, dy, stride, padding, dtype, form, "%s form %d" % (name, form), want=want)


def fuzz_shapes(rs, count):
    """Geometries whose GEMM views straddle the tile edges of both geometries (16 / 64 rows, 64 / 256 columns, 16-deep K)."""
    edge_ch = [1, 2, 3, 15, 16, 17, 31, 33, 63, 64, 65]
    for _ in range(count):
        c, f = (int(rs.choice(edge_ch)) for _ in range(2))
        if c * f > 1100:
            c = int(rs.choice(edge_ch[:5]))
        kh, kw = int(rs.randint(1, 5)), int(rs.randint(1, 5))
        sh, sw = int(rs.randint(1, 4)), int(rs.randint(1, 4))
        ph, pw = int(rs.randint(0, 4)), int(rs.randint(0, 4))
        h = int(rs.randint(max(1, kh - 2 * ph), 14))
        w = int(rs.randint(max(1, kw - 2 * pw), 14))
        n = int(rs.choice([1, 2, 3, 5]))
        yield (n, c, h, w), (f, c, kh, kw), (sh, sw), (ph, pw)


def test_fuzz_raw_calls_float32():
    """A few hundred raw calls per entry point: every geometry forced, unaligned base pointers, split contractions."""
    rs = np.random.RandomState(20240)
    calls = 0
    for i, (xs, ws, stride, padding) in enumerate(fuzz_shapes(rs, 90)):
        oh, ow = co.out_extent(xs[2], ws[2], stride[0], padding[0]), co.out_extent(xs[3], ws[3], stride[1], padding[1])
        x = rs.randn(*xs).astype(np.float32) * 3
        w = rs.randn(*ws).astype(np.float32)
        b = rs.randn(ws[0]).astype(np.float32) * 4
        dy = rs.randn(xs[0], ws[0], oh, ow).astype(np.float32)
        want = (co.conv2d(x, w, b, stride, padding), co.conv2d_dx(dy, w, xs, stride, padding),
                co.conv2d_dw(x, dy, ws, stride, padding), co.conv2d_db(dy))
        for form in FORMS:
            splits = [None, 1, 3][(i + form) % 3]
            check_conv(x, w, b, dy, stride, padding, np.float32, form, "fuzz %d %s %s s%s p%s form %d splits %s" % (
                i, xs, ws, stride, padding, form, splits), unaligned=bool((i + form) & 1), splits=splits, want=want)
            calls += 1
    assert calls >= 200


def test_fuzz_raw_calls_float64():
    rs = np.random.RandomState(20241)
    for i, (xs, ws, stride, padding) in enumerate(fuzz_shapes(rs, 40)):
        oh, ow = co.out_extent(xs[2], ws[2], stride[0], padding[0]), co.out_extent(xs[3], ws[3], stride[1], padding[1])
        x, w, b = rs.randn(*xs) * 3, rs.randn(*ws), rs.randn(ws[0]) * 4
        dy = rs.randn(xs[0], ws[0], oh, ow)
        check_conv(x, w, b, dy, stride, padding, np.float64, 0, "fuzz64 %d %s %s" % (i, xs, ws), unaligned=bool(i & 1))


def test_large_contraction_split_and_unsplit_agree_within_the_bound():
    """The LeNet first layer at batch 64: N OH OW = 50176, cut into the planner's ranges (> 1) and uncut."""
    rs = np.random.RandomState(5)
    x = (rs.rand(64, 1, 28, 28) * (rs.rand(64, 1, 28, 28) < 0.19)).astype(np.float32)
    w = rs.randn(6, 1, 5, 5).astype(np.float32)
    b = rs.randn(6).astype(np.float32)
    dy = rs.randn(64, 6, 28, 28).astype(np.float32)
    plan = cv.plan_conv2d(x.shape, w.shape, stride=1, padding=2)
    assert cv.filter_splits(plan, True) > 1
    for splits in (None, 1):
        check_conv(x, w, b, dy, 1, 2, np.float32, 0, "lenet conv1 batch 64 splits %s" % splits, splits=splits)


def test_relu_epilogue_keeps_the_mask_in_the_sign_bit():
    x, w, b, _ = co.conv_case_input("lenet_conv2")
    da.CONV_ROUTE = "native"
    for form in FORMS:
        da.CONV_FORM = form
        plain = np.asarray(da.conv2d(dev(x, np.float32), dev(w, np.float32), dev(b, np.float32), 1, 0))
        fused = da.conv2d(dev(x, np.float32), dev(w, np.float32), dev(b, np.float32), 1, 0, relu=True)
        assert fused._tag is da.RELU_SIGN
        got = np.asarray(fused)
        np.testing.assert_array_equal(got, np.maximum(plain, 0.0))
        np.testing.assert_array_equal(np.signbit(got), plain < 0)


def test_native_against_composed_route():
    """The second, independent implementation: the tap loop on the generic kernels, same inputs, both under the bound."""
    for name in ("non_square_everything", "stride3_pad2", "lenet_conv2"):
        xs, ws, stride, padding = co.CONV_CASES[name]
        x, w, b, dy = co.conv_case_input(name)
        res = {}
        for route in ("native", "composed"):
            da.CONV_ROUTE = route
            xd, wd, bd, dyd = (dev(a, np.float32) for a in (x, w, b, dy))
            dw, db = da.conv2d_bwd_filter(xd, dyd, ws, stride, padding)
            res[route] = [np.asarray(v, dtype=np.float64) for v in (
                da.conv2d(xd, wd, bd, stride, padding), da.conv2d_bwd_data(dyd, wd, xs, stride, padding), dw, db)]
        bounds = (co.fwd_bound(x, w, b, stride, padding, np.float32), co.dx_bound(dy, w, xs, stride, padding, np.float32),
                  co.dw_bound(x, dy, ws, stride, padding, np.float32), co.db_bound(dy, np.float32))
        for a, c, bound, what in zip(res["native"], res["composed"], bounds, ("y", "dx", "dw", "db")):
            assert a.shape == c.shape
            assert (np.abs(a - c) <= 2 * bound).all(), "%s %s: the routes differ by more than both bounds" % (name, what)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_pooling_is_exact(golden, dtype):
    da.CONV_ROUTE = "native"
    for name, (xs, kernel, stride, padding) in co.POOL_CASES.items():
        x, dy = co.pool_case_input(name)
        y, idx = da.max_pool2d(dev(x, dtype, unaligned=True), kernel, stride, padding)
        assert idx.dtype == np.int32
        np.testing.assert_array_equal(np.asarray(y), golden[name + ".y"], err_msg=name)
        np.testing.assert_array_equal(np.asarray(idx), golden[name + ".idx"], err_msg=name)
        dx = da.max_pool2d_bwd(dev(dy, dtype), idx, xs, kernel, stride, padding)
        bound = co.pool_dx_bound(dy, golden[name + ".idx"], xs, kernel, stride, dtype)
        if not bound.any():
            np.testing.assert_array_equal(np.asarray(dx), golden[name + ".dx"].astype(dtype), err_msg=name)
        else:
            co.assert_within(dx, golden[name + ".dx"], bound, name + " dx")
        da.CONV_ROUTE = "composed"
        yc, ic = da.max_pool2d(dev(x, dtype), kernel, stride, padding)
        np.testing.assert_array_equal(np.asarray(yc), np.asarray(y), err_msg=name)
        np.testing.assert_array_equal(np.asarray(ic).astype(np.int32), np.asarray(idx), err_msg=name)
        da.CONV_ROUTE = "native"


def test_pooling_all_equal_windows_and_nan():
    da.CONV_ROUTE = "native"
    x = np.full((1, 2, 6, 6), 2.5, dtype=np.float32)
    y, idx = da.max_pool2d(dev(x, np.float32), 3, 2, 1)
    _, want = co.max_pool2d(x, 3, 2, 1)
    np.testing.assert_array_equal(np.asarray(idx), want)
    dx = np.asarray(da.max_pool2d_bwd(tn.ones(y.shape), idx, x.shape, 3, 2, 1))
    np.testing.assert_array_equal(dx, co.max_pool2d_dx(np.ones(y.shape), want, x.shape))
    x[0, 0, 3, 3] = np.nan
    y, _ = da.max_pool2d(dev(x, np.float32), 2)
    got = np.asarray(y)
    assert np.isnan(got[0, 0, 1, 1]) and np.isnan(got).sum() == 1


def test_dx_is_not_computed_for_an_input_without_gradient(monkeypatch):
    lib = _lib.get()
    calls = {"data": 0, "filter": 0}
    real_data, real_filter = lib.conv2d_bwd_data, lib.conv2d_bwd_filter
    monkeypatch.setattr(lib, "conv2d_bwd_data", lambda *a: (calls.__setitem__("data", calls["data"] + 1), real_data(*a))[1])
    monkeypatch.setattr(lib, "conv2d_bwd_filter", lambda *a: (calls.__setitem__("filter", calls["filter"] + 1), real_filter(*a))[1])
    x, w, b, dy = co.conv_case_input("one_filter")
    wt, bt = Tensor(w, requires_grad=True), Tensor(b, requires_grad=True)
    wt.zero_grad(), bt.zero_grad()
    ops.conv2d(Tensor(x), wt, bt, 1, 1).backward(dy)
    assert calls == {"data": 0, "filter": 1}                     # dw and db from ONE launch, no dx
    xt = Tensor(x, requires_grad=True)
    xt.zero_grad()
    ops.conv2d(xt, wt, bt, 1, 1).backward(dy)
    assert calls == {"data": 1, "filter": 2}
    co.assert_within(xt.grad, co.conv2d_dx(dy, w, x.shape, 1, 1), co.dx_bound(dy, w, x.shape, 1, 1, np.float32), "dx")
    co.assert_within(wt.grad, 2 * co.conv2d_dw(x, dy, w.shape, 1, 1), 2 * co.dw_bound(x, dy, w.shape, 1, 1, np.float32),
                     "dw accumulated twice")


def test_filter_gradient_is_bit_identical_run_to_run():
    rs = np.random.RandomState(9)
    x = rs.randn(32, 6, 14, 14).astype(np.float32)
    dy = rs.randn(32, 16, 10, 10).astype(np.float32)
    da.CONV_ROUTE = "native"
    plan = cv.plan_conv2d(x.shape, (16, 6, 5, 5))
    assert cv.filter_splits(plan, True) > 1
    xd, dyd = dev(x, np.float32), dev(dy, np.float32)
    first = [np.asarray(a) for a in da.conv2d_bwd_filter(xd, dyd, (16, 6, 5, 5))]
    second = [np.asarray(a) for a in da.conv2d_bwd_filter(xd, dyd, (16, 6, 5, 5))]
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])


def test_captured_lenet_step_equals_the_eager_step():
    x, y = co.lenet_batches(steps=1)[0]
    eager, eager_loss = lh.build_lenet_model()
    for _ in range(3):
        loss_e = lh.train_step(eager, eager_loss, x, y)
    model, loss_layer = lh.build_lenet_model()
    xs, ys = Tensor(x), Tensor(y)
    step = tn.capture(lambda: lh.train_step(model, loss_layer, xs, ys), warmup=2)
    loss_c = step()
    tn.synchronize()
    assert np.array_equal(np.asarray(loss_c.values), np.asarray(loss_e.values))
    for a, b in zip(eager.net.parameter_tensors(), model.net.parameter_tensors()):
        assert np.array_equal(np.asarray(a.values), np.asarray(b.values))


def test_lenet_trajectory(golden):
    """Five Adam steps against the float64 replica: the native route within TRAJECTORY_FACTOR x the composed route's own
    deviation (measured here, on existing kernels only; recorded in profiles/conv_lenet_trajectory.txt)."""
    dev_of = {}
    for route in ("composed", "native"):
        da.CONV_ROUTE = route
        model, loss_layer = lh.build_lenet_model()
        losses, params = lh.run_trajectory(model, loss_layer)
        dev_of[route] = lh.trajectory_deviation(losses, params, golden)
        print("lenet trajectory %s: loss deviation %.3e (relative), parameter deviation %.3e (absolute)" % ((route,) + dev_of[route]))
    assert dev_of["native"][0] <= TRAJECTORY_FACTOR * dev_of["composed"][0]
    assert dev_of["native"][1] <= TRAJECTORY_FACTOR * dev_of["composed"][1]
