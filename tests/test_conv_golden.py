"""tests/golden/conv_cases.npz through the package (on the CPU test twin: the composed route; on the GPU: whatever route
conv.py picks): forward and all three gradients of every recorded case under the derived bound of tests/conv_oracle.py,
pooling bit for bit; and the fixture agrees with the oracle that recorded it."""

import numpy as np
import pytest

import conv_oracle as co
import lenet_helpers as lh
import tinynn_autograd_amd as tn
from tinynn_autograd_amd import device_array as da


@pytest.fixture(scope="module")
def golden():
    return lh.load_golden()


def test_fixture_is_what_the_oracle_computes(golden):
    assert {k.split(".")[0] for k in golden} == set(co.CONV_CASES) | set(co.POOL_CASES) | {"lenet"}
    for name, (xs, ws, stride, padding) in co.CONV_CASES.items():
        x, w, b, dy = co.conv_case_input(name)
        np.testing.assert_array_equal(golden[name + ".y"], co.conv2d(x, w, b, stride, padding))
        np.testing.assert_array_equal(golden[name + ".dw"], co.conv2d_dw(x, dy, ws, stride, padding))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", sorted(co.CONV_CASES))
def test_convolution_cases(golden, name, dtype):
    tn.set_default_float(dtype)
    xs, ws, stride, padding = co.CONV_CASES[name]
    x, w, b, dy = co.conv_case_input(name)
    xd, wd, bd, dyd = (tn.asarray(a, dtype=dtype) for a in (x, w, b, dy))
    co.assert_within(da.conv2d(xd, wd, bd, stride, padding), golden[name + ".y"],
                     co.fwd_bound(x, w, b, stride, padding, dtype), name + " y")
    co.assert_within(da.conv2d_bwd_data(dyd, wd, xs, stride, padding), golden[name + ".dx"],
                     co.dx_bound(dy, w, xs, stride, padding, dtype), name + " dx")
    dw, db = da.conv2d_bwd_filter(xd, dyd, ws, stride, padding)
    co.assert_within(dw, golden[name + ".dw"], co.dw_bound(x, dy, ws, stride, padding, dtype), name + " dw")
    co.assert_within(db, golden[name + ".db"], co.db_bound(dy, dtype), name + " db")


@pytest.mark.parametrize("name", sorted(co.POOL_CASES))
def test_pooling_cases(golden, name):
    xs, kernel, stride, padding = co.POOL_CASES[name]
    x, dy = co.pool_case_input(name)
    y, idx = da.max_pool2d(tn.asarray(x), kernel, stride, padding)
    np.testing.assert_array_equal(np.asarray(y), golden[name + ".y"])
    np.testing.assert_array_equal(np.asarray(idx).astype(np.int32), golden[name + ".idx"])
    dx = da.max_pool2d_bwd(tn.asarray(dy), idx, xs, kernel, stride, padding)
    bound = co.pool_dx_bound(dy, golden[name + ".idx"], xs, kernel, stride, np.float32)
    if not bound.any():
        np.testing.assert_array_equal(np.asarray(dx), golden[name + ".dx"].astype(np.float32))
    else:
        co.assert_within(dx, golden[name + ".dx"], bound, name + " dx")
