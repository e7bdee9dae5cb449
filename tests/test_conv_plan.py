"""conv.py, the host planner of convolution and pooling (no device): output extents against the closed form and the
oracle's shapes, every ValueError, the route choice with and without the native entry points, the kernel geometry."""

import numpy as np
import pytest

import conv_oracle as co
from tinynn_autograd_amd import conv as cv


def test_output_extents_over_a_grid():
    for h in range(1, 12):
        for k in range(1, 6):
            for s in range(1, 4):
                for p in range(0, 4):
                    if h + 2 * p < k:
                        with pytest.raises(ValueError, match="smaller than the kernel"):
                            cv.out_extent(h, k, s, p)
                        continue
                    want = (h + 2 * p - k) // s + 1
                    assert cv.out_extent(h, k, s, p) == want
                    plan = cv.plan_conv2d((2, 3, h, h + 1), (4, 3, k, 1), stride=(s, 1), padding=(p, 0))
                    y = co.conv2d(np.zeros((2, 3, h, h + 1)), np.zeros((4, 3, k, 1)), None, (s, 1), (p, 0))
                    assert plan.out_shape == y.shape == (2, 4, want, h + 1)
                    if p <= k // 2:
                        pool = cv.plan_pool2d((2, 3, h, h + 1), (k, 1), (s, 1), (p, 0))
                        assert pool.out_shape == co.max_pool2d(np.zeros((2, 3, h, h + 1)), (k, 1), (s, 1), (p, 0))[0].shape


def test_stride_and_padding_forms():
    plan = cv.plan_conv2d((1, 2, 9, 8), (3, 2, 3, 2), stride=[2, 1], padding=(1, 0))
    assert (plan.sh, plan.sw, plan.ph, plan.pw, plan.OH, plan.OW) == (2, 1, 1, 0, 5, 7)
    assert plan.geometry() == (1, 2, 9, 8, 3, 3, 2, 2, 1, 1, 0)
    assert cv.plan_pool2d((1, 1, 6, 6), 2).geometry() == (1, 6, 6, 2, 2, 2, 2, 0, 0)      # stride None = the window


@pytest.mark.parametrize("kwargs, match", [
    (dict(x_shape=(2, 3, 5), w_shape=(4, 3, 3, 3)), "N, C, H, W"),
    (dict(x_shape=(2, 3, 5, 5), w_shape=(4, 3, 3)), "F, C, KH, KW"),
    (dict(x_shape=(2, 3, 5, 5), w_shape=(4, 2, 3, 3)), "channels"),
    (dict(x_shape=(2, 3, 5, 5), w_shape=(4, 3, 3, 3), b_shape=(5,)), "bias"),
    (dict(x_shape=(2, 3, 5, 5), w_shape=(4, 3, 3, 3), stride=0), "stride"),
    (dict(x_shape=(2, 3, 5, 5), w_shape=(4, 3, 3, 3), stride=(1, 2, 3)), "pair"),
    (dict(x_shape=(2, 3, 5, 5), w_shape=(4, 3, 3, 3), stride=1.5), "integral"),
    (dict(x_shape=(2, 3, 5, 5), w_shape=(4, 3, 3, 3), padding=-1), "padding"),
    (dict(x_shape=(2, 3, 5, 5), w_shape=(4, 3, 3, 3), dilation=2), "dilation"),
    (dict(x_shape=(2, 3, 5, 5), w_shape=(4, 3, 3, 3), groups=3), "groups"),
    (dict(x_shape=(2, 3, 2, 5), w_shape=(4, 3, 3, 3)), "smaller than the kernel"),
    (dict(x_shape=(2, 3, 5, 0), w_shape=(4, 3, 3, 3), padding=2), "empty"),
    (dict(x_shape=(2, 3, 5, 5), w_shape=(4, 3, 3, 3), route="im2col"), "route"),
    (dict(x_shape=(2, 3, 5, 5), w_shape=(4, 3, 3, 3), route="native", native=False), "native"),
])
def test_conv_value_errors(kwargs, match):
    with pytest.raises(ValueError, match=match):
        cv.plan_conv2d(**kwargs)


@pytest.mark.parametrize("args, match", [
    (((2, 3, 5), 2), "N, C, H, W"),
    (((2, 3, 5, 5), 0), "kernel"),
    (((2, 3, 5, 5), 2, 0), "stride"),
    (((2, 3, 5, 5), 2, None, 2), "half the window"),
    (((2, 3, 5, 5), 3, None, (1, 2)), "half the window"),
    (((2, 3, 1, 5), 2), "smaller than the kernel"),
])
def test_pool_value_errors(args, match):
    with pytest.raises(ValueError, match=match):
        cv.plan_pool2d(*args)


def test_route_choice():
    shapes = ((2, 3, 5, 5), (4, 3, 3, 3))
    assert cv.plan_conv2d(*shapes, native=True).route == "native"
    assert cv.plan_conv2d(*shapes, native=False).route == "composed"
    assert cv.plan_conv2d(*shapes, native=True, float_ok=False).route == "composed"
    assert cv.plan_conv2d(*shapes, native=True, route="composed").route == "composed"
    assert cv.plan_pool2d(shapes[0], 2, native=True).route == "native"
    assert cv.plan_pool2d(shapes[0], 2, native=False).route == "composed"


def test_kernel_geometry_and_filter_workspace():
    assert cv.form_for(6) == cv.form_for(32) == cv.FORM_SMALL and cv.form_for(33) == cv.FORM_TILE
    assert cv.form_for(6, cv.FORM_TILE) == cv.FORM_TILE
    assert cv.tiles(6, 26) == 1 and cv.tiles(17, 257) == 4 and cv.tiles(65, 65) == 4 and cv.tiles(16, 151, cv.FORM_TILE) == 3
    lenet1 = cv.plan_conv2d((128, 1, 28, 28), (6, 1, 5, 5), padding=2)
    s = cv.filter_splits(lenet1, True)
    assert 1 < s <= cv.MAX_SPLITS and lenet1.N * lenet1.OH * lenet1.OW // s >= 4 * cv.K_TILE
    assert cv.filter_workspace_bytes(lenet1, True, 0, s) == 256 + s * cv.TILE_ELEMS * 4
    assert cv.filter_workspace_bytes(lenet1, True, 0, 1) == 0
    tiny = cv.plan_conv2d((1, 1, 4, 4), (2, 1, 3, 3))
    assert cv.filter_splits(tiny, True) == 1                      # a contraction of 4 has nothing to split
    assert [t[:2] for t in cv.taps(tiny)] == [(kh, kw) for kh in range(3) for kw in range(3)]      # row-major
