"""The attention planner (tinynn-autograd_amd/attention.py): extents, strides of both layouts, output shape, route choice,
every ValueError, and the causal rule through the routes of the session's backend."""

import math

import numpy as np
import pytest

import attn_oracle as ao
from tinynn_autograd_amd import attention as at


def test_bhtd_folds_the_leading_dimensions():
    p = at.plan_attention((2, 3, 5, 7, 4), (2, 3, 5, 9, 4), (2, 3, 5, 9, 6))
    assert p.geometry() == (30, 1, 7, 9, 4, 6)
    assert p.out_shape == (2, 3, 5, 7, 6) and p.lse_shape == (2, 3, 5, 7)
    assert p.q_strides == (28, 28, 4) and p.k_strides == (36, 36, 4) and p.v_strides == (54, 54, 6) and p.o_strides == (42, 42, 6)
    assert p.strides("q", "o") == [28, 28, 4, 42, 42, 6]
    assert p.scale == 1.0 / math.sqrt(4) and p.causal is False and p.route == "native"
    p = at.plan_attention((7, 4), (9, 4), (9, 6), causal=True, scale=0.3)
    assert p.geometry() == (1, 1, 7, 9, 4, 6) and p.out_shape == (7, 6) and p.lse_shape == (7,)
    assert p.scale == 0.3 and p.causal is True


def test_bthd_strides_address_the_projection_in_place():
    b, tq, tk, h, d, dv = 2, 5, 7, 3, 4, 6
    p = at.plan_attention((b, tq, h, d), (b, tk, h, d), (b, tk, h, dv), layout="bthd")
    assert p.geometry() == (b, h, tq, tk, d, dv)
    assert p.out_shape == (b, tq, h, dv) and p.lse_shape == (b, h, tq)
    for strides, t, w in ((p.q_strides, tq, d), (p.k_strides, tk, d), (p.v_strides, tk, dv), (p.o_strides, tq, dv)):
        flat = np.arange(b * t * h * w).reshape(b, t, h, w)
        sb, sh, sr = strides
        for bi, hi, ti in ((0, 0, 0), (1, 2, t - 1), (1, 1, 2)):
            assert flat[bi, ti, hi, 0] == bi * sb + hi * sh + ti * sr
    p = at.plan_attention((b, h, tq, d), (b, h, tk, d), (b, h, tk, dv), layout="bhtd")
    flat = np.arange(b * h * tq * d).reshape(b * h, tq, d)
    assert flat[4, 3, 0] == 4 * p.q_strides[0] + 3 * p.q_strides[2]


def test_route_choice():
    sh = lambda d, dv: ((2, 4, d), (2, 6, d), (2, 6, dv))
    assert at.plan_attention(*sh(128, 128)).route == "native"
    assert at.plan_attention(*sh(129, 8)).route == "composed"
    assert at.plan_attention(*sh(8, 129)).route == "composed"
    assert at.plan_attention(*sh(8, 8), native=False).route == "composed"
    assert at.plan_attention(*sh(8, 8), float_ok=False).route == "composed"
    assert at.plan_attention(*sh(8, 8), route="composed").route == "composed"
    assert at.plan_attention(*sh(8, 8), route="native").route == "native"
    for kwargs in (dict(native=False), dict(float_ok=False)):
        with pytest.raises(ValueError, match="native attention route"):
            at.plan_attention(*sh(8, 8), route="native", **kwargs)
    with pytest.raises(ValueError, match="native attention route"):
        at.plan_attention(*sh(129, 8), route="native")
    with pytest.raises(ValueError, match="route must be"):
        at.plan_attention(*sh(8, 8), route="fast")
    assert at.MAX_HEAD_DIM == 128


def test_empty_results_are_plans_not_errors():
    p = at.plan_attention((2, 0, 4), (2, 5, 4), (2, 5, 3))
    assert p.empty() and p.out_shape == (2, 0, 3)
    p = at.plan_attention((0, 3, 4), (0, 5, 4), (0, 5, 3))
    assert p.empty() and p.out_shape == (0, 3, 3)
    assert not at.plan_attention((1, 1, 1), (1, 1, 1), (1, 1, 1)).empty()


@pytest.mark.parametrize("shapes, kwargs, match", [
    (((2, 4, 3), (2, 0, 3), (2, 0, 5)), {}, "no keys"),
    (((2, 4, 0), (2, 5, 0), (2, 5, 5)), {}, "empty head dimension"),
    (((2, 4, 3), (2, 5, 3), (2, 5, 0)), {}, "empty value dimension"),
    (((2, 4, 3), (2, 5, 4), (2, 5, 5)), {}, "head dimension 3, k has 4"),
    (((2, 4, 3), (2, 5, 3), (2, 6, 5)), {}, "5 keys, v holds 6"),
    (((2, 4, 3), (3, 5, 3), (3, 5, 5)), {}, "leading dimensions"),
    (((2, 4, 3), (1, 5, 3), (1, 5, 5)), {}, "no broadcasting"),
    (((2, 4, 3), (5, 3), (5, 5)), {}, "leading dimensions"),
    (((3,), (5, 3), (5, 5)), {}, r"\[\.\.\., T, D\]"),
    (((2, 4, 3), (2, 5, 3), (2, 5, 5)), dict(layout="bthd"), r"\[B, T, H, D\]"),
    (((2, 4, 2, 3), (2, 5, 3, 3), (2, 5, 3, 5)), dict(layout="bthd"), "batch and head extents"),
    (((2, 4, 2, 3), (3, 5, 2, 3), (3, 5, 2, 5)), dict(layout="bthd"), "batch and head extents"),
    (((2, 4, 3), (2, 5, 3), (2, 5, 5)), dict(layout="tbhd"), "layout must be"),
    (((2, 4, 3), (2, 5, 3), (2, 5, 5)), dict(scale=float("inf")), "scale must be finite"),
])
def test_every_value_error(shapes, kwargs, match):
    with pytest.raises(ValueError, match=match):
        at.plan_attention(*shapes, **kwargs)


@pytest.mark.parametrize("tq, tk", [(3, 3), (5, 2), (2, 5), (1, 4)])
def test_causal_rule_is_top_left_aligned(tq, tk):
    """Through the code that applies it: the composed route's mask array, and the attention of both backends' routes whose
    probabilities (read off with v = identity) must vanish exactly above the diagonal and nowhere else."""
    import tinynn_autograd_amd as tn
    from tinynn_autograd_amd import device_array as da
    keep = ao.keep_mask(tq, tk, True)
    assert keep[:, 0].all()                                   # every row keeps key 0: no row is empty
    for i in range(tq):
        for j in range(tk):
            assert keep[i, j] == (j <= i)
    mask = np.asarray(da._attn_mask(tq, tk, np.dtype(np.float32)))
    np.testing.assert_array_equal(mask == 0, keep)
    np.testing.assert_array_equal(np.isneginf(mask), ~keep)
    rs = np.random.RandomState(tq * 10 + tk)
    q, k = rs.randn(1, tq, 4).astype(np.float32), rs.randn(1, tk, 4).astype(np.float32)
    eye = np.eye(tk, dtype=np.float32)[None]
    for route in (None, "composed"):
        p, _ = da.attention(tn.asarray(q), tn.asarray(k), tn.asarray(eye), causal=True, route=route)
        np.testing.assert_array_equal(np.asarray(p)[0] > 0, keep)
        p, _ = da.attention(tn.asarray(q), tn.asarray(k), tn.asarray(eye), causal=False, route=route)
        assert (np.asarray(p) > 0).all()
