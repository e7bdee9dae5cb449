"""gqa.py, the host planner of grouped-query attention: the refusals, the strides, the split rule and the routes.  numpy only."""

import math

import pytest

from tinynn_autograd_amd import attention as at
from tinynn_autograd_amd import decoding as dc
from tinynn_autograd_amd import gqa


def test_training_plan_extents_strides_and_shapes():
    p = gqa.plan_gqa_attention((2, 7, 6, 5), (2, 9, 2, 5), (2, 9, 2, 3), causal=True)
    assert (p.B, p.H, p.Hkv, p.group, p.Tq, p.Tk, p.D, p.Dv) == (2, 6, 2, 3, 7, 9, 5, 3)
    assert p.geometry() == (2, 6, 2, 7, 9, 5, 3)
    assert p.q_strides == (7 * 6 * 5, 5, 6 * 5) and p.o_strides == (7 * 6 * 3, 3, 6 * 3)
    assert p.k_strides == (9 * 2 * 5, 5, 2 * 5) and p.v_strides == (9 * 2 * 3, 3, 2 * 3)      # the head stride steps over Hkv heads
    assert p.strides("q", "k", "v", "o") == list(p.q_strides + p.k_strides + p.v_strides + p.o_strides)
    assert p.out_shape == (2, 7, 6, 3) and p.lse_shape == (2, 6, 7) and p.k_shape == (2, 9, 2, 5)
    assert p.causal and p.scale == 1.0 / math.sqrt(5) and p.route == "native" and p.layout == "bthd"
    assert gqa.plan_gqa_attention((2, 7, 6, 5), (2, 9, 2, 5), (2, 9, 2, 3), native=False).route == "composed"
    assert gqa.plan_gqa_attention((2, 7, 6, 5), (2, 9, 2, 5), (2, 9, 2, 3), float_ok=False).route == "composed"


def test_group_one_is_the_multi_head_plan():
    p = gqa.plan_gqa_attention((2, 7, 3, 5), (2, 9, 3, 5), (2, 9, 3, 4), scale=0.3)
    q = at.plan_attention((2, 7, 3, 5), (2, 9, 3, 5), (2, 9, 3, 4), scale=0.3, layout="bthd")
    assert p.group == 1 and p.strides("q", "k", "v", "o") == q.strides("q", "k", "v", "o")
    assert (p.out_shape, p.lse_shape, p.scale) == (q.out_shape, q.lse_shape, q.scale)


@pytest.mark.parametrize("shapes, match", [
    (((2, 7, 6, 5), (2, 9, 4, 5), (2, 9, 4, 3)), "no multiple"),
    (((2, 7, 6, 5), (2, 9, 0, 5), (2, 9, 0, 3)), "key / value heads"),
    (((2, 7, 6, 5), (2, 9, 2, 5), (2, 9, 3, 3)), "k holds 2 heads, v holds 3"),
    (((2, 7, 6, 5), (2, 9, 2, 4), (2, 9, 2, 3)), "head dimension"),
    (((2, 7, 6, 5), (2, 9, 2, 5), (2, 8, 2, 3)), "keys"),
    (((2, 7, 6, 5), (3, 9, 2, 5), (3, 9, 2, 3)), "batch and head extents"),
    (((2, 7, 6, 5), (2, 0, 2, 5), (2, 0, 2, 3)), "no keys"),
    (((7, 6, 5), (9, 2, 5), (9, 2, 3)), r"q \[B, Tq, H, D\]"),
])
def test_training_plan_refusals(shapes, match):
    with pytest.raises(ValueError, match=match):
        gqa.plan_gqa_attention(*shapes)


def test_the_old_planner_still_refuses_differing_heads():
    with pytest.raises(ValueError, match="batch and head extents"):
        at.plan_attention((2, 7, 6, 5), (2, 9, 2, 5), (2, 9, 2, 3), layout="bthd")


def test_the_group_limit_routes():
    big = ((1, 4, 9, 5), (1, 4, 1, 5), (1, 4, 1, 5))
    assert gqa.plan_gqa_attention(*big).route == "composed" and gqa.plan_gqa_attention(*big).group == 9
    with pytest.raises(ValueError, match="a group <= 8"):
        gqa.plan_gqa_attention(*big, route="native")
    assert gqa.plan_gqa_attention((1, 4, 8, 5), (1, 4, 1, 5), (1, 4, 1, 5)).route == "native"
    with pytest.raises(ValueError, match="route must be one of"):
        gqa.plan_gqa_attention((1, 4, 8, 5), (1, 4, 1, 5), (1, 4, 1, 5), route="fwd")
    assert gqa.plan_gqa_attention((1, 4, 8, 200), (1, 4, 1, 200), (1, 4, 1, 5)).route == "composed"     # head dimension
    assert gqa.plan_gqa_decode((1, 9, 5), (1, 4, 1, 5), (1, 4, 1, 5), 2).route == "composed"
    with pytest.raises(ValueError, match="a group <= 8"):
        gqa.plan_gqa_decode((1, 9, 5), (1, 4, 1, 5), (1, 4, 1, 5), 2, route="native")


@pytest.mark.parametrize("layout", gqa.LAYOUTS)
def test_decode_plan_strides_and_split(layout):
    B, H, Hkv, Tmax, D, Dv = 2, 8, 2, 300, 16, 24
    kc, vc = dc.cache_shape(layout, B, Hkv, Tmax, D), dc.cache_shape(layout, B, Hkv, Tmax, Dv)
    p = gqa.plan_gqa_decode((B, H, D), kc, vc, 200, True, (B, Hkv, D), (B, Hkv, Dv), layout=layout)
    base = dc.plan_decode((B, Hkv, D), kc, vc, 200, True, (B, Hkv, D), (B, Hkv, Dv), layout=layout)
    assert (p.group, p.states, p.keys, p.chunks) == (4, 4, 201, 4)
    assert p.geometry() == (B, H, Hkv, 200, Tmax, D, Dv)
    assert p.q_strides == (H * D, D, 0) and p.o_strides == (H * Dv, Dv, 0)
    assert p.strides() == p.q_strides + base.knew_strides + base.vnew_strides + base.kcache_strides + base.vcache_strides + p.o_strides
    # the split follows the number of workgroup ROWS, B Hkv — not B H
    assert p.splits == base.splits == dc.choose_splits(B * Hkv, 4) == 4
    assert p.out_shape == (B, H, Dv)
    assert p.workspace_bytes(4) == (B * H * 4 * (Dv + 2) * 4 + 15) // 16 * 16
    assert gqa.plan_gqa_decode((B, H, D), kc, vc, 200, True, (B, Hkv, D), (B, Hkv, Dv), layout=layout, splits=1).workspace_bytes(4) == 0
    assert gqa.plan_gqa_decode((B, 6, D), kc, vc, 200, layout=layout).states == 4            # group 3 runs in four states


def test_decode_plan_ragged_and_refusals():
    kc, vc = (2, 130, 2, 8), (2, 130, 2, 8)
    p = gqa.plan_gqa_decode((2, 4, 8), kc, vc, None, True, (2, 2, 8), (2, 2, 8), lens_shape=(2,), splits=3)
    assert p.ragged and p.length is None and p.chunks == 3 and p.splits == 3 and p.geometry() == (2, 4, 2, 130, 8, 8)
    with pytest.raises(ValueError, match="not both"):
        gqa.plan_gqa_decode((2, 4, 8), kc, vc, 3, lens_shape=(2,))
    with pytest.raises(ValueError, match="not both"):
        gqa.plan_gqa_decode((2, 4, 8), kc, vc)
    with pytest.raises(ValueError, match="k_new and v_new are required"):
        gqa.plan_gqa_decode((2, 4, 8), kc, vc, lens_shape=(2,))
    with pytest.raises(ValueError, match="one length per sequence"):
        gqa.plan_gqa_decode((2, 4, 8), kc, vc, None, True, (2, 2, 8), (2, 2, 8), lens_shape=(3,))
    with pytest.raises(ValueError, match="no multiple"):
        gqa.plan_gqa_decode((2, 3, 8), kc, vc, 3)
    with pytest.raises(ValueError, match="gqa_decode: k_new must be"):
        gqa.plan_gqa_decode((2, 4, 8), kc, vc, 3, True, (2, 4, 8), (2, 2, 8))                # k_new holds Hkv heads
    with pytest.raises(ValueError, match="gqa_decode: the cache is full"):
        gqa.plan_gqa_decode((2, 4, 8), kc, vc, 130, True, (2, 2, 8), (2, 2, 8))
    with pytest.raises(ValueError, match="gqa_decode: splits 4 outside"):
        gqa.plan_gqa_decode((2, 4, 8), kc, vc, 129, True, (2, 2, 8), (2, 2, 8), splits=4)
    with pytest.raises(ValueError, match="layout must be one of"):
        gqa.plan_gqa_decode((2, 4, 8), kc, vc, 3, layout="tbhd")
    with pytest.raises(ValueError, match=r"q must be \[B, H, D\]"):
        gqa.plan_gqa_decode((2, 1, 4, 8), kc, vc, 3)
    with pytest.raises(ValueError, match="does not match"):
        gqa.plan_gqa_decode((2, 4, 9), kc, vc, 3)                                          # head dimension of q and the cache
