"""The host planner of cache-extending attention (extend.py, numpy only): geometry, the strides of both layouts, the grid, the
key blocks a query block walks, the routes, and every refusal — each raised before anything could be launched."""

import pytest

from tinynn_autograd_amd import extend as ex


def shapes(layout, b, h, hkv, tmax, t, d, dv):
    s = lambda heads, rows, w: ex.operand_shape(layout, b, heads, rows, w)
    return dict(q_shape=s(h, t, d), k_cache_shape=s(hkv, tmax, d), v_cache_shape=s(hkv, tmax, dv), k_new_shape=s(hkv, t, d),
                v_new_shape=s(hkv, t, dv))


def plan(layout="bthd", b=2, h=4, hkv=2, tmax=300, t=70, d=16, dv=24, length=100, **kw):
    return ex.plan_extend(length=length, layout=layout, **dict(shapes(layout, b, h, hkv, tmax, t, d, dv), **kw))


def test_geometry_strides_and_grid():
    p = plan("bthd")
    assert p.geometry() == (2, 4, 2, 70, 100, 300, 16, 24) and p.group == 2 and p.keys == 170 and p.route == "native"
    assert p.out_shape == (2, 70, 4, 24) and p.scale == 0.25 and not p.empty()
    # (batch, head, row) of q, k_new, v_new, k_cache, v_cache, o
    assert p.strides() == (70 * 64, 16, 64) + (70 * 32, 16, 32) + (70 * 48, 24, 48) + (300 * 32, 16, 32) + (300 * 48, 24, 48) \
        + (70 * 96, 24, 96)
    assert p.query_blocks() == 2 and p.grid() == 2 * 4 * 2 and p.grid(8) == -(-2 * 4 * 70 // 4)
    q = plan("bhtd")
    assert q.geometry() == p.geometry() and q.out_shape == (2, 4, 70, 24)
    assert q.strides() == (4 * 70 * 16, 70 * 16, 16) + (2 * 70 * 16, 70 * 16, 16) + (2 * 70 * 24, 70 * 24, 24) \
        + (2 * 300 * 16, 300 * 16, 16) + (2 * 300 * 24, 300 * 24, 24) + (4 * 70 * 24, 70 * 24, 24)
    assert plan(h=0, hkv=0).empty() and plan(b=0).empty()
    assert plan(scale=0.5).scale == 0.5 and plan(hkv=4).group == 1 and plan(h=8, hkv=1).group == 8
    assert plan(length=0).keys == 70 and plan(length=230).keys == 300            # a prefill; the cache exactly full


def test_key_blocks_are_aligned_to_the_absolute_index():
    p = plan(length=100, t=70)
    # rows 0 .. 63 sit at positions 100 .. 163: blocks 0, 64, 128 (up to key 164 of 170); rows 64 .. 69 see every key
    assert p.key_blocks(0) == [(0, 64), (64, 128), (128, 170)]
    assert p.key_blocks(64) == [(0, 64), (64, 128), (128, 170)]
    p = plan(length=37, t=150)
    assert p.key_blocks(0) == [(0, 64), (64, 128)]                               # position 37 + 63 = 100 lies in block 64
    assert p.key_blocks(128)[-1] == (128, 187)
    assert all(k0 % ex.BLOCK_K == 0 for q0 in (0, 64, 128) for k0, _ in p.key_blocks(q0))
    assert plan(length=0, t=64).key_blocks(0) == [(0, 64)] and plan(length=1, t=64).key_blocks(0) == [(0, 64), (64, 65)]


def test_routes():
    assert ex.ROUTES == ("native", "composed") and ex.RULES == ()
    assert plan(native=False).route == "composed" and plan(float_ok=False).route == "composed"
    assert plan(route="composed").route == "composed" and plan(route="native").route == "native"
    assert plan(d=129, tmax=200).route == "composed" and plan(dv=200).route == "composed"   # beyond the kernel: composed
    big = dict(b=1, h=1, hkv=1, d=128, dv=128)
    assert plan(tmax=(1 << 24) - 1, **big).route == "native" and plan(tmax=1 << 24, **big).route == "composed"
    for kw in (dict(native=False), dict(float_ok=False), dict(d=129), dict(tmax=1 << 24, **big)):
        with pytest.raises(ValueError, match="the native attention_extend route needs"):
            plan(route="native", **kw)
    with pytest.raises(ValueError, match="route must be one of"):
        plan(route="fwd")


@pytest.mark.parametrize("kw,msg", [
    (dict(length=231), "length 231 \\+ T 70 new rows overflow a cache of 300 rows"),
    (dict(length=300), "overflow a cache of 300 rows"),
    (dict(t=301, length=0), "overflow a cache of 300 rows"),
    (dict(length=-1), "length -1 must be >= 0"),
    (dict(length=1.0), "length must be an integer"),
    (dict(length=True), "length must be an integer"),
    (dict(t=0), "T = 0 new rows"),
    (dict(h=3, hkv=2), "H 3 query heads is no multiple of Hkv 2"),
    (dict(h=0, hkv=2), "is no multiple"),
    (dict(d=0), "empty head dimension or cache"),
    (dict(tmax=0, length=0), "empty head dimension or cache"),
    (dict(scale=float("inf")), "scale must be finite"),
    (dict(layout="hbtd"), "layout must be one of"),
    (dict(pointers=(10, 20, 10, 30)), "alias a cache"),
    (dict(pointers=(10, 30, 20, 30)), "alias a cache"),
])
def test_refusals(kw, msg):
    with pytest.raises(ValueError, match="attention_extend: .*" + msg if "layout" not in kw else msg):
        plan(**kw)
    assert plan(pointers=(1, 2, 3, 4)).route == "native"


def test_shape_mismatches():
    base = shapes("bthd", 2, 4, 2, 300, 70, 16, 24)
    bad = [("q_shape", (2, 70, 4), "four axes"), ("k_cache_shape", (3, 300, 2, 16), "k_cache .* does not match q"),
           ("k_cache_shape", (2, 300, 2, 17), "k_cache .* does not match q"),
           ("v_cache_shape", (2, 299, 2, 24), "v_cache .* does not match k_cache"),
           ("v_cache_shape", (2, 300, 4, 24), "v_cache .* does not match k_cache"),
           ("k_new_shape", (2, 70, 4, 16), "k_new must be \\(2, 70, 2, 16\\)"),
           ("k_new_shape", (2, 69, 2, 16), "k_new must be"), ("v_new_shape", (2, 70, 2, 16), "v_new must be \\(2, 70, 2, 24\\)"),
           ("v_new_shape", (2, 2, 70, 24), "v_new must be")]
    for name, shape, msg in bad:
        with pytest.raises(ValueError, match="attention_extend: .*" + msg):
            ex.plan_extend(length=100, **dict(base, **{name: shape}))
    # the other layout reads the same shapes differently: 70 heads over 300
    with pytest.raises(ValueError, match="attention_extend: H 70 query heads is no multiple of Hkv 300"):
        ex.plan_extend(length=100, layout="bhtd", **base)
