"""tinynn-autograd_amd/decoding.py: the plans of a decoding step — extents, strides of both cache layouts, the key split and
its clamps, workspace sizes, routes, and every validation error.  numpy only: nothing here touches a device."""

import math

import pytest

from tinynn_autograd_amd import decoding as dc


def plan(b=2, h=3, tmax=300, d=16, dv=24, length=100, layout="bthd", **kw):
    return dc.plan_decode((b, h, d), dc.cache_shape(layout, b, h, tmax, d), dc.cache_shape(layout, b, h, tmax, dv), length,
                          layout=layout, **kw)


def test_extents_scale_and_strides_of_both_layouts():
    p = plan()
    assert p.geometry() == (2, 3, 100, 300, 16, 24) and p.out_shape == (2, 3, 24)
    assert p.append and p.keys == 101 and p.chunks == 2
    assert p.scale == 1.0 / math.sqrt(16) and plan(scale=0.5).scale == 0.5
    assert p.q_strides == p.knew_strides == (48, 16, 0) and p.vnew_strides == p.o_strides == (72, 24, 0)
    assert p.kcache_strides == (300 * 3 * 16, 16, 3 * 16) and p.vcache_strides == (300 * 3 * 24, 24, 3 * 24)
    t = plan(layout="bhtd")
    assert t.kcache_strides == (3 * 300 * 16, 300 * 16, 16) and t.vcache_strides == (3 * 300 * 24, 300 * 24, 24)
    assert t.q_strides == p.q_strides and len(t.strides()) == 18
    assert t.strides()[9:12] == t.kcache_strides and t.strides()[15:] == t.o_strides
    n = plan(append=False)
    assert not n.append and n.keys == 100 and n.chunks == 2
    assert plan(append=False, length=300).keys == 300                # a full cache can still be read


def test_split_choice_and_its_clamps():
    assert dc.choose_splits(1, 1) == 1
    assert dc.choose_splits(8, 512) == min(math.ceil(dc.TARGET / 8), dc.MAX_SPLITS, 512)
    assert dc.choose_splits(1, 10 ** 6) == dc.MAX_SPLITS                # never more than the header allows
    assert dc.choose_splits(10 ** 6, 10 ** 6) == 1                     # enough (b, h) already
    assert dc.choose_splits(dc.TARGET // 2, 100) == 2
    assert plan(length=0).splits == 1 and plan(length=63).splits == 1 and plan(length=64).splits == 2   # by the chunks
    p = plan(b=1, h=3, tmax=400, length=300, splits=3)
    assert p.chunks == 5 and p.runs() == [(0, 1), (1, 3), (3, 5)]
    assert [b - a for a, b in plan(b=1, h=3, tmax=400, length=300, splits=2).runs()] == [2, 3]
    for s in (1, 2, 3, 4, 5):
        runs = plan(tmax=400, length=300, splits=s).runs()
        assert runs[0][0] == 0 and runs[-1][1] == 5 and all(a < b for a, b in runs)
        assert all(runs[i][1] == runs[i + 1][0] for i in range(s - 1))


def test_fwd_route_and_its_rules(monkeypatch):
    assert dc.FWD_RULES == () or all(len(r) == 2 for r in dc.FWD_RULES)
    assert plan(route="fwd").route == "fwd"
    for kw in (dict(native=False), dict(float_ok=False), dict(d=129)):
        with pytest.raises(ValueError, match="fwd decode attention route"):
            plan(route="fwd", **kw)
    with pytest.raises(ValueError, match="fwd decode attention route"):                 # 2^31 elements: tnn_attn_fwd refuses
        plan(b=64, h=8, tmax=32769, d=128, dv=128, length=32768, route="fwd")
    with pytest.raises(ValueError, match="route must be one of"):
        dc.plan_sample((5, 9), (5,), route="fwd")
    monkeypatch.setattr(dc, "FWD_RULES", ((6, 128),))                                   # B H >= 6 and at most 128 keys
    assert plan(length=100).route == "fwd" and plan(length=128).route == "native" and plan(b=1, length=100).route == "native"
    assert plan(length=100, native=False).route == "composed" and plan(length=100, route="native").route == "native"
    monkeypatch.setattr(dc, "FWD_RULES", ((1, 1 << 40),))
    assert plan(b=64, h=8, tmax=32769, d=128, dv=128, length=32768).route == "native"   # too large for the old route


def test_workspace():
    assert plan(splits=1).workspace_bytes(4) == 0
    assert plan(splits=2).workspace_bytes(4) == (2 * 3 * 2 * 26 * 4 + 15) // 16 * 16
    assert plan(b=1, h=1, dv=1, splits=2).workspace_bytes(8) == 48
    assert plan(b=1, h=1, dv=1, splits=2).workspace_bytes(4) == 32           # 24 rounded up


def test_routes():
    assert plan().route == "native" and plan(native=False).route == "composed" and plan(float_ok=False).route == "composed"
    assert plan(route="composed").route == "composed"
    assert plan(d=129, length=5).route == "composed"
    for kw in (dict(native=False), dict(float_ok=False), dict(d=129)):
        with pytest.raises(ValueError, match="native decode attention route"):
            plan(route="native", **kw)
    with pytest.raises(ValueError, match="route must be one of"):
        plan(route="fast")


@pytest.mark.parametrize("call,msg", [
    (lambda: plan(layout="tbhd"), "layout must be one of"),
    (lambda: dc.plan_decode((2, 3, 1, 16), (2, 8, 3, 16), (2, 8, 3, 16), 1), r"q must be \[B, H, D\]"),
    (lambda: dc.plan_decode((2, 3, 16), (2, 8, 16), (2, 8, 3, 16), 1), "four axes"),
    (lambda: dc.plan_decode((2, 3, 16), (2, 8, 4, 16), (2, 8, 3, 16), 1), "k_cache .* does not match q"),
    (lambda: dc.plan_decode((2, 3, 16), (2, 3, 8, 16), (2, 3, 8, 16), 1), "k_cache .* does not match q"),       # the other layout
    (lambda: dc.plan_decode((2, 3, 16), (2, 8, 3, 16), (2, 9, 3, 16), 1), "v_cache .* does not match"),
    (lambda: dc.plan_decode((2, 3, 0), (2, 8, 3, 0), (2, 8, 3, 4), 1), "empty head dimension"),
    (lambda: dc.plan_decode((70000, 1, 4), (70000, 8, 1, 4), (70000, 8, 1, 4), 1), "must stay below"),
    (lambda: plan(k_new_shape=(2, 3, 17)), "k_new must be"),
    (lambda: plan(v_new_shape=(2, 3, 16)), "v_new must be"),
    (lambda: plan(length=2.5), "length must be an integer"),
    (lambda: plan(length=True), "length must be an integer"),
    (lambda: plan(length=300), "the cache is full"),
    (lambda: plan(length=301), r"outside \[0, 300\)"),
    (lambda: plan(length=-1), r"outside \[0, 300\)"),
    (lambda: plan(append=False, length=0), "without k_new / v_new length must be in"),
    (lambda: plan(append=False, length=301), "without k_new / v_new length must be in"),
    (lambda: plan(splits=0), r"splits 0 outside \[1, 2\]"),
    (lambda: plan(splits=3), r"splits 3 outside \[1, 2\]"),
    (lambda: plan(splits=1.5), "splits must be an integer"),
    (lambda: plan(scale=float("inf")), "scale must be finite"),
])
def test_decode_validation(call, msg):
    with pytest.raises(ValueError, match=msg):
        call()


def test_splits_never_exceed_the_header_limit():
    p = plan(b=1, h=1, tmax=64 * 300, length=64 * 300 - 1)
    assert p.chunks == 300 and p.splits == dc.MAX_SPLITS
    with pytest.raises(ValueError, match=r"outside \[1, %d\]" % dc.MAX_SPLITS):
        plan(b=1, h=1, tmax=64 * 300, length=64 * 300 - 1, splits=dc.MAX_SPLITS + 1)


def test_sample_plan():
    p = dc.plan_sample((5, 100), (5,), 0.7, 10, itemsize=4)
    assert (p.M, p.V, p.temperature, p.top_k, p.greedy, p.passes, p.route) == (5, 100, 0.7, 10, False, 4, "native")
    assert dc.plan_sample((5, 100), (5,), 1.0, 10, itemsize=8).passes == 8
    for k in (None, 100, 101):
        q = dc.plan_sample((5, 100), (5,), 1.0, k)
        assert q.top_k == 0 and q.passes == 0                  # every column: no select
    g = dc.plan_sample((5, 100), None, 0.0, 3)
    assert g.greedy and g.passes == 0                          # u is not read
    assert dc.plan_sample((0, 7), (0,)).empty()
    assert dc.plan_sample((5, 100), (5,), native=False).route == "composed"
    with pytest.raises(ValueError, match="native sampling route"):
        dc.plan_sample((5, 100), (5,), native=False, route="native")


@pytest.mark.parametrize("call,msg", [
    (lambda: dc.plan_sample((5,), (5,)), r"must be \[M, V\]"),
    (lambda: dc.plan_sample((5, 0), (5,)), r"must be \[M, V\]"),
    (lambda: dc.plan_sample((1, 1 << 31), (1,)), "below 2\\^31"),
    (lambda: dc.plan_sample((5, 9), (5,), temperature=-1.0), "temperature must be finite"),
    (lambda: dc.plan_sample((5, 9), (5,), temperature=float("nan")), "temperature must be finite"),
    (lambda: dc.plan_sample((5, 9), (5,), top_k=0), "top_k must be >= 1 or None"),
    (lambda: dc.plan_sample((5, 9), (5,), top_k=2.0), "top_k must be an integer"),
    (lambda: dc.plan_sample((5, 9), (4,)), "one number per row"),
    (lambda: dc.plan_sample((5, 9), None), "one number per row"),
    (lambda: dc.plan_sample((5, 9), (5,), route="fast"), "route must be one of"),
])
def test_sample_validation(call, msg):
    with pytest.raises(ValueError, match=msg):
        call()


def test_the_host_rule():
    """decoding.sample_host, the composed route: ties at the threshold go to the lowest indices, -inf is never chosen, the
    fallback is the last column of positive weight."""
    import numpy as np
    x = np.array([[1.0, 3.0, 3.0, 3.0, -np.inf, 0.0]], dtype=np.float32)
    assert dc.sample_host(x, None, 0.0, 0).tolist() == [1]
    assert dc.sample_host(x, [0.0], 1.0, 2).tolist() == [1] and dc.sample_host(x, [0.999], 1.0, 2).tolist() == [2]
    assert dc.sample_host(x, [0.999999], 1.0, 0).tolist() == [5]
    assert dc.sample_host(np.array([[-np.inf, 0.0, -np.inf]]), [0.0], 1.0, 0).tolist() == [1]
    assert dc.sample_host(np.array([[-np.inf, 0.0, -np.inf]]), [np.nextafter(1.0, 0.0)], 2.0, 0).tolist() == [1]
