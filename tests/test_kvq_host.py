"""The int8 key / value cache on the host side (kvq.py, the composed routes, KVCache(quant=)): planner routes and messages, the
format's properties on quantize_host, the composed decode against the float64 reference over its own codes, and generation."""

import numpy as np
import pytest

import kvq_oracle as ko
import token_support as ts
import tinynn_autograd_amd as tn
from tinynn_autograd_amd import device_array as da, generation as gen, kvq


def shapes(layout, b, h, hkv, tmax, d, dv):
    return ((b, h, d), kvq.codes_shape(layout, b, hkv, tmax, d), kvq.codes_shape(layout, b, hkv, tmax, dv),
            kvq.scales_shape(layout, b, hkv, tmax), kvq.scales_shape(layout, b, hkv, tmax))


def test_planner_routes_splits_and_messages():
    args = shapes("bhtd", 2, 8, 2, 1000, 64, 32)
    new = dict(k_new_shape=(2, 2, 64), v_new_shape=(2, 2, 32))
    p = kvq.plan_kvq_decode(*args, length=600, **new, layout="bhtd")
    assert (p.route, p.group, p.states, p.keys, p.chunks, p.splits) == ("native", 4, 4, 601, 3, 3)
    assert p.kcodes_strides == (2 * 1000 * 64, 1000 * 64, 64) and p.kscales_strides == (2000, 1000, 1)
    assert p.workspace_bytes() == 2 * 8 * 3 * 34 * 4 and len(p.strides()) == 24
    r = kvq.plan_kvq_decode(*args, lens_shape=(2,), **new, layout="bhtd")
    assert r.ragged and r.chunks == 4 and r.geometry()[3] == 0          # the grid comes from the cache's rows
    # what the kernel cannot take goes to the composed route, and asking for it natively says why
    odd = shapes("bthd", 1, 2, 2, 8, 24, 16)
    assert kvq.plan_kvq_decode(*odd, length=0, k_new_shape=(1, 2, 24), v_new_shape=(1, 2, 16)).route == "composed"
    for kw in (dict(native=False), dict(float_ok=False), dict(aligned=False)):
        assert kvq.plan_kvq_decode(*args, length=0, **new, layout="bhtd", **kw).route == "composed"
        with pytest.raises(ValueError, match="native int8 decode attention route needs"):
            kvq.plan_kvq_decode(*args, length=0, **new, layout="bhtd", route="native", **kw)
    with pytest.raises(ValueError, match="the cache is full"):
        kvq.plan_kvq_decode(*args, length=1000, **new, layout="bhtd")
    with pytest.raises(ValueError, match=r"splits 4 outside \[1, 3\]"):
        kvq.plan_kvq_decode(*args, length=600, **new, layout="bhtd", splits=4)
    with pytest.raises(ValueError, match="not both"):
        kvq.plan_kvq_decode(*args, length=3, lens_shape=(2,), **new, layout="bhtd")
    with pytest.raises(ValueError, match="k_new and v_new are required"):
        kvq.plan_kvq_decode(*args, length=3, layout="bhtd")
    with pytest.raises(ValueError, match="one per cache row"):
        kvq.plan_kvq_decode(*args[:4], (2, 1000, 2), length=3, **new, layout="bhtd")
    f = kvq.plan_kvq_fill((2, 5, 2, 64), (2, 5, 2, 32), *args[1:], row0=3, layout="bhtd")
    assert f.route == "native" and f.geometry() == (2, 5, 2, 64, 32, 3, 1000)
    with pytest.raises(ValueError, match=r"rows \[998, 1003\) lie outside"):
        kvq.plan_kvq_fill((2, 5, 2, 64), (2, 5, 2, 32), *args[1:], row0=998, layout="bhtd")


@pytest.mark.parametrize("width", [16, 48, 128])
def test_quantize_host_keeps_the_formats_properties(width):
    rs = np.random.RandomState(width)
    x = (rs.randn(7, 3, width) * np.exp(rs.randn(7, 3, 1) * 3)).astype(np.float32)
    x[2, 1] = 0.0
    x[3, 0, 1:] = 0.0                                             # one non-zero: code +-127 exactly
    codes, scales = kvq.quantize_host(x)
    assert codes.dtype == np.uint8 and scales.dtype == np.float32 and codes.shape == x.shape and scales.shape == (7, 3)
    ko.check_rows(x, codes, scales, "quantize_host W %d" % width)
    assert abs(int(codes.view(np.int8)[3, 0, 0])) == 127
    back = kvq.dequantize_host(codes, scales)
    assert back.dtype == np.float64 and np.abs(back - x).max() <= np.abs(x).max() / 127


@pytest.mark.parametrize("layout, group, length, ragged", [("bthd", 1, 0, False), ("bhtd", 2, 70, False), ("bthd", 3, 9, True)])
def test_composed_decode_against_float64(layout, group, length, ragged):
    b, hkv, d, dv, tmax = 2, 2, 16, 32, length + 4
    rs = np.random.RandomState(11 + length)
    q = (rs.randn(b, hkv * group, d) * 4).astype(np.float32)
    kn, vn = rs.randn(b, hkv, d).astype(np.float32), (rs.randn(b, hkv, dv) * 3).astype(np.float32)
    kc, vc = (da.zeros(kvq.codes_shape(layout, b, hkv, tmax, w), np.uint8) for w in (d, dv))
    ks, vs = (da.zeros(kvq.scales_shape(layout, b, hkv, tmax), np.float32) for _ in range(2))
    da.kvq_quantize_rows(rs.randn(b, length, hkv, d).astype(np.float32), (rs.randn(b, length, hkv, dv) * 3).astype(np.float32),
                         kc, vc, ks, vs, 0, layout)
    where = dict(lens=da.lengths(np.full(b, length))) if ragged else dict(length=length)
    o = np.asarray(da.attention_decode_kvq(q, kc, vc, ks, vs, k_new=kn, v_new=vn, layout=layout, **where))
    codes, scales = [np.asarray(a) for a in (kc, vc)], [np.asarray(a) for a in (ks, vs)]
    row = (slice(None),) * (1 if layout == "bthd" else 2) + (length,)
    ko.check_rows(kn, codes[0][row], scales[0][row], "the appended k row")
    ko.check_rows(vn, codes[1][row], scales[1][row], "the appended v row")
    want, bound = ko.decode_reference(q, codes[0], codes[1], scales[0], scales[1], length + 1, None, layout)
    assert o.dtype == np.float32 and (np.abs(o - want) <= bound).all()


def test_kvcache_quant_arguments():
    with pytest.raises(ValueError, match="extend=True with quant"):
        gen.KVCache(8, quant="int8", extend=True)
    with pytest.raises(ValueError, match="quant must be None or one of"):
        gen.KVCache(8, quant="int4")
    assert gen.KVCache(8, quant="int8").layer(0).quant == "int8" and gen.KVCache(8).layer(0).quant is None


def test_generate_with_and_without_quant():
    """quant=None is the parent's path (the ids of cache=True and of the uncached forward); an int8 cache generates through
    the composed route under the twin and leaves codes and scales behind."""
    ex = ts.load_example()
    np.random.seed(3)
    model, _ = ex.build(ex.parse(["--width", "32", "--heads", "2", "--kv-heads", "1", "--seq", "12", "--vocab", "11"]))
    prompt = np.random.RandomState(4).randint(0, 11, (2, 4))
    full = gen.generate(model, prompt, 5, temperature=0.0, cache=False)
    assert np.array_equal(gen.generate(model, prompt, 5, temperature=0.0), full)
    cache = gen.KVCache(9, quant="int8")
    ids = gen.generate(model, prompt, 5, temperature=0.0, cache=cache)
    assert ids.shape == (2, 9) and np.array_equal(ids[:, :4], prompt) and cache.length == 8
    layer = cache.layer(1)
    assert layer.k.dtype == np.uint8 and tuple(layer.k.shape) == (2, 9, 1, 16) and tuple(layer.k_scale.shape) == (2, 9, 1)
    with pytest.raises(ValueError, match="must be empty"):
        gen.generate(model, prompt, 5, temperature=0.0, cache=cache)
    if tn.backend_name() != "hip-gfx950":
        with pytest.raises(ValueError, match="capture=True over a quantized cache needs the native route"):
            gen.generate(model, prompt, 5, temperature=0.0, cache=gen.KVCache(9, quant="int8"), capture=True)


def test_the_rules_of_the_slower_shapes():
    assert kvq.expect_slower(1, 8, 257) and kvq.expect_slower(8, 64, 100)
    assert not kvq.expect_slower(1, 512, 257) and not kvq.expect_slower(8, 1, 4097) and not kvq.expect_slower(2, 8, 257)
