"""csrc/tnn_kvq.hip on the MI355X: the quantizing fill against the format's properties, the decoding step against float64 over
the device's OWN codes under the derived bound of tests/kvq_oracle.py, the ragged form bit-equal to the host-length call
sequence by sequence, and generation through KVCache(quant="int8").  Shapes are the smallest at which a path can go wrong:
head dimensions of 1, 4 and 8 lanes per key and one Dv != D, groups 1, 2, 3 (a spare query state) and 8 (q in LDS), lengths
around the 256-key chunk and beyond one pass of the key loop, every split count the planner can choose."""

import gc

import numpy as np
import pytest

import kvq_oracle as ko
import token_support as ts
import tinynn_autograd_amd as tn
from tinynn_autograd_amd import _lib, device_array as da, generation as gen, kvq

pytestmark = pytest.mark.gpu
C = kvq.CHUNK


def bits(a):
    return np.ascontiguousarray(a).view({1: np.uint8, 4: np.uint32}[a.dtype.itemsize])


def rows(layout, first, stop=None):
    return (slice(None),) * (1 if layout == "bthd" else 2) + (first if stop is None else slice(first, stop),)


def poisoned(rs, layout, b, hkv, tmax, d, dv, live):
    """Host caches: rows [0, live) quantized from random floats, every other row arbitrary codes under NaN scales."""
    out = []
    for w, amp in ((d, 1.0), (dv, 3.0)):
        codes = rs.randint(0, 256, kvq.codes_shape(layout, b, hkv, tmax, w)).astype(np.uint8)
        scales = np.full(kvq.scales_shape(layout, b, hkv, tmax), np.nan, dtype=np.float32)
        c, s = kvq.quantize_host((rs.randn(b, live, hkv, w) * amp).astype(np.float32))
        if layout == "bhtd":
            c, s = c.transpose(0, 2, 1, 3), s.transpose(0, 2, 1)
        codes[rows(layout, 0, live)], scales[rows(layout, 0, live)] = c, s
        out += [codes, scales]
    return out[0], out[2], out[1], out[3]                      # k_codes, v_codes, k_scales, v_scales


UPLOADED = []


def upload(host):
    dev = [da.asarray(a, dtype=a.dtype) for a in host]
    UPLOADED.extend(dev)
    return dev


@pytest.fixture(autouse=True)
def scrub_the_poison():
    """The poisoned caches (random bytes, NaN scales) are zeroed and every buffer of a test goes back to the native pool when
    the test ends: the pool hands recycled memory out as it is, and the trainers' native allocations of later test files find
    the blocks they found before this file existed instead of asking the driver for new ones."""
    yield
    while UPLOADED:
        UPLOADED.pop().fill(0)
    gc.collect()                     # (models and captured steps in reference cycles release their buffers now, not later)
    da.trim_cache()


def test_backend_and_entry_points():
    assert tn.backend_name() == "hip-gfx950" and _lib.get().has_kvq


@pytest.mark.parametrize("row0", [0, 3])
@pytest.mark.parametrize("t", [1, 5])
@pytest.mark.parametrize("layout", ["bthd", "bhtd"])
@pytest.mark.parametrize("d", [16, 48, 128])
def test_quantize_rows(d, layout, t, row0):
    b, hkv, dv, tmax = 2, 3, 32, 9
    rs = np.random.RandomState(d + t + row0)
    k = (rs.randn(b, t, hkv, d) * np.exp(rs.randn(b, t, hkv, 1) * 3)).astype(np.float32)
    v = (rs.randn(b, t, hkv, dv) * 3).astype(np.float32)
    k[1, t - 1, 2] = 0.0                                          # a zero row: scale 0, codes 0
    before = poisoned(rs, layout, b, hkv, tmax, d, dv, 0)
    dev = upload(before)
    da.kvq_quantize_rows(k, v, dev[0], dev[1], dev[2], dev[3], row0, layout, route="native")
    after = [np.asarray(a) for a in dev]
    move = (lambda a: a.transpose(0, 2, 1, 3) if a.ndim == 4 else a.transpose(0, 2, 1)) if layout == "bhtd" else (lambda a: a)
    at = rows(layout, row0, row0 + t)
    ko.check_rows(k, move(after[0][at]), move(after[2][at]), "k")
    ko.check_rows(v, move(after[1][at]), move(after[3][at]), "v")
    for got, was in zip(after, before):                          # the rows outside [row0, row0 + t) keep their poison
        got, was = bits(got).copy(), bits(was).copy()
        got[at], was[at] = 0, 0
        assert np.array_equal(got, was)


# (D, Dv, group): 1, 4 and 8 lanes per key, Dv on either side of D; every compiled state count and a spare state
GEOMETRY = [(16, 16, 1), (16, 16, 2), (16, 32, 3), (16, 16, 8), (64, 64, 1), (64, 32, 2), (64, 64, 3), (64, 64, 8),
            (128, 128, 1), (128, 128, 2), (128, 128, 3), (128, 128, 8)]


@pytest.mark.parametrize("length", [0, 1, C - 1, C, C + 1, 3 * C + 5])
@pytest.mark.parametrize("d, dv, group", GEOMETRY)
def test_decode_against_float64_on_the_devices_codes(d, dv, group, length):
    layout = "bthd" if (d // 16 + group + length) % 2 else "bhtd"
    b, hkv, tmax = 2, 2, length + 3
    rs = np.random.RandomState(1000 * d + 10 * group + length % 97)
    q = (rs.randn(b, hkv * group, d) * 4).astype(np.float32)
    kn, vn = rs.randn(b, hkv, d).astype(np.float32), (rs.randn(b, hkv, dv) * 3).astype(np.float32)
    before = poisoned(rs, layout, b, hkv, tmax, d, dv, length)
    chunks = -(-(length + 1) // C)
    for splits in sorted({1, min(2, chunks), chunks}):
        dev = upload(before)
        o = np.asarray(da.attention_decode_kvq(q, dev[0], dev[1], dev[2], dev[3], length, kn, vn, layout=layout, route="native",
                                               splits=splits))
        after = [np.asarray(a) for a in dev]
        what = "D %d Dv %d group %d len %d %s splits %d" % (d, dv, group, length, layout, splits)
        at = rows(layout, length)
        ko.check_rows(kn, after[0][at], after[2][at], what + " appended k")
        ko.check_rows(vn, after[1][at], after[3][at], what + " appended v")
        for got, was in zip(after, before):                      # every other row is untouched, NaN scales included
            got, was = bits(got).copy(), bits(was).copy()
            got[at], was[at] = 0, 0
            assert np.array_equal(got, was), what
        want, bound = ko.decode_reference(q, after[0], after[1], after[2], after[3], length + 1, None, layout, splits)
        err = np.abs(o.astype(np.float64) - want)
        print("%s: max error / bound %.3f" % (what, (err / np.maximum(bound, 1e-300)).max()))
        assert np.isfinite(o).all() and (err <= bound).all(), what


@pytest.mark.parametrize("layout, group", [("bthd", 1), ("bhtd", 3), ("bthd", 8)])
def test_ragged_equals_the_host_length_call_per_sequence(layout, group):
    b, hkv, d, dv, tmax, splits = 5, 2, 64, 64, 3 * C - 60, 3
    lens = np.array([0, C - 1, C, 2 * C + 40, tmax], dtype=np.int64)      # chunk edges, one 0, one outside [0, Tmax)
    rs = np.random.RandomState(7 + group)
    q = (rs.randn(b, hkv * group, d) * 4).astype(np.float32)
    kn, vn = rs.randn(b, hkv, d).astype(np.float32), (rs.randn(b, hkv, dv) * 3).astype(np.float32)
    before = poisoned(rs, layout, b, hkv, tmax, d, dv, tmax - 1)
    dev = upload(before)
    o = np.asarray(da.attention_decode_kvq(q, dev[0], dev[1], dev[2], dev[3], k_new=kn, v_new=vn, lens=da.lengths(lens),
                                           layout=layout, route="native", splits=splits))
    after = [np.asarray(a) for a in dev]
    for i, n in enumerate(lens):
        one = slice(i, i + 1)
        if not 0 <= n < tmax:
            assert not o[i].any() and all(np.array_equal(bits(g[one]), bits(w[one])) for g, w in zip(after, before))
            continue
        alone = upload([a[one] for a in before])
        want = np.asarray(da.attention_decode_kvq(q[one], alone[0], alone[1], alone[2], alone[3], int(n), kn[one], vn[one],
                                                  layout=layout, route="native", splits=min(splits, -(-(int(n) + 1) // C))))
        assert np.array_equal(bits(o[one]), bits(want)), "sequence %d (len %d)" % (i, n)
        assert all(np.array_equal(bits(g[one]), bits(np.asarray(w))) for g, w in zip(after, alone))


@pytest.mark.parametrize("kv_heads", [None, 2])
def test_generate_eager_captured_and_composed(kv_heads):
    """Greedy generation over an int8 cache on a two-block model: the captured ids are the eager ones, and the logits of the
    first decoding step lie within twice the decode bound (kvq_oracle, evaluated at this step's attention shape on inputs of
    the oracle's amplitudes) of the logits the composed route gives from the same cache."""
    ex = ts.load_example()
    np.random.seed(5)
    argv = ["--width", "64", "--heads", "4", "--seq", "16", "--vocab", "13"] + (["--kv-heads", "2"] if kv_heads else [])
    model, _ = ex.build(ex.parse(argv))
    b, p, n, hkv, d = 2, 4, 8, kv_heads or 4, 16
    prompt = np.random.RandomState(6).randint(0, 13, (b, p))
    eager = gen.generate(model, prompt, n, temperature=0.0, cache=gen.KVCache(p + n, quant="int8"), prompt_lens=np.full(b, p))
    captured = gen.generate(model, prompt, n, temperature=0.0, cache=gen.KVCache(p + n, quant="int8"), capture=True)
    uniform = gen.generate(model, prompt, n, temperature=0.0, cache=gen.KVCache(p + n, quant="int8"))
    assert np.array_equal(eager, captured) and np.array_equal(eager, uniform)

    def first_step_logits(route):
        cache = gen.KVCache(p + n, quant="int8")
        model.set_phase("TEST")
        try:
            gen._forward(model.net.layers, tn.Tensor(prompt), 0, cache)
            da.KVQ_ROUTE = route
            return np.asarray(gen._forward(model.net.layers, tn.Tensor(eager[:, p:p + 1]), p, cache).values, dtype=np.float64)
        finally:
            da.KVQ_ROUTE = None
            model.set_phase("TRAIN")

    rs = np.random.RandomState(8)
    host = poisoned(rs, "bthd", b, hkv, p + 1, d, d, p + 1)
    _, bound = ko.decode_reference((rs.randn(b, 4, d) * 4).astype(np.float32), host[0], host[1], host[2], host[3], p + 1)
    diff = np.abs(first_step_logits("native") - first_step_logits("composed"))
    print("first decode step: max logit difference %.3e, twice the bound %.3e" % (diff.max(), 2 * bound.max()))
    assert (diff <= 2 * bound.max()).all()
