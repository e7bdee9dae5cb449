"""csrc/tnn_wq.hip on the MI355X: the quantizer against the format's properties, the skinny product against float64 over the
device's OWN codes under the derived bound of tests/wq_oracle.py, and generation from the codes alone.  Shapes are the
smallest at which a path can go wrong: every compiled row form and two with spare rows, one lane per k-block, a masked group,
a full group, one panel and a partial second one, K of one and two k-blocks and around one round of the workgroup, every
kind of split count the planner can choose."""

import gc

import numpy as np
import pytest

import token_support as ts
import wq_oracle as wo
import tinynn_autograd_amd as tn
from tinynn_autograd_amd import _lib, device_array as da, generation as gen, wq
from tinynn_autograd_amd.core import ops
from tinynn_autograd_amd.core.layers import Dense

pytestmark = pytest.mark.gpu
F32 = _lib.F32
UPLOADED = []


def upload(host):
    dev = da.asarray(host, dtype=host.dtype)
    UPLOADED.append(dev)
    return dev


@pytest.fixture(autouse=True)
def scrub_the_poison():
    """What a test poisoned (guard bytes, NaN weights) is zeroed and every buffer goes back to the native pool when the test
    ends, as in test_gpu_kvq.py."""
    yield
    while UPLOADED:
        UPLOADED.pop().fill(0)
    gc.collect()
    da.trim_cache()


def bits(a):
    return np.ascontiguousarray(a).view({1: np.uint8, 4: np.uint32}[a.dtype.itemsize])


def weight(rs, k, n):
    """Column magnitudes spread over e^+-3, one zero column."""
    w = (rs.randn(k, n) * np.exp(rs.uniform(-3, 3, (1, n)))).astype(np.float32)
    w[:, n // 2] = 0.0
    return w


def test_backend_and_entry_points():
    assert tn.backend_name() == "hip-gfx950" and _lib.get().has_wq


@pytest.mark.parametrize("n", [4, 12, 64, 256, 260])
@pytest.mark.parametrize("k, pad", [(4, 0), (8, 0), (260, 0), (260, 8)])
def test_quantize_and_dequantize(k, pad, n):
    rs = np.random.RandomState(1000 * k + n + pad)
    wide = np.full((k, n + pad), np.nan, dtype=np.float32)         # (the padding of a row is never read: NaN would show)
    wide[:, :n] = weight(rs, k, n)
    guard, lib = 64, _lib.get()
    codes_was = np.full(guard + k * n + guard, 0xAB, dtype=np.uint8)
    scales_was = np.full(guard // 4 + n + guard // 4, np.nan, dtype=np.float32)
    w_dev, codes_dev, scales_dev = upload(wide), upload(codes_was), upload(scales_was)
    lib.wq_quantize(w_dev._ptr, n + pad, codes_dev._ptr + guard, scales_dev._ptr + guard, k, n, F32)
    codes_got, scales_got = np.asarray(codes_dev), np.asarray(scales_dev)
    codes, scales = codes_got[guard:-guard].reshape(wq.codes_shape(k, n)), scales_got[guard // 4:-(guard // 4)]
    wo.check_weight(wide[:, :n], codes, scales, "K %d N %d pad %d" % (k, n, pad))
    for got, was, g in ((codes_got, codes_was, guard), (scales_got, scales_was, guard // 4)):      # the guards keep their poison
        assert np.array_equal(bits(got[:g]), bits(was[:g])) and np.array_equal(bits(got[-g:]), bits(was[-g:]))
    back = np.asarray(da.wq_dequantize(upload(codes), upload(scales)))
    assert np.array_equal(bits(back), bits(wq.unpack_codes(codes).astype(np.float32) * scales[None, :]))


def lengths(n):
    """K of one and two k-blocks, and one k-block below, at and above one round of the workgroup at this N's lane group."""
    one_pass = 4 * wq.pass_blocks(n)
    return sorted({4, 8, one_pass - 4, one_pass, one_pass + 4})


@pytest.mark.parametrize("n", [4, 12, 64, 256, 260, 516])
@pytest.mark.parametrize("m", [1, 2, 3, 5, 8, 16])
def test_linear_against_float64_on_the_devices_codes(m, n):
    rs = np.random.RandomState(100 * m + n)
    for k in lengths(n):
        x, b = (rs.randn(m, k) * 4).astype(np.float32), (rs.randn(1, n) * 2).astype(np.float32)
        codes, scales = da.wq_quantize(weight(rs, k, n))
        x_dev, b_dev = upload(x), upload(b)
        for bias in (b, None):
            want, bound = wo.linear_reference(x, np.asarray(codes), np.asarray(scales), bias)
            for splits in sorted({1, min(2, wq.most_splits(k)), wq.choose_splits(m, k, n), wq.most_splits(k)}):
                y, again = (np.asarray(da.wq_linear(x_dev, codes, scales, None if bias is None else b_dev, route="native",
                                                    splits=splits)) for _ in range(2))
                what = "M %d K %d N %d splits %d bias %s" % (m, k, n, splits, bias is not None)
                err = np.abs(y.astype(np.float64) - want)
                print("%s: max error / bound %.3f" % (what, (err / np.maximum(bound, 1e-300)).max()))
                assert np.isfinite(y).all() and (err <= bound).all(), what
                assert np.array_equal(bits(y), bits(again)), what


def test_linear_reads_a_padded_x_in_place():
    m, k, n, pad, splits = 5, 72, 260, 8, 3
    rs = np.random.RandomState(9)
    wide = np.full((m, k + pad), np.nan, dtype=np.float32)
    wide[:, :k] = rs.randn(m, k)
    codes, scales = da.wq_quantize(weight(rs, k, n))
    x_dev, y, ws = upload(wide), da.zeros((m, n), np.float32), da.zeros((splits * m * n,), np.float32)
    _lib.get().wq_linear(x_dev._ptr, k + pad, codes._ptr, scales._ptr, None, y._ptr, ws._ptr, ws.nbytes, m, k, n, splits, F32)
    want, bound = wo.linear_reference(wide[:, :k], np.asarray(codes), np.asarray(scales))
    assert (np.abs(np.asarray(y) - want) <= bound).all()


def test_more_rows_take_dequantize_and_the_gemm():
    """M = 17 > wq.MAX_ROWS: the weight is dequantized and the float32 GEMM runs.  It multiplies by fl(code scale) instead of
    scaling the finished sum — one rounding per term more than the derived bound counts — so TWICE the bound is allowed."""
    m, k, n = 17, 260, 260
    rs = np.random.RandomState(17)
    x, b = (rs.randn(m, k) * 4).astype(np.float32), rs.randn(1, n).astype(np.float32)
    codes, scales = da.wq_quantize(weight(rs, k, n))
    assert wq.plan_linear(x.shape, codes.shape, scales.shape, b.shape).kernel == "dequant_gemm"
    want, bound = wo.linear_reference(x, np.asarray(codes), np.asarray(scales), b)
    for route in ("native", "composed"):
        y = np.asarray(da.wq_linear(x, codes, scales, b, route=route))
        assert np.isfinite(y).all() and (np.abs(y - want) <= 2 * bound).all(), route


@pytest.mark.parametrize("kv_heads", [None, 2])
def test_generate_from_the_codes_alone(kv_heads):
    """Greedy generation from int8 weights on the two-block example model (kv_heads: grouped heads over an int8 cache): the
    eager ragged, captured and uniform ids agree; with every quantized float weight NaN the ids are the same, so none is read;
    the head's logits of the first decoding step lie within the derived bound of float64 over its kept inputs and codes."""
    ex = ts.load_example()
    np.random.seed(5)
    argv = ["--width", "64", "--heads", "4", "--seq", "16", "--vocab", "12"] + (["--kv-heads", "2"] if kv_heads else [])
    model, _ = ex.build(ex.parse(argv))
    b, p, n = 2, 4, 8
    prompt = np.random.RandomState(6).randint(0, 12, (b, p))
    gen.generate(model, prompt, 1, temperature=0.0)                # (every layer has seen a batch: its parameters exist)
    qw = gen.quantize_weights(model, "int8")
    assert len(qw.quantized) == 2 * 6 + 1 and not qw.kept and qw.nbytes()[0] < 0.27 * qw.nbytes()[1]

    def run(**kw):
        cache = gen.KVCache(p + n, quant="int8") if kv_heads else True
        return gen.generate(model, prompt, n, temperature=0.0, cache=cache, weights=qw, **kw)

    eager, captured, uniform = run(prompt_lens=np.full(b, p)), run(capture=True), run()
    assert np.array_equal(eager, captured) and np.array_equal(eager, uniform)

    layers, head = model.net.layers, [layer for layer in model.net.layers if isinstance(layer, Dense)][-1]
    model.set_phase("TEST")
    ops.WQ_ACTIVE = qw.activate()
    try:
        cache = gen.KVCache(p + n)
        gen._forward(layers, tn.Tensor(prompt), 0, cache)
        logits = np.asarray(gen._forward(layers, tn.Tensor(eager[:, p:p + 1]), p, cache).values)
    finally:
        ops.WQ_ACTIVE = None
        model.set_phase("TRAIN")
    codes, scales = qw.table[id(head.params["w"])]
    want, bound = wo.linear_reference(np.asarray(head.inputs.values), np.asarray(codes), np.asarray(scales),
                                      np.asarray(head.params["b"].values))
    assert head.inputs.shape[0] == b and (np.abs(logits.reshape(want.shape) - want) <= bound).all()

    for _, _, tensor in qw._owners:                                # (the scrub fixture zeroes them afterwards)
        tensor.values.fill(np.nan)
        UPLOADED.append(tensor.values)
    assert np.array_equal(run(), uniform) and np.array_equal(run(capture=True), uniform)
