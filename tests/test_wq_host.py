"""The int8 weight-only linear layer on the host side (wq.py, the composed route, generate(weights=)): the format's properties
on quantize_host, the planner's routes, lane groups and split ranges, and generation from the codes under the CPU twin."""

import numpy as np
import pytest

import token_support as ts
import wq_oracle as wo
from tinynn_autograd_amd import device_array as da, generation as gen, wq


@pytest.mark.parametrize("k, n", [(4, 4), (8, 12), (260, 64), (64, 260)])
def test_quantize_host_keeps_the_formats_properties(k, n):
    rs = np.random.RandomState(k + n)
    w = (rs.randn(k, n) * np.exp(rs.randn(1, n) * 3)).astype(np.float32)
    w[:, 1] = 0.0
    w[1:, 2] = 0.0                                                # one non-zero: code +-127 exactly
    codes, scales = wq.quantize_host(w)
    wo.check_weight(w, codes, scales, "quantize_host %d x %d" % (k, n))
    assert abs(int(wq.unpack_codes(codes)[0, 2])) == 127
    assert codes[1 // 4, 3, 1 % 4] == wq.unpack_codes(codes).view(np.uint8)[1, 3]         # [kb, n, j] is w[4 kb + j, n]
    back = wq.dequantize_host(codes, scales)
    assert back.dtype == np.float64 and (np.abs(back - w) <= scales.astype(np.float64)[None, :] / 2).all()
    again, _ = wq.quantize_host(back.astype(np.float32))          # the round trip is a fixed point
    assert np.array_equal(again, codes)


def test_planner_routes_groups_and_split_ranges():
    for n, group in ((4, 1), (12, 4), (64, 16), (256, 64), (260, 64), (516, 64)):
        p = wq.plan_linear((3, 64), wq.codes_shape(64, n), (n,), (1, n))
        assert (p.route, p.kernel, p.rows, p.group, p.panels) == ("native", "linear", 4, group, -(-n // 256)), p
        assert wq.pass_blocks(n) == 16 * 64 // group
    assert [wq.plan_linear((m, 8), (2, 4, 4), (4,)).rows for m in (1, 2, 3, 5, 8, 16)] == [1, 2, 4, 8, 8, 16]
    big = wq.plan_linear((17, 8), (2, 4, 4), (4,))
    assert (big.route, big.kernel, big.splits, big.workspace_bytes()) == ("native", "dequant_gemm", 1, 0)
    for kw in (dict(native=False), dict(float_ok=False), dict(aligned=False)):
        assert wq.plan_linear((1, 8), (2, 4, 4), (4,), **kw).kernel == "dequant_gemm"
        with pytest.raises(ValueError, match="native int8 linear route needs"):
            wq.plan_linear((1, 8), (2, 4, 4), (4,), route="native", **kw)
    # the split: contiguous runs that cover every k-block once, as many as the extents allow, never more than MAX_SPLITS
    for k in (4, 8, 60, 68, 4096):
        most = wq.most_splits(k)
        assert most == min(k // 4, wq.MAX_SPLITS) and 1 <= wq.choose_splits(1, k, 4096) <= most
        for splits in (1, most):
            runs = [wq.split_range(k, splits, s) for s in range(splits)]
            assert runs[0][0] == 0 and runs[-1][1] == k // 4 and all(a[1] == b[0] and a[0] < a[1] for a, b in zip(runs, runs[1:]))
    assert wq.plan_linear((2, 8), (2, 8, 4), (8,), splits=2).workspace_bytes() == 2 * 2 * 8 * 4
    with pytest.raises(ValueError, match=r"splits 3 outside \[1, 2\]"):
        wq.plan_linear((2, 8), (2, 8, 4), (8,), splits=3)
    # a weight the format does not fit keeps its float values
    assert [wq.plan_weight(s) for s in ((64, 64), (64, 13), (6, 64), (64,))] == ["int8", "float", "float", "float"]
    with pytest.raises(ValueError, match="multiples of 4"):
        wq.codes_shape(6, 64)


@pytest.mark.parametrize("m", [3, 17])
def test_composed_linear_against_float64(m):
    rs = np.random.RandomState(m)
    w, x, b = (rs.randn(*s).astype(np.float32) for s in ((40, 12), (m, 40), (1, 12)))
    codes, scales = da.wq_quantize(w)
    wo.check_weight(w, np.asarray(codes), np.asarray(scales))
    want, bound = wo.linear_reference(x, np.asarray(codes), np.asarray(scales), b)
    y = np.asarray(da.wq_linear(x, codes, scales, b, route="composed"))
    # (the composed product multiplies by the DEQUANTIZED float32 weight: one rounding per term more than the bound counts)
    assert y.dtype == np.float32 and (np.abs(y - want) <= 2 * bound).all()


def test_generate_from_int8_weights_equals_the_dequantized_model():
    ex = ts.load_example()
    np.random.seed(3)
    argv = ["--width", "32", "--heads", "2", "--kv-heads", "1", "--seq", "12", "--vocab", "11"]
    model, _ = ex.build(ex.parse(argv))
    prompt = np.random.RandomState(4).randint(0, 11, (2, 4))
    gen.generate(model, prompt, 1, temperature=0.0)               # (every layer has seen a batch: its parameters exist)
    qw = gen.quantize_weights(model, "int8")
    names = [name for name, _ in qw.quantized]
    assert "1.attn.wq" in names and "1.fc1.w" in names and "1.fc2.w" in names and len(names) == 2 * 6
    assert any(name.endswith(".w") and shape == (32, 11) for name, shape, _ in qw.kept)        # the head: N = 11 does not fit
    ids = gen.generate(model, prompt, 5, temperature=0.0, weights=qw)
    assert np.array_equal(ids, gen.generate(model, prompt, 5, temperature=0.0, weights="int8"))
    both = gen.generate(model, prompt, 5, temperature=0.0, weights=qw, cache=gen.KVCache(9, quant="int8"))
    assert both.shape == (2, 9) and np.array_equal(both[:, :5], ids[:, :5])      # (the first new token comes from the prefill)
    for (_, _, tensor), (codes, scales) in zip(qw._owners, qw.table.values()):
        tensor.values[...] = da.wq_dequantize(codes, scales)
    assert np.array_equal(ids, gen.generate(model, prompt, 5, temperature=0.0))
    with pytest.raises(ValueError, match="QuantizedWeights of THIS model"):
        gen.generate(ex.build(ex.parse(argv))[0], prompt, 5, weights=qw)
    with pytest.raises(ValueError, match="quant must be one of"):
        gen.quantize_weights(model, "int4")
