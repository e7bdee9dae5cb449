"""Decoding on the CPU test twin, where everything takes the composed route: the raw calls within the oracle's bounds, the ops'
leaf results and argument checks, the layers' `cache` / `offset` arguments and their errors, a cached forward against the
uncached one, generate() with and without the cache against the fixture's tokens, and the example's --generate flag."""

import numpy as np
import pytest

import attn_oracle as ao
import decode_oracle as do
import decode_support as ds
import token_support as ts
import tinynn_autograd_amd as tn
from tinynn_autograd_amd import device_array as da, generation as gen
from tinynn_autograd_amd.core import ops
from tinynn_autograd_amd.core.layers import Embedding, MultiHeadAttention, TransformerBlock
from tinynn_autograd_amd.core.nn import Net
from tinynn_autograd_amd.core.tensor import Tensor


@pytest.fixture(scope="module")
def golden():
    return ds.load_golden()


@pytest.fixture(autouse=True)
def _switches():
    yield
    da.DECODE_ROUTE = None


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", sorted(do.DECODE_CASES))
def test_decode_attention_composed_within_the_bounds(golden, name, dtype):
    tn.set_default_float(dtype)
    case = do.decode_case(name, np.float32)
    res = ds.reference(case, dtype, 1)
    o, kc, vc = ds.run_decode("composed", case, dtype)
    assert o.dtype == dtype and o.shape == res.values["o"].shape and np.isfinite(o).all()
    ao.assert_within(o, golden["decode." + name], res.bounds["o"], "%s composed" % name)
    want_k, want_v = ds.expected_caches(case, dtype)
    assert np.array_equal(ds.bits(kc), ds.bits(want_k)) and np.array_equal(ds.bits(vc), ds.bits(want_v))


@pytest.mark.parametrize("name", sorted(do.SAMPLE_CASES))
def test_sampling_composed_equals_the_fixture(golden, name):
    x, temperature, top_k = do.sample_case(name, np.float32)
    for dtype in (np.float32, np.float64):
        tn.set_default_float(dtype)
        got = ds.run_sample("composed", x, golden["sample.%s.u" % name], temperature, top_k, dtype)
        assert np.array_equal(got, golden["sample.%s.ids" % name])
    assert np.array_equal(ds.run_sample("composed", x, None, 0.0, None, np.float32), np.argmax(x, axis=1))


def test_ops_give_leaves_and_refuse_unknown_arguments():
    case = do.decode_case("append_bthd", np.float32)
    q, kn, vn = (Tensor(case[n], requires_grad=True) for n in ("q", "k_new", "v_new"))
    kc, vc = tn.asarray(case["k_cache"]), tn.asarray(case["v_cache"])
    out = ops.attention_decode_(q, kc, vc, case["length"], kn, vn, route="composed")
    assert not out.requires_grad and out.dependency == [] and tuple(out.shape) == (2, 3, 24)
    res = ds.reference(case, np.float32, 1)
    ao.assert_within(np.asarray(out.values), res.values["o"], res.bounds["o"], "ops.attention_decode_")
    same = ops.attention_decode(case["q"], kc, vc, case["length"] + 1)               # the row is in the cache now
    ao.assert_within(np.asarray(same.values), res.values["o"], res.bounds["o"], "ops.attention_decode")
    ids = ops.sample_rows_(Tensor(np.array([[0.0, 5.0, 1.0]], dtype=np.float32), requires_grad=True), temperature=0.0)
    assert not ids.requires_grad and ids.dependency == [] and np.asarray(ids.values).tolist() == [1]
    assert np.asarray(ops.sample_rows(np.array([[0.0, 5.0, 1.0]], dtype=np.float32), [0.0], top_k=1).values).tolist() == [1]
    for call in (lambda: ops.attention_decode_(q, kc, vc, 3, kn, vn, causal=True), lambda: ops.attention_decode(case["q"], kc, vc, 3, mask=1),
                 lambda: ops.sample_rows_(q, top_p=0.9), lambda: ops.sample_rows(case["q"], top_p=0.9)):
        with pytest.raises(TypeError, match="unsupported arguments"):
            call()
    with pytest.raises(ValueError, match="come together"):
        da.attention_decode(q.values, kc, vc, 3, k_new=kn.values)
    with pytest.raises(TypeError, match="written in place"):
        da.attention_decode(q.values, case["k_cache"], vc, 3)                       # a host array would be copied
    with pytest.raises(ValueError, match="u is needed"):
        da.sample_rows(q.values.reshape(6, 16), None, temperature=1.0)


def test_embedding_offset():
    rs = np.random.RandomState(3)
    layer = Embedding(7, 4, max_len=6)
    ids = rs.randint(0, 7, (2, 6))
    whole = np.asarray(layer.forward(Tensor(ids)).values)
    for offset, t in ((0, 6), (2, 3), (5, 1)):
        part = np.asarray(layer.forward(Tensor(ids[:, offset:offset + t]), offset=offset).values)
        assert np.array_equal(part, whole[:, offset:offset + t])                    # bit for bit: the same rows added
    with pytest.raises(ValueError, match="at offset 5 exceed max_len 6"):
        layer.forward(Tensor(ids[:, :2]), offset=5)
    with pytest.raises(ValueError, match="offset must be >= 0"):
        layer.forward(Tensor(ids[:, :2]), offset=-1)
    free = Embedding(7, 4)                                                           # no positions: the offset changes nothing
    assert np.array_equal(np.asarray(free.forward(Tensor(ids), offset=3).values), np.asarray(free.forward(Tensor(ids)).values))


def test_layer_cache_errors():
    x = Tensor(np.random.RandomState(0).randn(2, 3, 8).astype(np.float32))
    with pytest.raises(ValueError, match="needs causal=True"):
        MultiHeadAttention(2, num_in=8).forward(x, cache=gen.LayerCache(4))
    with pytest.raises(ValueError, match="needs causal=True"):
        TransformerBlock(2, num_in=8).forward(x, cache=gen.LayerCache(4))
    layer = MultiHeadAttention(2, num_in=8, causal=True)
    with pytest.raises(ValueError, match="a prompt of 3 tokens exceeds the cache's 2 rows"):
        layer.forward(x, cache=gen.LayerCache(2))
    cache = gen.LayerCache(4)
    layer.forward(x, cache=cache)
    assert cache.length == 3 and tuple(cache.k.shape) == (2, 4, 2, 4)
    with pytest.raises(ValueError, match="ONE new token"):
        layer.forward(x, cache=cache)
    one = Tensor(np.zeros((2, 1, 8), dtype=np.float32))
    layer.forward(one, cache=cache)
    assert cache.length == 4
    before = np.asarray(cache.k).copy()
    with pytest.raises(ValueError, match="the cache is full"):
        layer.forward(one, cache=cache)
    assert cache.length == 4 and np.array_equal(np.asarray(cache.k), before)         # raised before any launch
    with pytest.raises(ValueError, match="allocated for"):
        small = gen.LayerCache(6)
        layer.forward(x, cache=small)
        layer.forward(Tensor(np.zeros((1, 1, 8), dtype=np.float32)), cache=small)
    with pytest.raises(ValueError, match="max_len must be >= 1"):
        gen.KVCache(0)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_cached_forward_equals_the_uncached_last_rows(golden, dtype):
    """Prefill of 4 tokens + 8 decoding steps of the fixture's model: the logits of every step within 4 logit bounds of the
    float64 oracle's (the reference's own float32 discrepancy, tests/gen_decode_golden.py; the factor 4 because the
    summation orders differ, as in tests/gen_token_golden.py) on BOTH paths — the cached one row and the last row of the
    uncached forward over the whole prefix.  Two logits of one path then move by at most 8 bounds against each other: the
    fixture's top-2 margin exceeds that (asserted here), so neither path can change a token."""
    tn.set_default_float(dtype)
    bound = do.MARGIN * float(golden["lm.logit_bound"]) if dtype == np.float32 else 1e-11
    steps = do.lm_generate(do.lm_params(float(golden["lm.head_scale"])), do.lm_prompt(), do.LM_NEW)[1]
    assert do.top2_margin(steps) > 2 * do.MARGIN * float(golden["lm.logit_bound"])
    net = ds.lm_net(golden, True, dtype)
    net.set_phase("TEST")
    ids = golden["lm.ids"]
    params = do.lm_params(float(golden["lm.head_scale"]))
    cache = gen.KVCache(ids.shape[1])
    v = do.to.LM_CASE["V"]
    for n in range(do.LM_NEW):
        upto = do.LM_PROMPT + n
        want = do.lm_logits(params, ids[:, :upto])[:, -1]
        if n == 0:
            step = gen._forward(net.layers, Tensor(ids[:, :upto]), 0, cache)
        else:
            step = gen._forward(net.layers, Tensor(ids[:, upto - 1:upto]), upto - 1, cache)
        full = gen._forward(net.layers, Tensor(ids[:, :upto]), 0, None)
        got_c = np.asarray(step.values, dtype=np.float64).reshape(3, -1, v)[:, -1]
        got_f = np.asarray(full.values, dtype=np.float64).reshape(3, -1, v)[:, -1]
        assert np.abs(got_c - want).max() <= bound, "cached, step %d: %.3e" % (n, np.abs(got_c - want).max())
        assert np.abs(got_f - want).max() <= bound, "uncached, step %d: %.3e" % (n, np.abs(got_f - want).max())
        assert cache.length == upto


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("fused", [True, False])
def test_generate_gives_the_fixtures_tokens(golden, fused, dtype):
    tn.set_default_float(dtype)
    net = ds.lm_net(golden, fused, dtype)
    prompt = do.lm_prompt()
    for cache in (True, False):
        out = gen.generate(net, prompt, do.LM_NEW, temperature=0.0, cache=cache)
        assert out.dtype == np.int64 and np.array_equal(out, golden["lm.ids"]), "cache=%s" % cache
    assert net.get_phase() == "TRAIN"                                                # restored
    net.set_phase("TEST")
    assert np.array_equal(gen.generate(net, tn.asarray(prompt), 2, temperature=0.0), golden["lm.ids"][:, :do.LM_PROMPT + 2])
    assert net.get_phase() == "TEST"


def test_generate_arguments(golden):
    net = ds.lm_net(golden, True, np.float32)
    prompt = do.lm_prompt()
    assert np.array_equal(gen.generate(net, prompt, 0), prompt)
    with pytest.raises(ValueError, match="exceed the embedding's max_len 12"):
        gen.generate(net, prompt, 9)
    with pytest.raises(ValueError, match="integers"):
        gen.generate(net, prompt.astype(np.float32), 2)
    with pytest.raises(ValueError, match="u must be"):
        gen.generate(net, prompt, 2, u=np.zeros((3, 2)))
    with pytest.raises(ValueError, match="u must be"):
        gen.generate(net, prompt, 2, u=np.ones((2, 3)))
    u = np.random.RandomState(7).random_sample((3, 3))
    a = gen.generate(net, prompt, 3, temperature=0.8, top_k=4, u=u)
    assert a.shape == (3, 7) and np.array_equal(a[:, :4], prompt) and ((a >= 0) & (a < 11)).all()
    assert np.array_equal(gen.generate(net, prompt, 3, temperature=0.8, top_k=4, seed=7), a)       # the same draw
    assert np.array_equal(gen.generate(net, prompt, 3, temperature=0.8, top_k=1, u=u),
                          gen.generate(net, prompt, 3, temperature=0.0))                            # top-1 is greedy
    assert net.get_phase() == "TRAIN"


def test_example_generates():
    """examples/charlm_run.py --generate: trains briefly, continues the first test sequences greedily; the ids are in range
    and the share of motif continuations is a fraction."""
    example = ts.load_example()
    args = example.parse(["--n_train", "64", "--n_test", "8", "--num_ep", "1", "--batch_size", "32", "--generate", "4"])
    history = example.main(args)
    generated, share = args.generation
    assert len(history) == 1 and generated.shape == (8, 2 * 4 + 4) and generated.dtype == np.int64
    assert ((generated >= 0) & (generated < 16)).all() and 0.0 <= share <= 1.0
    plain = example.parse(["--n_train", "32", "--n_test", "8", "--num_ep", "1", "--batch_size", "32"])
    assert len(example.main(plain)) == 1 and plain.generation is None
