"""TEST INFRASTRUCTURE shared by the extend tests on the CPU twin and on the MI355X: cases from a seed, one raw call of one
route as numpy arrays (with poisoned dead rows and at unaligned addresses, as decode_support.py), what the caches must hold
afterwards, and a recorder of the attention calls a layer makes."""

import os

import numpy as np

import extend_oracle as eo
from decode_support import bits, poisoned                       # noqa: F401  (re-exported)
from norm_support import dev
from tinynn_autograd_amd import device_array as da

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "extend_cases.npz")


def load_golden():
    with np.load(GOLDEN) as data:
        return dict(data)


def make_case(seed, layout, b, h, hkv, tmax, length, t, d, dv, dtype=np.float32, scale=None):
    q, kc, vc, kn, vn = eo.extend_inputs(np.random.RandomState(seed), layout, b, h, hkv, tmax, t, d, dv, dtype)
    return dict(q=q, k_cache=kc, v_cache=vc, length=length, k_new=kn, v_new=vn, layout=layout, scale=scale)


def device_caches(case, dtype, unaligned=False, poison=True):
    """The caches on the device; poison: every row from `length` on (the rows about to be appended included) holds NaN."""
    layout, length = case["layout"], case["length"]
    kc, vc = (poisoned(case[n], layout, length, dtype) if poison else np.asarray(case[n], dtype=dtype) for n in ("k_cache", "v_cache"))
    return dev(kc, dtype, unaligned), dev(vc, dtype, unaligned)


def run_extend(route, case, dtype, unaligned=False, poison=True, caches=None):
    """One raw call of one route -> (o, k_cache, v_cache) as numpy arrays, the caches AFTER the call.  caches: device arrays
    to go on with (a sequence of calls that appends chunk after chunk), else made from the case."""
    kd, vd = caches if caches is not None else device_caches(case, dtype, unaligned, poison)
    qd, kn, vn = (dev(case[n], dtype, unaligned) for n in ("q", "k_new", "v_new"))
    o = da.attention_extend(qd, kd, vd, case["length"], kn, vn, scale=case.get("scale"), layout=case["layout"], route=route)
    return np.asarray(o), np.asarray(kd), np.asarray(vd)


def expected_caches(case, dtype, poison=True):
    """What the caches must hold after the call, bit for bit: rows [length, length + T) replaced, nothing else touched."""
    layout, length = case["layout"], case["length"]
    kc, vc = (poisoned(case[n], layout, length, dtype) if poison else np.asarray(case[n], dtype=dtype) for n in ("k_cache", "v_cache"))
    return (eo.put_rows(kc, layout, length, np.asarray(case["k_new"], dtype=dtype)),
            eo.put_rows(vc, layout, length, np.asarray(case["v_new"], dtype=dtype)))


def reference(case, dtype):
    return eo.extend_reference(case["q"], case["k_cache"], case["v_cache"], case["length"], case["k_new"], case["v_new"],
                               case.get("scale"), case["layout"], dtype)


def chunk(case, start, stop, length):
    """Rows [start, stop) of the case's new rows as a case of their own at `length` cached rows."""
    cut = lambda x: np.ascontiguousarray(eo.rows_of(x, case["layout"], start, stop))
    return dict(case, q=cut(case["q"]), k_new=cut(case["k_new"]), v_new=cut(case["v_new"]), length=length)


def run_chunks(route, case, dtype, cuts):
    """The case's T rows as a sequence of calls of cuts[0], cuts[1], ... rows that append to ONE pair of caches ->
    (o of all rows, k_cache, v_cache)."""
    assert sum(cuts) == case["q"].shape[eo.AXES[case["layout"]][0]]
    caches = device_caches(case, dtype)
    outs, done = [], 0
    for c in cuts:
        o, _, _ = run_extend(route, chunk(case, done, done + c, case["length"] + done), dtype, caches=caches)
        outs.append(o)
        done += c
    return np.concatenate(outs, axis=eo.AXES[case["layout"]][0]), np.asarray(caches[0]), np.asarray(caches[1])


# ---------------------------------------------------------------------- layers and the fixture's language model
def record_attention(monkeypatch):
    """Wrap the attention ops a layer may call; returns {op name: [(numpy operands, keyword arguments, numpy result)]}."""
    from tinynn_autograd_amd.core import ops
    seen = {}
    host = lambda a: np.array(np.asarray(getattr(a, "values", a)))
    for name in ("attention_", "attention_gqa_", "attention_extend_", "attention_decode_", "attention_decode_gqa_"):
        real = getattr(ops, name)

        def call(*args, _real=real, _name=name, **kw):
            before = [host(a) if hasattr(a, "shape") else a for a in args]
            out = _real(*args, **kw)
            seen.setdefault(_name, []).append((before, kw, host(out)))
            return out
        monkeypatch.setattr(ops, name, call)
    return seen


def build_layer(kind, fused, kv_heads, rope, rows, dtype, width=16, heads=4):
    import tinynn_autograd_amd as tn
    from tinynn_autograd_amd.core.layers import MultiHeadAttention, TransformerBlock
    from tinynn_autograd_amd.rope import Rotary
    tn.set_default_float(dtype)
    np.random.seed(11)                                         # the initializers draw from the host generator
    rotary = Rotary(rows) if rope else None
    if kind == "mha":
        return MultiHeadAttention(heads, num_in=width, causal=True, fused=fused, kv_heads=kv_heads, rope=rotary)
    return TransformerBlock(heads, hidden=2 * width, num_in=width, causal=True, fused=fused, kv_heads=kv_heads, rope=rotary)


def check_layer(monkeypatch, kind, fused, kv_heads, rope, dtype, p1=5, p2=7, batch=2):
    """A prefill of p1 rows followed by an extension of p2 rows against ONE prefill of p1 + p2 rows of the same layer:
      * the caches agree bit for bit (the projections are row-wise and the extension appends what it is given);
      * the layer made ONE ops.attention_extend_ call at length p1 whose result lies within the oracle's bounds on the
        operands it was given;
      * its q rows are bit for bit the single prefill's, so both attention results lie within the bound of one reference:
        the last p2 positions of the two differ by at most twice the bound;
      * (MultiHeadAttention) the layer outputs of those positions differ by at most that, carried through |wo|, plus the
        rounding of the output projection in either path: (E + 2) u (|att| |wo| + |bo|) each."""
    import attn_oracle as ao
    from tinynn_autograd_amd import generation as gen
    from tinynn_autograd_amd.core.tensor import Tensor
    rows = p1 + p2
    layer = build_layer(kind, fused, kv_heads, rope, rows, dtype)
    layer.set_phase("TEST")
    x = np.random.RandomState(5).randn(batch, rows, 16).astype(dtype)
    seen = record_attention(monkeypatch)
    whole_cache = gen.LayerCache(rows)
    whole = np.asarray(layer.forward(Tensor(x), cache=whole_cache).values)
    cache = gen.LayerCache(rows, extend=True)
    pre = np.asarray(layer.forward(Tensor(x[:, :p1]), cache=cache).values)
    assert cache.length == p1 and pre.shape == (batch, p1, 16)
    ext = np.asarray(layer.forward(Tensor(x[:, p1:]), cache=cache).values)
    assert cache.length == rows and ext.shape == (batch, p2, 16) and np.isfinite(ext).all()
    for mine, theirs in ((cache.k, whole_cache.k), (cache.v, whole_cache.v)):
        assert np.array_equal(bits(np.asarray(mine)), bits(np.asarray(theirs)))
    assert len(seen["attention_extend_"]) == 1 and not seen.get("attention_decode_") and not seen.get("attention_decode_gqa_")
    (q, kc, vc, length, kn, vn), kw, att = seen["attention_extend_"][0]
    assert length == p1 and kw["layout"] == "bthd" and kc.shape[2] == (kv_heads or 4)
    res = eo.extend_reference(q, kc, vc, p1, kn, vn, None, "bthd", dtype)
    ao.assert_within(att, res.values["o"], res.bounds["o"], "%s extension" % kind)
    first = seen["attention_gqa_" if kv_heads else "attention_"][0]
    assert np.array_equal(bits(first[0][0][:, p1:]), bits(q))
    assert (np.abs(first[2][:, p1:].astype(np.float64) - att) <= 2 * res.bounds["o"]).all()
    if kind == "mha":
        u = eo.unit(dtype)
        wo, bo = (np.abs(np.asarray(layer.params[n].values, dtype=np.float64)) for n in ("wo", "bo"))
        flat = lambda a: np.asarray(a, dtype=np.float64).reshape(batch * p2, 16)
        bound = 2 * flat(res.bounds["o"]) @ wo + 2 * (16 + 2) * u * (np.abs(flat(res.values["o"])) @ wo + bo)
        assert (np.abs(flat(ext) - flat(whole[:, p1:])) <= bound).all()
    return layer


def check_model_logits(golden, fused, dtype):
    """The fixture's language model (decode_support.lm_net): a prefill of 4 tokens and an extension of 7 through a
    KVCache(extend=True) give the logits of positions 4 .. 10 within MARGIN logit bounds of the float64 oracle's — the
    criterion of tests/test_decode_host.py's cached forward, on the same positions."""
    import decode_oracle as do
    import decode_support as ds
    import tinynn_autograd_amd as tn
    from tinynn_autograd_amd import generation as gen
    from tinynn_autograd_amd.core.tensor import Tensor
    tn.set_default_float(dtype)
    bound = do.MARGIN * float(golden["lm.logit_bound"]) if dtype == np.float32 else 1e-11
    net = ds.lm_net(golden, fused, dtype)
    net.set_phase("TEST")
    ids = golden["lm.ids"][:, :11]
    want = do.lm_logits(do.lm_params(float(golden["lm.head_scale"])), ids)
    cache = gen.KVCache(11, extend=True)
    v = want.shape[-1]
    pre = np.asarray(gen._forward(net.layers, Tensor(ids[:, :4]), 0, cache).values, dtype=np.float64).reshape(3, 4, v)
    ext = np.asarray(gen._forward(net.layers, Tensor(ids[:, 4:]), 4, cache).values, dtype=np.float64).reshape(3, 7, v)
    assert cache.length == 11
    assert np.abs(pre - want[:, :4]).max() <= bound and np.abs(ext - want[:, 4:]).max() <= bound, np.abs(ext - want[:, 4:]).max()


def check_generate(golden, fused, dtype):
    """Greedy generation on the fixture model, whose top-2 margin exceeds the logit bounds at every step: prefill_chunk in
    {1, 3, P} and a two-turn continuation through a kept KVCache(extend=True) give the tokens of the plain call."""
    import decode_oracle as do
    import decode_support as ds
    import tinynn_autograd_amd as tn
    from tinynn_autograd_amd import generation as gen
    tn.set_default_float(dtype)
    net = ds.lm_net(golden, fused, dtype)
    prompt, ids = do.lm_prompt(), golden["lm.ids"]
    plain = gen.generate(net, prompt, do.LM_NEW, temperature=0.0)
    assert np.array_equal(plain, ids)
    for c in (1, 3, do.LM_PROMPT):
        assert np.array_equal(gen.generate(net, prompt, do.LM_NEW, temperature=0.0, prefill_chunk=c), plain), c
    # two turns: 4 + 3 tokens, then the last token and the fixture's next two as the new prompt, 3 more — the tokens of ONE
    # call on the concatenated prompt (every step's logits are the fixture's own)
    kept = gen.KVCache(12, extend=True)
    one = gen.generate(net, prompt, 3, temperature=0.0, cache=kept)
    assert np.array_equal(one, ids[:, :7]) and kept.length == 6
    k_before = kept.layer(1).k
    two = gen.generate(net, ids[:, 6:9], 3, temperature=0.0, cache=kept)
    assert two.shape == (3, 6) and np.array_equal(two, ids[:, 6:12]) and kept.length == 11
    assert kept.layer(1).k is k_before                                                # nothing new was allocated
    assert np.array_equal(gen.generate(net, ids[:, :9], 3, temperature=0.0), ids)
    three = gen.generate(net, ids[:, 6:9], 3, temperature=0.0, cache=gen.KVCache(12, extend=True), prefill_chunk=2)
    assert three.shape == (3, 6)                                                      # an empty instance behaves as cache=True
    assert net.get_phase() == "TRAIN"
