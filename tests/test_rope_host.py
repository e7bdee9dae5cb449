"""The rotary position embedding above the kernel — the device_array route, the graph nodes and wrappers,
MultiHeadAttention(rope=) and TransformerBlock(rope=), generation — on the backend of the session (the CPU test twin runs the
composed route): results inside the oracle's derived bounds (tests/rope_oracle.py), the vjps, the round trip, rope=None
bit for bit and call for call, the language model's tokens, and the max_len refusals before any launch.

Gradient through rope and attention (test_gradients_through_rope_and_attention): the summed bounds of the parts.  With qr, kr
the DEVICE's rotated operands, gqa_oracle gives the float64 gradients g64 of the attention against them and their bound
b_attn; the device's dq is the inverse rotation, evaluated in the operand dtype, of a gradient within b_attn of g64, so
    |dq - inv64(g64)| <= rope_bound(g64) + propagate(b_attn) (1 + 2^-20)
(the last factor covers the rotation bound being taken at g64 instead of at the device's own intermediate gradient)."""

import numpy as np
import pytest

import dropout_support as dsu
import gqa_oracle as go
import rope_oracle as ro
import rope_support as rsup
import tinynn_autograd_amd as tn
from tinynn_autograd_amd import _lib, device_array as da, generation as gen, rope as rp
from tinynn_autograd_amd.core import ops
from tinynn_autograd_amd.core.layers import MultiHeadAttention, TransformerBlock
from tinynn_autograd_amd.core.tensor import Tensor

DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def golden():
    return rsup.load_golden()


def test_the_session_route():
    lib = _lib.get()
    rot = rp.Rotary(8)
    plan = rp.plan_rope((1, 2, 2, 4), None, None, rot.max_len, native=lib.has_rope)
    assert plan.route == ("native" if lib.has_rope else "composed")
    if tn.backend_name() != "hip-gfx950":
        assert plan.route == "composed"
    assert da.ROPE_ROUTE is None


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pairing", ro.PAIRINGS)
@pytest.mark.parametrize("name", sorted(ro.CASES))
def test_composed_route_within_the_bounds(golden, name, pairing, dtype):
    """Both layouts, forward and inverse, fresh and in place; the float32 forward also against the fixture's values."""
    R = ro.CASES[name][5]
    rot = rsup.rotary(R, pairing)
    for layout in ro.LAYOUTS:
        xa, xb = ro.case_input(name, dtype, layout)
        for inverse in (False, True):
            ya, yb = rsup.run("composed", xa, xb, rot, dtype, ro.GOLDEN_OFFSET, None, layout, inverse)
            ra, rb = rsup.references(xa, xb, rot, dtype, ro.GOLDEN_OFFSET, None, layout, inverse)
            ro.assert_within(ya, ra, "%s %s a" % (name, layout))
            if xb is not None:
                ro.assert_within(yb, rb, "%s %s b" % (name, layout))
            ia, ib = rsup.run("composed", xa, xb, rot, dtype, ro.GOLDEN_OFFSET, None, layout, inverse, inplace=True)
            assert np.array_equal(rsup.bits(ia), rsup.bits(ya)) and (xb is None or np.array_equal(rsup.bits(ib), rsup.bits(yb)))
        if layout == "bthd" and dtype == np.float32:
            want = golden["%s.%s.a" % (pairing, name)]
            ya, _ = rsup.run("composed", xa, xb, rot, dtype, ro.GOLDEN_OFFSET, None, layout, False)
            fwd, _ = rsup.references(xa, xb, rot, dtype, ro.GOLDEN_OFFSET, None, layout, False)
            assert (np.abs(ya - want) <= fwd.bounds * (1 + 2.0 ** -20)).all()      # (the fixture is the oracle rounded to float64)


@pytest.mark.parametrize("dtype", DTYPES)
def test_device_positions_on_the_composed_route(dtype):
    rot = rsup.rotary(4, "half", 16)
    xa, xb = ro.case_input("aligned_tail", dtype)                          # (3, 1, 4, 2, 16, 8): T == 1
    rot8 = rsup.rotary(8, "interleaved", 16)
    for r in (rot, rot8):
        positions = [0, 15, 5]
        ya, yb = rsup.run("composed", xa, xb, r, dtype, positions=positions)
        ra, rb = rsup.references(xa, xb, r, dtype, positions=positions)
        ro.assert_within(ya, ra, "positions a")
        ro.assert_within(yb, rb, "positions b")
        for b, p in enumerate(positions):
            oa, ob = rsup.run("composed", xa[b:b + 1], xb[b:b + 1], r, dtype, offset=p)
            assert np.array_equal(rsup.bits(ya[b:b + 1]), rsup.bits(oa)) and np.array_equal(rsup.bits(yb[b:b + 1]), rsup.bits(ob))
        ya, yb = rsup.run("composed", xa, xb, r, dtype, positions=[-1, 16, 2])
        assert not ya[:2].any() and not yb[:2].any()
        ra, _ = rsup.references(xa, xb, r, dtype, positions=[-1, 16, 2])
        ro.assert_within(ya, ra, "bad positions")
        ia, _ = rsup.run("composed", xa, xb, r, dtype, positions=[-1, 16, 2], inplace=True)
        assert np.array_equal(rsup.bits(ia), rsup.bits(ya))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pairing", ro.PAIRINGS)
def test_nodes_vjps_and_the_round_trip(pairing, dtype):
    tn.set_default_float(dtype)
    rot = rsup.rotary(6, pairing, 32)
    rs = np.random.RandomState(ro.case_seed("nodes" + pairing))
    q, k = rs.randn(2, 5, 3, 9).astype(dtype), rs.randn(2, 5, 1, 9).astype(dtype)
    gq, gk = rs.randn(*q.shape).astype(dtype), rs.randn(*k.shape).astype(dtype)
    cos_t, sin_t = rot.host_tables(6, dtype)
    qt, kt = (Tensor(a, requires_grad=True, dtype=dtype) for a in (q, k))
    qr, kr = ops.rope_(qt, kt, rotary=rot, offset=3)
    for got, x in ((qr, q), (kr, k)):
        ro.assert_within(np.asarray(got.values), ro.reference(x, cos_t, sin_t, 3, None, "bthd", pairing, False, dtype), "forward")
    (qr * Tensor(gq, dtype=dtype)).sum().backward()
    (kr * Tensor(gk, dtype=dtype)).sum().backward()
    for t, g in ((qt, gq), (kt, gk)):                                    # the vjp is the inverse rotation of the gradient
        ro.assert_within(np.asarray(t.grad), ro.reference(g, cos_t, sin_t, 3, None, "bthd", pairing, True, dtype), "vjp")
    single = ops.rope(q, rotary=rot, offset=3)
    assert np.array_equal(rsup.bits(np.asarray(single.values)), rsup.bits(np.asarray(qr.values)))
    back = ops.rope_(Tensor(np.asarray(qr.values), dtype=dtype), rotary=rot, offset=3, inverse=True)
    ro.roundtrip(q, np.asarray(qr.values), np.asarray(back.values), cos_t, sin_t, 3, "bthd", pairing, dtype, "node")
    # inverse=True nodes: the vjp is the forward rotation
    qi = Tensor(q, requires_grad=True, dtype=dtype)
    (ops.rope_(qi, rotary=rot, offset=3, inverse=True) * Tensor(gq, dtype=dtype)).sum().backward()
    ro.assert_within(np.asarray(qi.grad), ro.reference(gq, cos_t, sin_t, 3, None, "bthd", pairing, False, dtype), "vjp of inverse")
    # device positions: inference only, leaves without a grad_fn
    q1 = Tensor(q[:, :1], requires_grad=True, dtype=dtype)
    out = ops.rope_(q1, rotary=rot, positions=da.lengths([4, 31]))
    assert not out.requires_grad
    ro.assert_within(np.asarray(out.values), ro.reference(q[:, :1], cos_t, sin_t, 0, [4, 31], "bthd", pairing, False, dtype), "pos")


def test_rejected_arguments():
    rot = rp.Rotary(8)
    x = Tensor(np.zeros((1, 2, 1, 4), dtype=np.float32))
    with pytest.raises(TypeError, match="unsupported arguments"):
        ops.rope_(x, rotary=rot, scaling=2.0)
    with pytest.raises(TypeError, match="unsupported arguments"):
        ops.rope(x, rotary=rot, ntk=True)
    with pytest.raises(ValueError, match="rotary="):
        ops.rope_(x)
    with pytest.raises(ValueError, match="lie outside the table"):
        ops.rope_(x, rotary=rot, offset=7)
    with pytest.raises(ValueError, match="device positions need T == 1"):
        ops.rope_(x, rotary=rot, positions=da.lengths([0]))
    with pytest.raises(ValueError, match="agree in B, T and D"):
        ops.rope_(x, Tensor(np.zeros((1, 3, 1, 4), dtype=np.float32)), rotary=rot)
    with pytest.raises(ValueError, match="four axes|operands are"):
        ops.rope_(Tensor(np.zeros((2, 4), dtype=np.float32)), rotary=rot)
    xd = tn.asarray(np.zeros((1, 2, 1, 4), dtype=np.float32))
    with pytest.raises(ValueError, match="two tensors overlap"):
        da.rope(xd, xd, rotary=rot, out=(tn.zeros((1, 2, 1, 4)), xd))
    with pytest.raises(ValueError, match="out must be"):
        da.rope(xd, rotary=rot, out="here")
    with pytest.raises(ValueError, match="blocks must be"):
        da.rope(xd, rotary=rot, blocks=rp.MAX_BLOCKS + 1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gradients_through_rope_and_attention(dtype):
    route = None
    rs = np.random.RandomState(ro.case_seed("rope+attention"))
    q, k, v, do_ = go.make_inputs(rs, 2, 4, 2, 9, 9, 8, 8, dtype, q_amp=2.0)
    rot = rsup.rotary(8, "half", 16)
    dq, dk, qr, kr = rsup.attention_grads(route, q, k, v, do_, rot, dtype)
    cos_t, sin_t = rot.host_tables(8, dtype)
    for got, x in ((qr, q), (kr, k)):
        ro.assert_within(got, ro.reference(x, cos_t, sin_t, 0, None, "bthd", "half", False, dtype), "rotated operand")
    res = go.reference(qr, kr, v, do_, True, None, dtype)
    for name, got in (("dq", dq), ("dk", dk)):
        inv = ro.reference(res.values[name], cos_t.astype(np.float64), sin_t.astype(np.float64), 0, None, "bthd", "half", True, dtype)
        total = inv.bounds + ro.propagate(res.bounds[name], cos_t, sin_t, 0, "bthd", "half") * (1 + 2.0 ** -20)
        err = np.abs(got.astype(np.longdouble) - inv.values).astype(np.float64)
        print("%s %s: worst error / bound %.3f" % (name, np.dtype(dtype).name, float((err / total).max())))
        assert (err <= total).all(), name


def _built(kind, **kw):
    np.random.seed(3)
    if kind == "mha":
        return MultiHeadAttention(4, num_in=16, causal=True, kv_heads=2, **kw)
    return TransformerBlock(4, hidden=32, num_in=16, causal=True, kv_heads=2, **kw)


@pytest.mark.parametrize("kind", ["mha", "block"])
def test_rope_none_is_the_layer_as_it_was(kind, monkeypatch):
    """Bit-equal outputs and gradients, and the same native calls in the same order, with rope=None and without the argument —
    uncached, prefill and a decoding step."""
    rs = np.random.RandomState(5)
    x, g = rs.randn(2, 4, 16).astype(np.float32), rs.randn(2, 4, 16).astype(np.float32)
    seen = dsu.count_calls(monkeypatch)

    def trace(layer):
        del seen[:]
        for p in layer.params.values():
            p.zero_grad()
        out = layer.forward(Tensor(x))
        out.backward(g)
        cache = gen.LayerCache(6)
        pre = layer.forward(Tensor(x), cache=cache)
        step = layer.forward(Tensor(x[:, :1]), cache=cache)
        grads = [np.asarray(p.grad) for p in layer.params.values()]
        return list(seen), [np.asarray(out.values), np.asarray(pre.values), np.asarray(step.values)] + grads

    trace(_built(kind))                                                   # (the composed route uploads a causal mask once)
    calls_a, vals_a = trace(_built(kind))
    calls_b, vals_b = trace(_built(kind, rope=None))
    assert calls_a == calls_b and calls_a and not [c for c in calls_a if c.startswith("rope")]
    assert all(np.array_equal(rsup.bits(a), rsup.bits(b)) for a, b in zip(vals_a, vals_b))
    with_rope = _built(kind, rope=rp.Rotary(8))
    calls_c, vals_c = trace(with_rope)
    assert not np.array_equal(vals_c[0], vals_a[0])                      # and with a Rotary the positions enter

def test_layer_positions_cached_against_uncached():
    """One layer: the prefill plus decoding steps give the rows of the uncached forward — the step's position is the cache row —
    uniform and ragged; v is not rotated and the cached key is the rotated one."""
    rs = np.random.RandomState(7)
    x = rs.randn(2, 6, 16).astype(np.float32)
    layer = _built("mha", rope=rp.Rotary(8))
    full = np.asarray(layer.forward(Tensor(x)).values)
    for ragged in (False, True):
        lens = da.lengths([4, 4]) if ragged else None
        cache = gen.LayerCache(6)
        pre = np.asarray(layer.forward(Tensor(x[:, :4]), cache=cache).values)
        np.testing.assert_allclose(pre, full[:, :4], rtol=0, atol=1e-5)
        cache.lens = lens
        for t in (4, 5):
            step = np.asarray(layer.forward(Tensor(x[:, t:t + 1]), cache=cache).values)
            np.testing.assert_allclose(step[:, 0], full[:, t], rtol=0, atol=1e-5)
            if ragged:
                lens.host += 1
                lens.dev[...] = tn.asarray(lens.host)
    p = layer.params
    rows = x.reshape(12, 16).astype(np.float64)
    k64 = (rows @ np.asarray(p["wk"].values, dtype=np.float64) + np.asarray(p["bk"].values, dtype=np.float64)).reshape(2, 6, 2, 4)
    v64 = (rows @ np.asarray(p["wv"].values, dtype=np.float64) + np.asarray(p["bv"].values, dtype=np.float64)).reshape(2, 6, 2, 4)
    cos_t, sin_t = layer.rope.host_tables(4, np.float64)
    kr64 = ro.reference(k64, cos_t, sin_t, dtype=np.float64).values.astype(np.float64)
    np.testing.assert_allclose(np.asarray(cache.k), kr64, rtol=0, atol=1e-5)
    np.testing.assert_allclose(np.asarray(cache.v), v64, rtol=0, atol=1e-5)


def test_generation_with_a_rotary(golden):
    """rope_oracle's two-block model (grouped heads, no position table, one shared Rotary), greedy: cached, uncached and
    ragged-at-uniform-lengths generation all pick the float64 oracle's tokens, whose top-2 margin exceeds 2 x LM_MARGIN logit
    bounds at every step."""
    c = ro.LM
    seed, scale, bound = int(golden["lm.seed"]), float(golden["lm.head_scale"]), float(golden["lm.logit_bound"])
    params, prompt = ro.lm_params(seed, scale), ro.lm_prompt(seed)
    ids = golden["lm.ids"]
    tn.set_default_float(np.float32)
    net = rsup.lm_net(params, np.float32)
    rotaries = {id(l.rope) for l in net.layers if getattr(l, "rope", None) is not None}
    assert len(rotaries) == 1 and "pos" not in net.layers[0].params
    steps = ro.lm_generate(params, prompt, 1)[1]
    got = rsup.lm_last_logits(net, prompt)
    assert np.abs(got - steps[0]).max() <= ro.LM_MARGIN * bound
    cached = gen.generate(net, prompt, c["new"], temperature=0.0, cache=True)
    full = gen.generate(net, prompt, c["new"], temperature=0.0, cache=False)
    assert np.array_equal(cached, ids) and np.array_equal(full, ids)
    lens = np.full((c["B"],), c["prompt"], dtype=np.int64)
    ragged = gen.generate(net, prompt, c["new"], temperature=0.0, prompt_lens=lens)
    assert np.array_equal(np.asarray(ragged), ids)
    rot = net.layers[1].rope
    assert len(rot._device) == 1                                          # one pair of device tables for the whole model
    before = [id(a) for a in rot._device[(4, np.dtype(np.float32))]]
    gen.generate(net, prompt, 2, temperature=0.0)
    assert [id(a) for a in rot._device[(4, np.dtype(np.float32))]] == before


def test_max_len_refusals_fire_before_any_launch(monkeypatch):
    c = ro.LM
    params, prompt = ro.lm_params(0, 1.0), ro.lm_prompt(0)
    net = rsup.lm_net(params, np.float32, max_len=8)
    x = np.zeros((2, 9, 16), dtype=np.float32)
    layer = _built("mha", rope=rp.Rotary(8))
    block = _built("block", rope=rp.Rotary(8))
    seen = dsu.count_calls(monkeypatch)
    lens = np.full((c["B"],), c["prompt"], dtype=np.int64)
    for kw in (dict(), dict(cache=False), dict(prompt_lens=lens), dict(prompt_lens=lens, eos_id=3)):
        with pytest.raises(ValueError, match="exceed the rotary tables' max_len 8"):
            gen.generate(net, prompt, 5, temperature=0.0, **kw)
    assert not seen
    for l in (layer, block):
        xt = Tensor(x)
        del seen[:]
        with pytest.raises(ValueError, match="outside the rotary tables' max_len 8"):
            l.forward(xt)
        assert not seen
    # a decoding step at a cache row beyond the tables; a ragged step whose host mirror is beyond them
    long_layer = _built("mha", rope=rp.Rotary(4))
    cache = gen.LayerCache(8)
    long_layer.forward(Tensor(x[:, :4]), cache=cache)
    step = Tensor(x[:, :1])
    del seen[:]
    with pytest.raises(ValueError, match="positions 4 .. 4 lie outside the rotary tables' max_len 4"):
        long_layer.forward(step, cache=cache)
    cache.lens = da.lengths([2, 4])
    del seen[:]
    with pytest.raises(ValueError, match="positions 2 .. 4 lie outside"):
        long_layer.forward(step, cache=cache)
    assert not seen
    assert np.array_equal(gen.generate(net, prompt, 4, temperature=0.0).shape, (c["B"], c["prompt"] + 4))      # 8 fits
