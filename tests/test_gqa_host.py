"""Grouped-query attention above the kernels — device_array routes, graph nodes, wrappers, MultiHeadAttention(kv_heads=) and
TransformerBlock — on the backend of the session (the CPU test twin runs the composed route): the golden values inside the
oracle's bounds, arena-backed gradients, the ragged composed decode, rejected arguments, parameter shapes and order, the
grouped layer against a plain layer with repeated key / value weights, and the unchanged call trace of kv_heads=None.

Layer bounds (test_grouped_layer_equals_the_plain_layer_with_repeated_weights).  Both layers evaluate, in the operand dtype,
the SAME real-valued function (repeating wk / wv / bk / bv column blocks over the group IS the head mapping), so each lies
within a first-order bound of the float64 replica attn_oracle.MHA64 and the two agree within the sum of the two.  An element
of the output, or of a weight gradient, is a sum of products reached through a chain of dot products of lengths E (three
projections), D (scores), Tk (softmax sum and p v), E (output projection) and B T (weight gradients) — forward and backward
pass through each at most twice — plus the exp, log, division and scaling roundings of the softmax (under 16).  To first
order its error is at most  N u sum|terms|  with  N = 4 (2 E + D + 2 Tk + B T + 16)  and sum|terms| the sum of the absolute
values behind the element: MHA64.grad_scales for the gradients, |att64| |wo| + |bo| for the output."""

import os

import numpy as np
import pytest

import attn_oracle as ao
import dropout_support as dsu
import gqa_oracle as go
import tinynn_autograd_amd as tn
from tinynn_autograd_amd import _lib, device_array as da, generation as gen
from tinynn_autograd_amd.core import ops
from tinynn_autograd_amd.core.layers import MultiHeadAttention, TransformerBlock, MHA_PARAM_ORDER, BLOCK_PARAM_ORDER
from tinynn_autograd_amd.core.tensor import Tensor

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gqa_cases.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def leaf(a):
    t = Tensor(a, requires_grad=True)
    t.zero_grad()
    return t


def test_the_session_route():
    lib = _lib.get()
    plan = da._gqa_plan(tn.ones((1, 2, 4, 3)), tn.ones((1, 5, 2, 3)), tn.ones((1, 5, 2, 3)), False, None, None)
    assert plan.route == ("native" if lib.has_gqa else "composed")
    if tn.backend_name() != "hip-gfx950":
        assert plan.route == "composed"
    assert da.GQA_ROUTE is None


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", sorted(go.GQA_CASES))
def test_composed_training_route_matches_the_golden_values(golden, name, dtype):
    q, k, v, do_, causal, scale = go.case_input(name)          # float32-exact inputs, as the fixture's
    q, k, v, do_ = (a.astype(dtype) for a in (q, k, v, do_))
    tn.set_default_float(dtype)
    res = go.reference(q, k, v, do_, causal, scale, dtype)
    for field in go.FIELDS:
        np.testing.assert_array_equal(res.values[field], golden["attn.%s.%s" % (name, field)])     # the fixture is the oracle's
    o, lse = da.gqa_attention(q, k, v, causal, scale, route="composed")
    dq, delta = da.gqa_attention_bwd_q(q, k, v, o, do_, lse, causal, scale, route="composed")
    dk, dv = da.gqa_attention_bwd_kv(q, k, v, do_, lse, delta, causal, scale, route="composed")
    assert dk.shape == k.shape and dv.shape == v.shape and o.dtype == dtype
    go.check(dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv), res, "%s composed" % name)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", sorted(go.GQA_DECODE_CASES))
def test_composed_decode_route_matches_the_golden_values(golden, name, dtype):
    case = go.decode_case(name)                                # float32-exact inputs, as the fixture's
    case = {key: (a.astype(dtype) if isinstance(a, np.ndarray) else a) for key, a in case.items()}
    tn.set_default_float(dtype)
    res = go.decode_reference(dtype=dtype, **case)
    np.testing.assert_array_equal(res.values["o"], golden["decode." + name])
    kc, vc = tn.asarray(case["k_cache"]), tn.asarray(case["v_cache"])
    o = da.gqa_decode(case["q"], kc, vc, case["length"], case["k_new"], case["v_new"], layout=case["layout"], route="composed")
    go.assert_within(o, res.values["o"], res.bounds["o"], "%s composed" % name)
    np.testing.assert_array_equal(np.asarray(kc), res.values["k_cache"])              # the append, and nothing else, bit for bit
    np.testing.assert_array_equal(np.asarray(vc), res.values["v_cache"])


def test_composed_ragged_decode_is_the_uniform_call_per_sequence(monkeypatch):
    rs = np.random.RandomState(5)
    q, kc, vc, kn, vn = go.decode_inputs(rs, "bthd", 3, 4, 2, 20, 6, 5)
    lens = [7, 0, 25]                                                              # the last one is outside [0, Tmax)
    kd, vd = tn.asarray(kc), tn.asarray(vc)
    o = np.asarray(da.gqa_decode(q, kd, vd, None, kn, vn, lens=da.lengths(lens), route="composed"))
    for b in (0, 1):
        one = slice(b, b + 1)
        k1, v1 = tn.asarray(kc[one]), tn.asarray(vc[one])
        want = da.gqa_decode(q[one], k1, v1, lens[b], kn[one], vn[one], route="composed")
        np.testing.assert_array_equal(o[one], np.asarray(want))
        np.testing.assert_array_equal(np.asarray(kd)[one], np.asarray(k1))
    assert not o[2].any()
    np.testing.assert_array_equal(np.asarray(kd)[2], kc[2])                          # an invalid length leaves the caches alone
    monkeypatch.setattr(_lib, "capturing", True)
    with pytest.raises(RuntimeError, match="graph capture cannot do"):
        da.gqa_decode(q, kd, vd, None, kn, vn, lens=da.lengths(lens), route="composed")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_node_forward_gradients_and_arena_views(dtype):
    tn.set_default_float(dtype)
    rs = np.random.RandomState(17)
    q, k, v, do_ = go.make_inputs(rs, 2, 6, 2, 9, 12, 5, 7, dtype)
    res = go.reference(q, k, v, do_, True, None, dtype)
    arena = tn.zeros((q.size + k.size + v.size,))
    leaves, off = [], 0
    for a in (q, k, v):
        t = Tensor(a, requires_grad=True)
        t._grad_home = arena[off:off + a.size].reshape(a.shape)
        t.zero_grad()
        leaves.append(t)
        off += a.size
    qt, kt, vt = leaves
    out = ops.attention_gqa(qt, kt, vt, causal=True)
    assert out.values.dtype == dtype and out.shape == do_.shape and out.requires_grad
    out.backward(do_)
    for t in leaves:
        assert t.grad is t._grad_home and t.grad.shape == t.shape
    go.check(dict(o=out.values, dq=qt.grad, dk=kt.grad, dv=vt.grad), res, "node")
    # q frozen: only k and v are edges; the per-edge forms (one tensor on two edges) add up
    kt2, vt2 = leaf(k), leaf(v)
    out2 = ops.attention_gqa(Tensor(q), kt2, vt2, causal=True)
    assert [d["tensor"] for d in out2.dependency] == [kt2, vt2]
    out2.backward(do_)
    go.check(dict(dk=kt2.grad, dv=vt2.grad), res, "q frozen")
    kv = leaf(rs.randn(2, 12, 2, 5).astype(dtype))
    q5 = (rs.randn(2, 9, 6, 5) * 2).astype(dtype)
    g5 = rs.randn(2, 9, 6, 5).astype(dtype)
    ops.attention_gqa(Tensor(q5), kv, kv).backward(g5)
    r5 = go.reference(q5, np.asarray(kv.values), np.asarray(kv.values), g5, False, None, dtype)
    want = r5.values["dk"] + r5.values["dv"]
    bound = r5.bounds["dk"] + r5.bounds["dv"] + 2 * go.unit(dtype) * (np.abs(r5.values["dk"]) + np.abs(r5.values["dv"]))
    go.assert_within(kv.grad, want, bound, "k and v are one tensor")


def test_rejected_arguments():
    q, k, v = (Tensor(np.ones(s, dtype=np.float32)) for s in ((1, 3, 4, 2), (1, 5, 2, 2), (1, 5, 2, 2)))
    for fn in (ops.attention_gqa, ops.attention_gqa_):
        with pytest.raises(TypeError, match="out of scope"):
            fn(q, k, v, mask=None)
    with pytest.raises(TypeError, match="unsupported arguments"):
        ops.attention_gqa(q, k, v, layout="bhtd")
    with pytest.raises(ValueError, match="no multiple"):
        ops.attention_gqa(q, Tensor(np.ones((1, 5, 3, 2), dtype=np.float32)), Tensor(np.ones((1, 5, 3, 2), dtype=np.float32)))
    with pytest.raises(ValueError, match="route must be"):
        ops.attention_gqa_(q, k, v, route="quick")
    kc, vc = tn.zeros((1, 8, 2, 2)), tn.zeros((1, 8, 2, 2))
    q1, new = Tensor(np.ones((1, 4, 2), dtype=np.float32)), Tensor(np.ones((1, 2, 2), dtype=np.float32))
    for fn, args in ((ops.attention_decode_gqa_, (q1, kc, vc, 2, new, new)),
                     (ops.attention_decode_ragged_gqa_, (q1, kc, vc, da.lengths([2]), new, new)),
                     (ops.attention_decode_gqa, (q1, kc, vc, 2, new, new))):
        with pytest.raises(TypeError, match="unsupported arguments"):
            fn(*args, bf16=True)
    with pytest.raises(ValueError, match="length= .* or lens="):
        ops.attention_decode_gqa(q1, kc, vc)
    out = ops.attention_decode_gqa(q1, kc, vc, lens=da.lengths([2]), k_new=new, v_new=new)
    assert out.shape == (1, 4, 2) and not out.requires_grad and not out.dependency
    # the old ops still raise on unknown arguments, and now say where grouped-query heads went
    with pytest.raises(TypeError, match="attention_decode_gqa_"):
        ops.attention_decode_(q1, tn.zeros((1, 8, 4, 2)), tn.zeros((1, 8, 4, 2)), 2, kv_heads=2)
    with pytest.raises(TypeError, match="attention_decode_ragged_gqa_"):
        ops.attention_decode_ragged_(q1, tn.zeros((1, 8, 4, 2)), tn.zeros((1, 8, 4, 2)), da.lengths([2]), q1, q1, kv_heads=2)


def test_layer_parameter_shapes_order_and_rng_draws():
    np.random.seed(3)
    layer = MultiHeadAttention(4, num_in=8, kv_heads=2)
    assert list(layer.params) == list(MHA_PARAM_ORDER)
    want = {"wq": (8, 8), "bq": (1, 8), "wk": (8, 4), "bk": (1, 4), "wv": (8, 4), "bv": (1, 4), "wo": (8, 8), "bo": (1, 8)}
    assert {n: tuple(layer.params[n].shape) for n in MHA_PARAM_ORDER} == want
    # the draws come in parameter order: wq is what a plain layer draws first from the same seed
    np.random.seed(3)
    plain = MultiHeadAttention(4, num_in=8)
    np.testing.assert_array_equal(np.asarray(layer.params["wq"].values), np.asarray(plain.params["wq"].values))
    np.random.seed(3)
    lazy = MultiHeadAttention(4, kv_heads=2)
    lazy.forward(Tensor(np.zeros((1, 3, 8), dtype=np.float32)))
    for n in MHA_PARAM_ORDER:
        np.testing.assert_array_equal(np.asarray(lazy.params[n].values), np.asarray(layer.params[n].values))
    for bad in (3, 0, 8):
        with pytest.raises(ValueError, match="divisor of num_heads"):
            MultiHeadAttention(4, kv_heads=bad)
    np.random.seed(4)
    block = TransformerBlock(4, num_in=8, causal=True, kv_heads=1)
    assert list(block.params) == list(BLOCK_PARAM_ORDER)
    assert tuple(block.params["attn.wk"].shape) == (8, 2) and tuple(block.params["attn.bv"].shape) == (1, 2)
    assert block.forward(Tensor(np.ones((2, 3, 8), dtype=np.float32))).shape == (2, 3, 8)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("heads, kv_heads", [(4, 2), (4, 1), (2, 2)])
def test_grouped_layer_equals_the_plain_layer_with_repeated_weights(dtype, heads, kv_heads):
    tn.set_default_float(dtype)
    B, T, E = 2, 5, 8
    rs = np.random.RandomState(21)
    x, g = rs.randn(B, T, E).astype(dtype), rs.randn(B, T, E).astype(dtype)
    np.random.seed(5)
    grouped = MultiHeadAttention(heads, num_in=E, causal=True, kv_heads=kv_heads)
    for n in ("bq", "bk", "bv", "bo"):                        # (zeros by default: give the biases something to carry)
        grouped.params[n].values = tn.asarray((rs.randn(*grouped.params[n].shape) * 0.1).astype(dtype))
    params = [np.asarray(grouped.params[n].values) for n in MHA_PARAM_ORDER]
    for n, a in zip(MHA_PARAM_ORDER, params):                 # (the initialisers draw float32: every parameter in `dtype`)
        grouped.params[n].values = tn.asarray(a.astype(dtype))
    plain = MultiHeadAttention(heads, num_in=E, causal=True)
    for n, a in zip(MHA_PARAM_ORDER, go.plain_params(params, heads, kv_heads)):
        plain.params[n].values = tn.asarray(a.astype(dtype))
    outs = {}
    for name, layer in (("grouped", grouped), ("plain", plain)):
        for p in layer.params.values():
            p.zero_grad()
        out = layer.forward(Tensor(x))
        out.backward(g)
        outs[name] = np.asarray(out.values, dtype=np.float64)
    ref = ao.MHA64(go.plain_params(params, heads, kv_heads), heads, causal=True)
    # MHA64's loss is ((out - y) ** 2).sum() / B: y = out64 - g B / 2 makes its output gradient exactly g
    _, out64, _ = ref.loss_and_grads(x, np.zeros((B, T, E)))
    _, out64, g64 = ref.loss_and_grads(x, out64 - np.asarray(g, dtype=np.float64) * B / 2.0)
    N = 4 * (2 * E + E // heads + 2 * T + B * T + 16)
    u = go.unit(dtype)
    wq, bq, wk, bk, wv, bv, wo, bo = ref.p
    rows = np.asarray(x, dtype=np.float64).reshape(B * T, E)
    q64, k64, v64 = ((rows @ w + c).reshape(B, T, heads, E // heads) for w, c in ((wq, bq), (wk, bk), (wv, bv)))
    att64 = ao.reference(q64, k64, v64, None, True, None, "bthd").values["o"].reshape(B * T, E)
    b_out = (N * u * (np.abs(att64) @ np.abs(wo) + np.abs(bo))).reshape(B, T, E)
    for name in outs:
        assert (np.abs(outs[name] - out64) <= b_out).all(), name
    assert (np.abs(outs["grouped"] - outs["plain"]) <= 2 * b_out).all()                  # the sum of the two bounds
    for at, n in enumerate(MHA_PARAM_ORDER):
        gp, gg = np.asarray(plain.params[n].grad, dtype=np.float64), np.asarray(grouped.params[n].grad, dtype=np.float64)
        want, scale = g64[at], ref.grad_scales[at]
        assert (np.abs(gp - want) <= N * u * scale).all(), "plain " + n
        if n[1] in "kv":                                      # the grouped layer's gradient: the group sums of the column blocks
            want, scale = go.fold_columns(want, heads, kv_heads), go.fold_columns(scale, heads, kv_heads)
            gp = go.fold_columns(gp, heads, kv_heads)
        assert gg.shape == want.shape
        assert (np.abs(gg - want) <= N * u * scale).all(), "grouped " + n
        assert (np.abs(gg - gp) <= 2 * N * u * scale).all(), "grouped vs plain " + n         # the sum of the two bounds


def test_kv_heads_none_runs_the_calls_it_ran_before(monkeypatch):
    """kv_heads=None (and the default) is the multi-head path launch for launch: the same native calls, in the same order, as
    the hand-written chain the layer has always been — three dense_, attention_, dense_ — and none of the grouped ones."""
    rs = np.random.RandomState(2)
    x, g = rs.randn(2, 4, 8).astype(np.float32), rs.randn(2, 4, 8).astype(np.float32)
    np.random.seed(1)
    layer = MultiHeadAttention(2, num_in=8, causal=True, kv_heads=None)
    seen = dsu.count_calls(monkeypatch)

    def traced(fn):
        del seen[:]
        fn()
        return list(seen)

    def by_layer(l):
        for p in l.params.values():
            p.zero_grad()
        l.forward(Tensor(x)).backward(g)

    def by_hand():
        p = layer.params
        for t in p.values():
            t.zero_grad()
        rows = ops.reshape(Tensor(x), (8, 8))
        q, k, v = (ops.reshape(ops.dense_(rows, p["w" + n], p["b" + n]), (2, 4, 2, 4)) for n in "qkv")
        att = ops.attention_(q, k, v, causal=True, layout="bthd")
        ops.reshape(ops.dense_(ops.reshape(att, (8, 8)), p["wo"], p["bo"]), (2, 4, 8)).backward(g)

    by_hand()                                                 # (the composed route uploads a new causal mask once)
    want = traced(by_hand)
    assert traced(lambda: by_layer(layer)) == want and want
    np.random.seed(1)
    default = MultiHeadAttention(2, num_in=8, causal=True)
    assert traced(lambda: by_layer(default)) == want
    assert not [c for c in want if c.startswith("gqa")]
    # the cached path of a grouped layer keeps Hkv heads in its cache
    np.random.seed(1)
    grouped = MultiHeadAttention(4, num_in=8, causal=True, kv_heads=2)
    cache = gen.LayerCache(6)
    grouped.forward(Tensor(x), cache=cache)
    assert tuple(cache.k.shape) == (2, 6, 2, 2) and cache.length == 4
    step = grouped.forward(Tensor(x[:, :1]), cache=cache)
    assert step.shape == (2, 1, 8) and cache.length == 5
