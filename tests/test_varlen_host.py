"""Attention with per-sequence lengths on the CPU test twin, where everything takes the composed route: the raw calls and the
ops against the per-sequence oracle (forward and all three gradients, causal and not, plain and grouped heads, both layouts),
dead elements exactly +0, lens=None the bits of the call without the argument, the layers and Model.forward(lens=), and the
refusals — a host list, a Lengths outside [0, T], lens with a cache — before any launch."""

import numpy as np
import pytest

import attn_oracle as ao
import gqa_oracle as go
import gqa_support as gs
import varlen_support as vs
import tinynn_autograd_amd as tn
from tinynn_autograd_amd import _lib, device_array as da
from tinynn_autograd_amd.core import ops
from tinynn_autograd_amd.core.layers import MultiHeadAttention, TransformerBlock
from tinynn_autograd_amd.core.losses import SoftmaxCrossEntropyLoss
from tinynn_autograd_amd.core.model import Model
from tinynn_autograd_amd.core.optimizer import Adam
from tinynn_autograd_amd.core.tensor import Tensor


@pytest.fixture(autouse=True)
def _switches():
    yield
    da.VARLEN_ROUTE = None
    tn.set_default_float(np.float32)


CASES = [("bthd", 4, 2, 2, 9, 5, 3, (9, 0, 1, 6)), ("bthd", 3, 4, 2, 70, 8, 8, (70, 37, 64)), ("bthd", 2, 4, 1, 7, 4, 6, (3, 7)),
         ("bhtd", 4, 1, 1, 13, 6, 4, (1, 13, 8, 0))]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("causal", [False, True])
def test_the_composed_route_against_the_oracle(causal, dtype):
    tn.set_default_float(dtype)
    for layout, b, h, hkv, t, d, dv, lens in CASES:
        q, k, v, do_ = vs.make_inputs(ao.case_seed("host%s%d" % (layout, t)), layout, b, h, hkv, t, d, dv, dtype)
        res = vs.reference(q, k, v, do_, lens, causal, None, layout, dtype)
        got = vs.run("composed", q, k, v, do_, lens, causal, None, layout, dtype)
        what = "%s T %d lens %s causal %s" % (layout, t, lens, causal)
        assert all(a.dtype == dtype and np.isfinite(a).all() for a in got.values())
        vs.check(got, res, what)
        vs.assert_dead_are_plus_zero(got, lens, layout, what)
        if layout == "bthd" and h == hkv:          # the plain functions take the same lengths in layout "bthd"
            vs.check(vs.run_plain("composed", q, k, v, do_, lens, causal, None, dtype), res, what + " (plain)")


@pytest.mark.parametrize("grouped", [False, True])
def test_the_ops_against_the_oracle(grouped):
    """ops.attention_ / ops.attention_gqa_ with lens=: the node's values and the gradients that backward() leaves."""
    b, h, hkv, t, d, dv, lens = 3, 4, (2 if grouped else 4), 11, 8, 6, (11, 4, 0)
    q, k, v, do_ = vs.make_inputs(7 + grouped, "bthd", b, h, hkv, t, d, dv)
    for causal in (False, True):
        res = vs.reference(q, k, v, do_, lens, causal, None, "bthd", np.float32)
        tq, tk, tv = (Tensor(a, requires_grad=True) for a in (q, k, v))
        ld = da.lengths(lens)
        out = (ops.attention_gqa_(tq, tk, tv, causal=causal, lens=ld) if grouped
               else ops.attention_(tq, tk, tv, causal=causal, layout="bthd", lens=ld))
        out.backward(tn.asarray(do_))
        got = dict(o=np.asarray(out.values), dq=np.asarray(tq.grad), dk=np.asarray(tk.grad), dv=np.asarray(tv.grad))
        vs.check(got, res, "op grouped %s causal %s" % (grouped, causal))
        vs.assert_dead_are_plus_zero(got, lens, "bthd", "op")
    # the functional forms hand lens on; mask=, dropout= and dtype= keep raising exactly as before
    fn = ops.attention_gqa if grouped else ops.attention
    extra = {} if grouped else dict(layout="bthd")
    o2 = fn(q, k, v, causal=True, lens=da.lengths(lens), **extra)
    assert np.array_equal(vs.bits(np.asarray(o2.values)), vs.bits(got["o"]))
    for bad in ("mask", "dropout", "dtype"):
        with pytest.raises(TypeError, match="unsupported arguments"):
            fn(q, k, v, **{bad: 1})
    with pytest.raises(TypeError, match="ragged chunks and bf16 are out of scope"):
        ops.attention_extend_(Tensor(q), None, None, 0, Tensor(k), Tensor(v), lens=da.lengths(lens))


def test_lens_none_is_the_call_without_the_argument():
    q, k, v, do_ = vs.make_inputs(3, "bthd", 2, 2, 2, 9, 5, 3)
    for fwd in (da.attention, da.gqa_attention):
        opts = dict(layout="bthd") if fwd is da.attention else {}
        a, b = fwd(q, k, v, causal=True, **opts), fwd(q, k, v, causal=True, lens=None, **opts)
        assert all(np.array_equal(vs.bits(np.asarray(x)), vs.bits(np.asarray(y))) for x, y in zip(a, b))
    full = vs.run("composed", q, k, v, do_, (9, 9), True, None, "bthd", np.float32)          # all lengths T: the same maths
    plain = gs.run_training("composed", q, k, v, do_, True, None, np.float32)
    res = go.reference(q, k, v, do_, True, None, np.float32)
    for name in ("o", "lse", "dq", "dk", "dv"):
        assert (np.abs(full[name].astype(np.float64) - plain[name]) <= 2 * res.bounds[name]).all(), name


def test_refusals_come_before_any_launch(monkeypatch):
    q, k, v, _ = vs.make_inputs(5, "bthd", 2, 2, 2, 9, 5, 3)
    calls = []
    monkeypatch.setattr(da, "matmul", lambda *a, **kw: calls.append("matmul") or (_ for _ in ()).throw(AssertionError("a launch")))
    for fwd in (da.attention, da.gqa_attention):
        opts = dict(layout="bthd") if fwd is da.attention else {}
        for host in ([9, 3], (9, 3), np.array([9, 3])):
            with pytest.raises(TypeError, match="lens must be a ragged.Lengths or a dense int64 device array"):
                fwd(q, k, v, lens=host, **opts)
        with pytest.raises(TypeError, match="dense int64 device array"):
            fwd(q, k, v, lens=tn.asarray(np.array([9.0, 3.0], dtype=np.float32)), **opts)
        for bad in ([10, 3], [-1, 3]):
            with pytest.raises(ValueError, match=r"outside \[0, T = 9\]"):
                fwd(q, k, v, lens=da.lengths(bad), **opts)
        with pytest.raises(ValueError, match=r"lens must have shape \(B,\)"):
            fwd(q, k, v, lens=da.lengths([9, 3, 1]), **opts)
    with pytest.raises(ValueError, match="Tq == Tk"):
        da.attention(q[:, :4], k, v, layout="bthd", lens=da.lengths([4, 3]))
    with pytest.raises(ValueError, match="exactly three axes"):
        da.attention(q, k, v, layout="bhtd", lens=da.lengths([2, 2]))
    assert not calls


def test_the_composed_route_refuses_a_graph_capture(monkeypatch):
    q, k, v, _ = vs.make_inputs(5, "bthd", 2, 2, 2, 9, 5, 3)
    ld = da.lengths([9, 3])
    monkeypatch.setattr(_lib, "capturing", True)
    with pytest.raises(RuntimeError, match="a graph capture cannot do"):
        da.attention(q, k, v, layout="bthd", lens=ld)


def test_a_device_array_of_lengths_is_read_back():
    q, k, v, do_ = vs.make_inputs(6, "bthd", 2, 2, 2, 9, 5, 3)
    a = vs.run("composed", q, k, v, do_, (9, 3), False, None, "bthd", np.float32)
    b = vs.run("composed", q, k, v, do_, (9, 3), False, None, "bthd", np.float32, lens_dev=tn.asarray(np.array([9, 3], dtype=np.int64)))
    assert all(np.array_equal(vs.bits(a[n]), vs.bits(b[n])) for n in a)


def _mha(kv_heads, causal, dtype, seed=11):
    layer = MultiHeadAttention(4, num_in=16, causal=causal, kv_heads=kv_heads, fused=True)
    rs = np.random.RandomState(seed)
    for name, p in layer.params.items():
        p.values = tn.asarray(rs.uniform(-0.5, 0.5, tuple(p.shape)).astype(dtype), dtype=dtype)
        p.zero_grad()
    return layer


@pytest.mark.parametrize("kv_heads", [None, 2])
def test_a_non_causal_layer_sees_live_tokens_only(kv_heads):
    """MultiHeadAttention.forward(lens=) in float64: the live rows of sequence b equal the layer run on that sequence alone cut
    to lens[b] tokens, and the parameter gradients of a loss over the live rows equal the sum of the per-sequence ones.  Two
    float64 evaluations of the same sums in different groupings: 1e-12 of the largest magnitude (u = 2**-53, a few hundred
    terms).  Without lens the non-causal rows attend over padding and miss this by orders of magnitude."""
    tn.set_default_float(np.float64)
    lens, t = (6, 0, 3), 6
    x = np.random.RandomState(2).randn(3, t, 16)
    g = np.random.RandomState(3).randn(3, t, 16)
    for b, n in enumerate(lens):
        g[b, n:] = 0.0                                     # the loss ignores the padding
    layer = _mha(kv_heads, False, np.float64)
    out = layer.forward(Tensor(x, dtype=np.float64), lens=da.lengths(lens))
    out.backward(tn.asarray(g))
    got = np.asarray(out.values)
    grads = {n: np.asarray(p.grad) for n, p in layer.params.items()}
    want_grads = {n: np.zeros_like(a) for n, a in grads.items()}
    for b, n in enumerate(lens):
        if n == 0:
            continue
        for p in layer.params.values():
            p.zero_grad()
        alone = layer.forward(Tensor(x[b:b + 1, :n], dtype=np.float64))
        alone.backward(tn.asarray(g[b:b + 1, :n]))
        assert np.abs(got[b, :n] - np.asarray(alone.values)[0]).max() <= 1e-12 * np.abs(got).max()
        for name, p in layer.params.items():
            want_grads[name] += np.asarray(p.grad)
    for name in grads:
        assert np.abs(grads[name] - want_grads[name]).max() <= 1e-12 * max(np.abs(want_grads[name]).max(), 1.0), name
    # the dead rows leave the attention op as +0: what remains there is the output projection's bias
    bias = np.asarray(layer.params["bo"].values)[0]
    assert np.array_equal(got[1], np.broadcast_to(bias, (t, 16))) and np.array_equal(got[2, 3:], np.broadcast_to(bias, (3, 16)))


def test_lens_with_a_cache_raises_before_any_launch(monkeypatch):
    layer = _mha(None, True, np.float32)
    block = TransformerBlock(4, hidden=32, num_in=16, causal=True)
    x = Tensor(np.zeros((2, 5, 16), dtype=np.float32))
    cache = object()                               # (never looked at: the refusal comes first)
    monkeypatch.setattr(ops, "dense_", lambda *a, **kw: (_ for _ in ()).throw(AssertionError("a launch")))
    monkeypatch.setattr(ops, "layer_norm_", lambda *a, **kw: (_ for _ in ()).throw(AssertionError("a launch")))
    for part in (layer, block):
        with pytest.raises(ValueError, match="do not go together"):
            part.forward(x, cache=cache, lens=da.lengths([5, 2]))


def test_model_forward_hands_lens_to_the_layers_that_take_it(monkeypatch):
    """Net.forward / Model.forward(lens=) on gqa_oracle's two-block language model: every attention node gets the lengths (and
    nothing else does), the causal model's live logits are those of the run without them (two float32 evaluations: within the
    fixture's margin of the float64 logits' own error scale), and lens=None is the call without the argument."""
    params = go.lm_params(5, 1.0)
    net = gs.lm_net(params)
    model = Model(net, SoftmaxCrossEntropyLoss(), Adam())
    ids = np.random.RandomState(9).randint(0, go.LM["V"], (2, 9)).astype(np.int64)
    lens = da.lengths([9, 4])
    seen = []
    real = ops.attention_gqa_
    monkeypatch.setattr(ops, "attention_gqa_", lambda *a, **kw: seen.append(kw.get("lens")) or real(*a, **kw))
    model.set_phase("TEST")
    with_lens = np.asarray(model.forward(Tensor(ids), lens=lens).values)
    assert seen == [lens, lens]
    del seen[:]
    without = np.asarray(model.forward(Tensor(ids)).values)
    none = np.asarray(model.forward(Tensor(ids), lens=None).values)
    assert seen == [None] * 4 and np.array_equal(vs.bits(without), vs.bits(none))
    want = go.lm_logits(params, ids).reshape(without.shape)
    scale = go.LM_MARGIN * np.abs(want - without).max()
    live = np.zeros((2, 9), dtype=bool)
    live[0], live[1, :4] = True, True
    live = live.reshape(-1)
    assert scale > 0 and np.abs(with_lens.astype(np.float64) - without)[live].max() <= scale
    assert np.abs(with_lens.astype(np.float64) - without)[~live].max() > scale        # the padding rows did change
