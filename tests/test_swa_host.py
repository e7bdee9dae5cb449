"""swa.py, window= and the ring cache on the CPU twin (composed route): rule, walk, oracle, refusals, window=None, generation."""

import numpy as np
import pytest

import attn_oracle as ao
import gated_support as gsup
import swa_oracle as so
import tinynn_autograd_amd as tn
from tinynn_autograd_amd import device_array as da
from tinynn_autograd_amd import swa
from tinynn_autograd_amd.core import ops
from tinynn_autograd_amd.core.layers import MultiHeadAttention, TransformerBlock
from tinynn_autograd_amd.core.tensor import Tensor


@pytest.mark.parametrize("T", [1, 63, 64, 65, 130, 200, 300])
@pytest.mark.parametrize("W", [1, 2, 17, 63, 64, 65, 129, 400])
def test_the_rule_and_the_walk_against_brute_force(T, W):
    keep = np.array([[i - W < j <= i for j in range(T)] for i in range(T)])
    assert np.array_equal(swa.band_mask(T, W), keep) and np.array_equal(so.keep(T, W), keep)
    blocks = range(0, T, swa.BLOCK)
    tile = lambda q0, k0: keep[q0:q0 + swa.BLOCK, k0:k0 + swa.BLOCK]
    whole = swa.band_mask(T + swa.BLOCK, W)       # (the test of a block pair does not know T: whole 64 x 64 tiles)
    for q0 in blocks:
        assert swa.key_blocks(q0, T, W) == [k0 for k0 in blocks if tile(q0, k0).any()]
        for k0 in swa.key_blocks(q0, T, W):       # interior: every pair of the tile is kept
            assert swa.interior(q0, k0, W) == bool(whole[q0:q0 + swa.BLOCK, k0:k0 + swa.BLOCK].all())
    for j0 in blocks:
        assert swa.query_blocks(j0, T, W) == [q0 for q0 in blocks if tile(q0, j0).any()]
    band, causal = swa.visited_blocks(T, W)
    assert band == sum(len(swa.key_blocks(q0, T, W)) for q0 in blocks) <= causal


@pytest.mark.parametrize("T,W,group,layout", [(9, 1, 1, "bhtd"), (9, 4, 2, "bthd"), (70, 17, 1, "bthd"), (70, 100, 4, "bthd")])
def test_the_composed_route_against_the_float64_rule(T, W, group, layout):
    q, k, v, do_ = ao.make_inputs(np.random.RandomState(T + W), layout, 2, 4, T, T, 8, 6)
    if group > 1:
        k, v = np.ascontiguousarray(k[:, :, :4 // group]), np.ascontiguousarray(v[:, :, :4 // group])
    qd, kd, vd, dod = (tn.asarray(a, dtype=np.float32) for a in (q, k, v, do_))
    o, lse = da.attention_swa(qd, kd, vd, W, layout=layout)
    dq, dk, dv = da.attention_swa_bwd(qd, kd, vd, o, dod, lse, W, layout=layout)
    res = so.reference(q, k, v, do_, W, layout, group)
    ao.check(dict(o=np.asarray(o), lse=np.asarray(lse), dq=np.asarray(dq), dk=np.asarray(dk), dv=np.asarray(dv)), res,
             "composed T %d W %d" % (T, W))


def test_the_refusals_come_before_any_launch(monkeypatch):
    q = Tensor(np.zeros((2, 8, 2, 4), dtype=np.float32))
    seen = gsup.count_calls(monkeypatch)
    lens = da.lengths([8, 3])
    k9 = Tensor(np.zeros((2, 9, 2, 4), dtype=np.float32))
    x = Tensor(np.zeros((2, 8, 8), dtype=np.float32))
    layer = MultiHeadAttention(2, num_in=8, causal=True, window=4)
    del seen[:]
    bthd = dict(causal=True, layout="bthd")
    for exc, match, call in (
            (ValueError, "causal=True", lambda: ops.attention_(q, q, q, layout="bthd", window=4)),
            (ValueError, "lens=", lambda: ops.attention_(q, q, q, window=4, lens=lens, **bthd)),
            (ValueError, "lens=", lambda: ops.attention_gqa_(q, q, q, causal=True, window=4, lens=lens)),
            (ValueError, "Tq == Tk", lambda: ops.attention_(q, k9, k9, window=4, **bthd)),
            (ValueError, ">= 1", lambda: ops.attention_(q, q, q, window=0, **bthd)),
            (TypeError, "integer", lambda: ops.attention_(q, q, q, window=2.5, **bthd)),
            (ValueError, "native", lambda: da.attention_swa(q.values, q.values, q.values, 4, route="native")),   # (the twin)
            (ValueError, "causal=True", lambda: MultiHeadAttention(2, num_in=8, window=4)),
            (ValueError, "causal=True", lambda: TransformerBlock(2, num_in=8, window=4)),
            (ValueError, "padded batch", lambda: layer.forward(x, lens=lens))):
        with pytest.raises(exc, match=match):
            call()
    assert seen == []


def test_window_none_is_the_path_as_it_was(monkeypatch):
    x = Tensor(np.random.RandomState(0).randn(2, 8, 8).astype(np.float32))
    ops.attention_(x, x, x, causal=True)                  # (uploads the causal mask once, outside the count)
    seen = gsup.count_calls(monkeypatch)
    direct = ops.attention_(x, x, x, causal=True)
    calls = list(seen)
    del seen[:]
    same = ops.attention_(x, x, x, causal=True, window=None)
    assert seen == calls and not [c for c in calls if c.startswith("swa_")]
    assert np.array_equal(np.asarray(same.values), np.asarray(direct.values))


def ring_lm(window, seed=1, fused=True):
    """Two causal blocks with rope, kv_heads = 2 and a window over 11 tokens; seed 1: smallest top-2 margin 0.17 (composed)."""
    import token_support as ts
    from tinynn_autograd_amd.core.layers import Dense, Embedding, LayerNorm
    from tinynn_autograd_amd.core.nn import Net
    from tinynn_autograd_amd.rope import Rotary
    rot, rs = Rotary(32), np.random.RandomState(seed)
    net = Net([Embedding(11, 16, fused=fused)] +
              [TransformerBlock(4, hidden=32, num_in=16, causal=True, fused=fused, kv_heads=2, rope=rot, window=window) for _ in range(2)] +
              [LayerNorm(16, fused=fused), ts.load_example().Rows(), Dense(11, num_in=16, fused=fused)])
    scale = lambda n, p: (1.0 if len(p.shape) == 2 and p.shape[0] > 1 else 0.1)
    net.set_parameters([{n: Tensor((rs.randn(*p.shape) * scale(n, p) + (1.0 if n.endswith("gamma") else 0.0)).astype(np.float32),
                                   requires_grad=True) for n, p in layer.items()} for layer in net.get_parameters()])
    return net, rs.randint(0, 11, (2, 9)).astype(np.int64)


def test_the_ring_cache_generates_what_the_whole_prefix_does():
    """window = 5, 9 + 12 tokens: LayerCache's ring (host emulation) against the whole growing prefix, uniform and ragged."""
    from tinynn_autograd_amd.generation import KVCache, generate
    net, prompt = ring_lm(5)
    want = generate(net, prompt, 12, temperature=0.0, cache=False)
    assert min(gsup.lm_margin(net, want[:, :n]) for n in range(9, 21)) > 0.05
    assert np.array_equal(generate(net, prompt, 12, temperature=0.0), want)
    ragged = generate(net, prompt, 12, temperature=0.0, prompt_lens=[9, 6])
    short = generate(net, prompt[1:, :6], 12, temperature=0.0, cache=False)
    assert np.array_equal(ragged[0], want[0]) and np.array_equal(ragged[1, :18], short[0])
    for bad in (dict(cache=KVCache(21, quant="int8")), dict(prefill_chunk=4)):        # refused before any launch
        with pytest.raises(ValueError, match="window"):
            generate(net, prompt, 12, temperature=0.0, **bad)


@pytest.mark.parametrize("T,R,lens", [(3, 5, None), (5, 5, None), (9, 5, None), (9, 5, (9, 6, 0)), (4, 1, (1, 4, 3))])
def test_the_ring_fill_and_step_on_the_composed_route(T, R, lens):
    rs, B = np.random.RandomState(T + R), 3
    k, v = rs.randn(B, T + 1, 2, 4).astype(np.float32), rs.randn(B, T + 1, 2, 6).astype(np.float32)
    ld = None if lens is None else da.lengths(list(lens))
    kr, vr = da.swa_fill(tn.asarray(k[:, :T]), tn.asarray(v[:, :T]), R, lens=ld)
    q = rs.randn(B, 4, 4).astype(np.float32)
    for b, n in enumerate(lens or (T,) * B):
        assert np.array_equal(np.asarray(kr)[b:b + 1], so.ring_of(k[b:b + 1], n, R)) and np.array_equal(np.asarray(vr)[b:b + 1], so.ring_of(v[b:b + 1], n, R))
        hk, hv = k[b:b + 1, :n + 1].copy(), v[b:b + 1, :n + 1].copy()
        hk[:, n], hv[:, n] = k[b:b + 1, T], v[b:b + 1, T]                    # the step's row at position n
        o = da.attention_decode_swa(tn.asarray(q[b:b + 1]), kr[b:b + 1], vr[b:b + 1], tn.asarray(k[b:b + 1, T]), tn.asarray(v[b:b + 1, T]), pos=n)
        np.testing.assert_allclose(np.asarray(o), so.decode(q[b:b + 1], hk[:, max(0, n + 1 - R):], hv[:, max(0, n + 1 - R):], 2), rtol=1e-5, atol=1e-6)
        assert np.array_equal(np.asarray(kr)[b:b + 1], so.ring_of(hk, n + 1, R))
