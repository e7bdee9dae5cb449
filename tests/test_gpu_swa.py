"""csrc/tnn_swa.hip on the MI355X: forward, dq, dk and dv against the float64 rule (tests/swa_oracle.py) under the bounds of
tests/attn_oracle.py with the row's kept-key count in place of Tk; every output finite (W < 64 with T > 64: rows whose first
visited block is wholly masked); for W >= T the bits of the causal kernels; NaN in a key block outside the walk; a two-block
model against the composed route.  T on both sides of one and two block edges, W = 1 (the diagonal alone), 63 / 64 / 65
around the block, 129 with an interior block, NT = 1, 4, 8, groups 1, 2, 4, both layouts."""

import numpy as np
import pytest

import attn_oracle as ao
import gqa_oracle as go
import swa_oracle as so
import token_support as ts
import tinynn_autograd_amd as tn
from tinynn_autograd_amd import device_array as da
from tinynn_autograd_amd.core.layers import Dense, Embedding, LayerNorm, TransformerBlock
from tinynn_autograd_amd.core.losses import CrossEntropyLoss
from tinynn_autograd_amd.core.nn import Net
from tinynn_autograd_amd.core.tensor import Tensor
from tinynn_autograd_amd.rope import Rotary

pytestmark = pytest.mark.gpu
B, H, NAMES = 2, 4, ("o", "lse", "dq", "dk", "dv")
CASES = [                                         # (T, W, D, Dv, group, layout): every value at least once, not the product
    (1, 1, 8, 8, 1, "bhtd"), (1, 64, 40, 24, 2, "bthd"),
    (63, 1, 8, 8, 1, "bthd"), (63, 17, 40, 24, 4, "bthd"), (63, 64, 128, 128, 1, "bhtd"),
    (65, 2, 8, 8, 2, "bthd"), (65, 63, 40, 24, 1, "bhtd"), (65, 64, 8, 8, 4, "bthd"), (65, 65, 128, 128, 2, "bthd"),
    (65, 129, 40, 24, 1, "bthd"),
    (130, 1, 40, 24, 1, "bhtd"), (130, 2, 8, 8, 1, "bthd"), (130, 17, 128, 128, 4, "bthd"), (130, 63, 8, 8, 2, "bthd"),
    (130, 64, 40, 24, 1, "bthd"), (130, 65, 8, 8, 1, "bhtd"), (130, 129, 40, 24, 2, "bthd"),
    (200, 1, 8, 8, 4, "bthd"), (200, 17, 40, 24, 1, "bhtd"), (200, 63, 128, 128, 1, "bthd"), (200, 64, 8, 8, 2, "bthd"),
    (200, 65, 40, 24, 4, "bthd"), (200, 129, 8, 8, 1, "bhtd"), (200, 129, 128, 128, 2, "bthd"),
]


def inputs(name, T, D, Dv, group, layout):
    q, k, v, do_ = ao.make_inputs(np.random.RandomState(ao.case_seed(name)), layout, B, H, T, T, D, Dv)
    if group > 1:
        k, v = np.ascontiguousarray(k[:, :, :H // group]), np.ascontiguousarray(v[:, :, :H // group])
    return q, k, v, do_


def run(q, k, v, do_, W, layout, group=1):
    """The native launches; W None: the causal kernels (tnn_attn_* for plain heads, tnn_gqa_* for grouped ones)."""
    qd, kd, vd, dod = (tn.asarray(a, dtype=np.float32) for a in (q, k, v, do_))
    if W is not None:
        o, lse = da.attention_swa(qd, kd, vd, W, layout=layout, route="native")
        dq, dk, dv = da.attention_swa_bwd(qd, kd, vd, o, dod, lse, W, layout=layout, route="native")
    else:
        fwd, bwd_q, bwd_kv = ((da.attention, da.attention_bwd_q, da.attention_bwd_kv) if group == 1 else
                              (da.gqa_attention, da.gqa_attention_bwd_q, da.gqa_attention_bwd_kv))
        opts = dict(causal=True, route="native", **(dict(layout=layout) if group == 1 else {}))
        o, lse = fwd(qd, kd, vd, **opts)
        dq, delta = bwd_q(qd, kd, vd, o, dod, lse, **opts)
        dk, dv = bwd_kv(qd, kd, vd, dod, lse, delta, **opts)
    return {n: np.asarray(a) for n, a in zip(NAMES, (o, lse, dq, dk, dv))}


@pytest.mark.parametrize("T,W,D,Dv,group,layout", CASES)
def test_against_the_float64_rule(T, W, D, Dv, group, layout):
    q, k, v, do_ = inputs("swa%d_%d" % (T, W), T, D, Dv, group, layout)
    got = run(q, k, v, do_, W, layout, group)
    for name in NAMES:                            # on its own: an all-NaN row would else read as a tolerance failure
        assert np.isfinite(got[name]).all(), "%s holds a non-finite value" % name
    res = so.reference(q, k, v, do_, W, layout, group)
    ao.check(got, res, "T %d W %d D %d/%d group %d %s" % (T, W, D, Dv, group, layout), verbose=True)


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("extra", [0, 7])
@pytest.mark.parametrize("T", [65, 130])
def test_a_window_of_the_whole_sequence_has_the_causal_bits(T, extra, group):
    q, k, v, do_ = inputs("bits%d" % T, T, 40, 24, group, "bthd")
    got, want = run(q, k, v, do_, T + extra, "bthd"), run(q, k, v, do_, None, "bthd", group)
    for name in NAMES:
        assert np.array_equal(got[name].view(np.uint32), want[name].view(np.uint32)), name


def test_a_key_block_outside_the_walk_is_never_read():
    """T = 200, W = 17: rows from 128 on visit key blocks 64 and 128 only; NaN in rows 0 .. 63 of k and v changes no bit there."""
    T, W = 200, 17
    q, k, v, do_ = inputs("poison", T, 40, 24, 2, "bthd")
    clean = run(q, k, v, do_, W, "bthd")
    pk, pv = k.copy(), v.copy()
    pk[:, :64], pv[:, :64] = np.nan, np.nan
    got = run(q, pk, pv, do_, W, "bthd")
    for name in NAMES:
        a, b = (x[:, :, 128:] if name == "lse" else x[:, 128:] for x in (got[name], clean[name]))
        assert np.isfinite(a).all() and np.array_equal(a.view(np.uint32), b.view(np.uint32)), name


def _lm(window, fused, dtype, params=None):
    width, seq = 16, 70
    rows = ts.load_example().Rows
    net = Net([Embedding(11, width, fused=fused)] +
              [TransformerBlock(4, hidden=32, num_in=width, causal=True, fused=fused, kv_heads=2, rope=Rotary(seq), window=window)
               for _ in range(2)] + [LayerNorm(width, fused=fused), rows(), Dense(11, num_in=width, fused=fused)])
    if params is None:
        rs = np.random.RandomState(3)
        params = [{n: rs.uniform(-0.4, 0.4, tuple(p.shape)) + (1.0 if n.endswith("gamma") else 0.0) for n, p in layer.items()}
                  for layer in net.get_parameters()]
    net.set_parameters([{n: Tensor(a.astype(dtype), requires_grad=True, dtype=dtype) for n, a in layer.items()} for layer in params])
    return net, params


def _loss_and_grads(net, ids, targets, fused, dtype):
    tn.set_default_float(dtype)
    for p in net.parameter_tensors():
        p.zero_grad()
    loss = CrossEntropyLoss(fused=fused).loss(net.forward(Tensor(ids)), targets)
    loss.backward()
    return float(np.asarray(loss.values)), np.concatenate([np.asarray(p.grad, dtype=np.float64).ravel() for p in net.parameter_tensors()])


def test_a_training_step_of_a_two_block_model():
    """Loss and gradients with window = 17 over 70 tokens: float32 native against the float64 composed route.  The bound is
    the composed route's OWN float32 error times gqa_oracle.LM_MARGIN, as for the other attention families."""
    rs = np.random.RandomState(21)
    ids = rs.randint(0, 11, (3, 70)).astype(np.int64)
    targets = rs.randint(0, 11, (3 * 70,)).astype(np.int64)
    ref_net, params = _lm(17, False, np.float64)
    loss64, grad64 = _loss_and_grads(ref_net, ids, targets, False, np.float64)
    loss_c, grad_c = _loss_and_grads(_lm(17, False, np.float32, params)[0], ids, targets, False, np.float32)
    loss_n, grad_n = _loss_and_grads(_lm(17, True, np.float32, params)[0], ids, targets, True, np.float32)     # (ends in float32)
    own_l, own_g = abs(loss_c - loss64), np.abs(grad_c - grad64).max()
    print("loss: float64 %.9f, composed %.3e off, native %.3e off; gradients: composed %.3e off, native %.3e off"
          % (loss64, own_l, abs(loss_n - loss64), own_g, np.abs(grad_n - grad64).max()))
    assert np.isfinite(grad_n).all() and np.abs(grad64).max() > 0
    assert abs(loss_n - loss64) <= go.LM_MARGIN * max(own_l, ao.U32 * abs(loss64))
    assert np.abs(grad_n - grad64).max() <= go.LM_MARGIN * own_g


@pytest.mark.parametrize("group", [1, 4])
@pytest.mark.parametrize("R", [1, 5, 64, 70, 200])
def test_ring_decode(R, group):
    """Before the wrap, on it and after several turns; splits 1 and the most; host and per-sequence device positions: o against
    float64 over the explicit last R rows, the ring afterwards, and for p < R the bits of the linear decode ops.  Bound: twice the
    error of the EXISTING decode op over the same rows in linear order (measured: existing <= 3.07e-6, ring <= 2.95e-6)."""
    D, Dv, hkv, rs = 40, 24, H // group, np.random.RandomState(R + group)
    most = min(-(-R // 64), 256)
    for pos in sorted({R // 2, R - 1, R, 3 * R + 2}):
        hk, hv = rs.randn(B, pos + 1, hkv, D).astype(np.float32), (3 * rs.randn(B, pos + 1, hkv, Dv)).astype(np.float32)
        q = (2 * rs.randn(B, H, D)).astype(np.float32)
        for ps in ((pos, pos), (pos, max(pos - 2, 0))):            # (host position; device positions)
            rows = [slice(max(0, p + 1 - R), p + 1) for p in ps]
            want = np.concatenate([so.decode(q[b:b + 1], hk[b:b + 1, rows[b]], hv[b:b + 1, rows[b]], group) for b in range(B)])
            kn, vn = (np.stack([h[b, p] for b, p in enumerate(ps)]) for h in (hk, hv))
            before = [np.concatenate([so.ring_of(h[b:b + 1], p, R) for b, p in enumerate(ps)]) for h in (hk, hv)]
            after = [r.copy() for r in before]
            for b, p in enumerate(ps):
                after[0][b, p % R], after[1][b, p % R] = kn[b], vn[b]
            where = dict(pos=pos) if ps[0] == ps[1] else dict(lens=da.lengths(list(ps)))
            lin = [np.concatenate([np.pad(h[b:b + 1, rows[b]], ((0, 0), (0, R + 1 - (rows[b].stop - rows[b].start)), (0, 0), (0, 0)))
                                   for b in range(B)]) for h in (hk, hv)]          # the same rows in linear order, the step's last
            n = [rows[b].stop - rows[b].start - 1 for b in range(B)]
            ref = np.asarray(da.gqa_decode(tn.asarray(q), tn.asarray(lin[0]), tn.asarray(lin[1]), k_new=tn.asarray(kn), v_new=tn.asarray(vn),
                                           route="native", **(dict(length=n[0]) if n[0] == n[1] else dict(lens=da.lengths(n)))))
            bound = 2 * max(np.abs(ref - want).max(), ao.U32 * np.abs(want).max())
            for splits in sorted({1, most}):
                kr, vr = tn.asarray(before[0]), tn.asarray(before[1])
                got = np.asarray(da.attention_decode_swa(tn.asarray(q), kr, vr, tn.asarray(kn), tn.asarray(vn), route="native", splits=splits, **where))
                print("R %d group %d pos %s splits %d: existing %.2e off, ring %.2e off" % (R, group, ps, splits, np.abs(ref - want).max(), np.abs(got - want).max()))
                assert np.isfinite(got).all() and np.abs(got - want).max() <= bound
                assert np.array_equal(np.asarray(kr), after[0]) and np.array_equal(np.asarray(vr), after[1])
                if max(ps) < R and splits <= -(-(min(ps) + 1) // 64):       # not wrapped: the linear ops on the same cache
                    old = dict(length=pos) if "pos" in where else where
                    same = da.gqa_decode(tn.asarray(q), tn.asarray(before[0]), tn.asarray(before[1]), k_new=tn.asarray(kn),
                                         v_new=tn.asarray(vn), route="native", splits=splits, **old)
                    assert np.array_equal(np.asarray(same).view(np.uint32), got.view(np.uint32)), (pos, splits)


@pytest.mark.parametrize("T,R,lens", [(3, 5, None), (5, 5, None), (9, 5, None), (130, 70, (130, 64, 0)), (4, 1, (1, 4, 3)), (70, 200, (7, 70, 1))])
def test_ring_fill(T, R, lens):
    rs, b = np.random.RandomState(T + R), 3
    k, v = rs.randn(b, T, 2, 40).astype(np.float32), rs.randn(b, T, 2, 3).astype(np.float32)
    kr, vr = da.swa_fill(tn.asarray(k), tn.asarray(v), R, lens=None if lens is None else da.lengths(list(lens)), route="native")
    for i, n in enumerate(lens or (T,) * b):
        assert np.array_equal(np.asarray(kr)[i:i + 1], so.ring_of(k[i:i + 1], n, R)) and np.array_equal(np.asarray(vr)[i:i + 1], so.ring_of(v[i:i + 1], n, R))


def test_generation_through_the_ring():
    """window = 5, 9 + 12 greedy tokens: the ring against the whole growing prefix — uniform, and ragged through the captured step."""
    from test_swa_host import ring_lm
    from tinynn_autograd_amd.generation import generate
    net, prompt = ring_lm(5)
    want = generate(net, prompt, 12, temperature=0.0, cache=False)
    assert np.array_equal(generate(net, prompt, 12, temperature=0.0), want)
    ragged = generate(net, prompt, 12, temperature=0.0, prompt_lens=[9, 6], capture=True)
    short = generate(net, prompt[1:, :6], 12, temperature=0.0, cache=False)
    assert np.array_equal(ragged[0], want[0]) and np.array_equal(ragged[1, :18], short[0])
