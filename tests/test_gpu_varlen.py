"""csrc/tnn_varlen.hip on the MI355X: training attention with per-sequence lengths.  Native under the per-sequence oracle's
derived bounds, composed under them, the two routes within twice the bound; every dead element exactly +0; NaN in every dead
row of q, k, v, o and dO reaches no output and changes no bit; every sequence's live rows bit for bit those of tnn_attn_* /
tnn_gqa_* on that sequence alone; head dimensions over every NT and the element path; groups and the need_* switches;
identical bits on a repeated call; a captured forward that follows new contents of the lengths on replay; a two-block model on
both routes.  The shapes are the smallest at which a path can go wrong: T = 130 is three 64-row blocks with a ragged last one,
and the lengths sit on both sides of a block edge."""

import numpy as np
import pytest

import attn_oracle as ao
import gqa_oracle as go
import gqa_support as gs
import token_support as ts
import varlen_support as vs
import tinynn_autograd_amd as tn
from tinynn_autograd_amd import device_array as da
from tinynn_autograd_amd.core.layers import Dense, Embedding, LayerNorm, TransformerBlock
from tinynn_autograd_amd.core.losses import CrossEntropyLoss
from tinynn_autograd_amd.core.nn import Net
from tinynn_autograd_amd.core.tensor import Tensor
from tinynn_autograd_amd.rope import Rotary

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
T, LENS = 130, (0, 1, 63, 64, 65, 130)
NAMES = ("o", "lse", "delta", "dq", "dk", "dv")
_CACHE = {}


@pytest.fixture(autouse=True)
def _switches():
    yield
    da.VARLEN_ROUTE = None
    tn.set_default_float(np.float32)


def block_case(layout, causal, dtype):
    """Inputs, oracle and the native result of the 'lengths around the block' case: computed once, shared, never modified."""
    key = (layout, causal, np.dtype(dtype).name)
    if key not in _CACHE:
        h = 2 if layout == "bthd" else 1
        q, k, v, do_ = vs.make_inputs(ao.case_seed("block" + layout), layout, len(LENS), h, h, T, 16, 24, dtype)
        res = vs.reference(q, k, v, do_, LENS, causal, None, layout, dtype)
        tn.set_default_float(dtype)
        native = vs.run("native", q, k, v, do_, LENS, causal, None, layout, dtype)
        _CACHE[key] = ((q, k, v, do_), res, native)
    return _CACHE[key]


def same_bits(a, b, what):
    for name in a:
        if a[name] is None:
            assert b[name] is None, name
            continue
        assert np.array_equal(vs.bits(a[name]), vs.bits(b[name])), "%s: %s differs" % (what, name)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("layout", ["bthd", "bhtd"])
def test_lengths_around_the_block(layout, causal, dtype):
    tn.set_default_float(dtype)
    (q, k, v, do_), res, native = block_case(layout, causal, dtype)
    what = "%s causal %s %s" % (layout, causal, np.dtype(dtype).name)
    assert all(a.dtype == dtype for a in native.values())
    vs.check(native, res, what + " native", verbose=True)
    vs.assert_dead_are_plus_zero(native, LENS, layout, what + " native")
    composed = vs.run("composed", q, k, v, do_, LENS, causal, None, layout, dtype)
    vs.check(composed, res, what + " composed")
    vs.assert_dead_are_plus_zero(composed, LENS, layout, what + " composed")
    for name in NAMES:
        gap = np.abs(native[name].astype(np.float64) - composed[name])
        assert (gap <= 2 * res.bounds[name]).all(), "%s %s: the routes differ by more than twice the bound" % (what, name)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("layout", ["bthd", "bhtd"])
def test_poisoned_padding(layout, causal, dtype):
    """NaN in every dead row of q, k, v, dO — and of o, between the forward and the backward — is never read."""
    tn.set_default_float(dtype)
    (q, k, v, do_), _, native = block_case(layout, causal, dtype)
    pq, pk, pv, pdo = vs.poisoned((q, k, v, do_), LENS, layout)
    assert np.isnan(pq).any() and np.isnan(pdo).any()
    got = vs.run("native", pq, pk, pv, pdo, LENS, causal, None, layout, dtype, o_poison=True)
    assert all(np.isfinite(a).all() for a in got.values())
    same_bits(native, got, "poisoned %s causal %s" % (layout, causal))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hkv", [2, 1])
def test_a_sequence_alone(hkv, dtype):
    """The live rows of every sequence equal, bit for bit, tnn_gqa_* on that sequence cut to lens[b] rows (Hkv == H: the bits of
    tnn_attn_*, which the plain functions are run for as well)."""
    tn.set_default_float(dtype)
    lens = (1, 63, 64, 65, 130)
    q, k, v, do_ = vs.make_inputs(ao.case_seed("alone%d" % hkv), "bthd", len(lens), 2, hkv, T, 16, 24, dtype)
    for causal in (False, True):
        got = vs.run("native", q, k, v, do_, lens, causal, None, "bthd", dtype)
        for b, n in enumerate(lens):
            cut = [a[b:b + 1, :n] for a in (q, k, v, do_)]
            alone = gs.run_training("native", *cut, causal, None, dtype)
            for name in ("o", "dq", "dk", "dv"):
                assert np.array_equal(vs.bits(got[name][b:b + 1, :n]), vs.bits(alone[name])), (name, b, n, causal)
            assert np.array_equal(vs.bits(got["lse"][b:b + 1, :, :n]), vs.bits(alone["lse"])), ("lse", b, n, causal)
            if hkv == 2:
                qd, kd, vd, dod = (tn.asarray(a, dtype=dtype) for a in cut)
                o, lse = da.attention(qd, kd, vd, causal=causal, layout="bthd", route="native")
                dq, delta = da.attention_bwd_q(qd, kd, vd, o, dod, lse, causal=causal, layout="bthd", route="native")
                dk, dv = da.attention_bwd_kv(qd, kd, vd, dod, lse, delta, causal=causal, layout="bthd", route="native")
                for name, a in (("o", o), ("dq", dq), ("dk", dk), ("dv", dv)):
                    assert np.array_equal(vs.bits(got[name][b:b + 1, :n]), vs.bits(np.asarray(a))), ("plain " + name, b, n, causal)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dims", [(5, 3), (16, 24), (40, 40), (72, 40), (128, 128)])
def test_head_dimensions(dims, dtype):
    """Every NT (1, 2, 4, 8) and the element path (D = 5, Dv = 3: no 16-byte accesses), T = 70 past one block, and an
    unaligned operand view."""
    tn.set_default_float(dtype)
    d, dv = dims
    lens = (70, 37)
    q, k, v, do_ = vs.make_inputs(ao.case_seed("dims%d" % d), "bthd", 2, 2, 2, 70, d, dv, dtype)
    res = vs.reference(q, k, v, do_, lens, True, None, "bthd", dtype)
    for unaligned in (False, True):
        got = vs.run("native", q, k, v, do_, lens, True, None, "bthd", dtype, unaligned=unaligned)
        what = "D %d Dv %d unaligned %s" % (d, dv, unaligned)
        vs.check(got, res, what)
        vs.assert_dead_are_plus_zero(got, lens, "bthd", what)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hkv", [4, 2, 1])
def test_groups_and_the_need_switches(hkv, dtype):
    tn.set_default_float(dtype)
    lens = (70, 37, 0)
    q, k, v, do_ = vs.make_inputs(ao.case_seed("groups%d" % hkv), "bthd", 3, 4, hkv, 70, 16, 24, dtype)
    res = vs.reference(q, k, v, do_, lens, True, None, "bthd", dtype)
    full = vs.run("native", q, k, v, do_, lens, True, None, "bthd", dtype)
    vs.check(full, res, "Hkv %d" % hkv)
    vs.assert_dead_are_plus_zero(full, lens, "bthd", "Hkv %d" % hkv)
    for need in ((False, True, True), (True, False, True), (True, True, False)):
        got = vs.run("native", q, k, v, do_, lens, True, None, "bthd", dtype, need=need)
        for name, wanted in zip(("dq", "dk", "dv"), need):
            assert (got[name] is None) == (not wanted), (name, need)
            got[name] = got[name] if wanted else None
        same_bits({n: a for n, a in got.items() if a is not None}, full, "need %s" % (need,))


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_repeated_call_gives_identical_bits(dtype):
    tn.set_default_float(dtype)
    (q, k, v, do_), _, native = block_case("bthd", True, dtype)
    same_bits(native, vs.run("native", q, k, v, do_, LENS, True, None, "bthd", dtype), "repeat")


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_captured_forward_follows_the_lengths(dtype):
    """The lengths are read on the device: one recording serves new contents of the array."""
    tn.set_default_float(dtype)
    first, second = (70, 37, 1), (5, 70, 64)
    q, k, v, do_ = vs.make_inputs(ao.case_seed("capture"), "bthd", 3, 2, 1, 70, 16, 24, dtype)
    qd, kd, vd = (tn.asarray(a, dtype=dtype) for a in (q, k, v))
    ld = tn.asarray(np.array(first, dtype=np.int64))
    step = tn.capture(lambda: da.gqa_attention(qd, kd, vd, causal=True, route="native", lens=ld), warmup=1)
    for lens in (first, second, first):
        ld[...] = tn.asarray(np.array(lens, dtype=np.int64))
        o, lse = step()
        res = vs.reference(q, k, v, do_, lens, True, None, "bthd", dtype)
        got = dict(o=np.asarray(o), lse=np.asarray(lse))
        vs.check(got, res, "replay lens %s" % (lens,), fields=("o", "lse"))
        vs.assert_dead_are_plus_zero(got, lens, "bthd", "replay")


def _lm(kv_heads, rope, fused, dtype, params=None):
    """Embedding, two causal blocks, a norm and a head over a vocabulary of 11; params: another net's, copied."""
    width, seq = 16, 70
    rotary = Rotary(seq) if rope else None
    rows = ts.load_example().Rows
    net = Net([Embedding(11, width, max_len=None if rope else seq, fused=fused)] +
              [TransformerBlock(4, hidden=32, num_in=width, causal=True, fused=fused, kv_heads=kv_heads, rope=rotary) for _ in range(2)] +
              [LayerNorm(width, fused=fused), rows(), Dense(11, num_in=width, fused=fused)])
    if params is None:
        rs = np.random.RandomState(3)
        params = [{n: rs.uniform(-0.4, 0.4, tuple(p.shape)) + (1.0 if n.endswith("gamma") else 0.0) for n, p in layer.items()}
                  for layer in net.get_parameters()]
    net.set_parameters([{n: Tensor(a.astype(dtype), requires_grad=True, dtype=dtype) for n, a in layer.items()} for layer in params])
    return net, params


def _loss_and_grads(net, ids, targets, lens, fused, dtype):
    tn.set_default_float(dtype)
    for p in net.parameter_tensors():
        p.zero_grad()
    loss = CrossEntropyLoss(ignore_index=-1, fused=fused).loss(net.forward(Tensor(ids), lens=da.lengths(lens)), targets)
    loss.backward()
    return float(np.asarray(loss.values)), np.concatenate([np.asarray(p.grad, dtype=np.float64).ravel() for p in net.parameter_tensors()])


@pytest.mark.parametrize("kv_heads,rope", [(2, True), (None, False)])
def test_a_two_block_model_on_both_routes(kv_heads, rope):
    """Loss and gradients of one padded batch (targets at dead positions ignored): float32 native against float32 composed,
    both judged against the float64 evaluation of the composed route.  The bound is the composed route's OWN float32 error,
    taken over the whole gradient, times gqa_oracle.LM_MARGIN (two float32 evaluations whose summation orders differ)."""
    lens = (70, 37, 5)
    rs = np.random.RandomState(21)
    ids = rs.randint(0, 11, (3, 70)).astype(np.int64)
    targets = rs.randint(0, 11, (3, 70)).astype(np.int64)
    for b, n in enumerate(lens):
        targets[b, n:] = -1
    targets = targets.reshape(-1)
    ref_net, params = _lm(kv_heads, rope, False, np.float64)
    loss64, grad64 = _loss_and_grads(ref_net, ids, targets, lens, False, np.float64)
    loss_c, grad_c = _loss_and_grads(_lm(kv_heads, rope, False, np.float32, params)[0], ids, targets, lens, False, np.float32)
    loss_n, grad_n = _loss_and_grads(_lm(kv_heads, rope, True, np.float32, params)[0], ids, targets, lens, True, np.float32)
    own_l, own_g = abs(loss_c - loss64), np.abs(grad_c - grad64).max()
    print("loss: float64 %.9f, composed %.3e off, native %.3e off; gradients: composed %.3e off, native %.3e off (max |g| %.3e)"
          % (loss64, own_l, abs(loss_n - loss64), own_g, np.abs(grad_n - grad64).max(), np.abs(grad64).max()))
    assert np.isfinite(grad_n).all() and np.abs(grad64).max() > 0
    assert abs(loss_n - loss64) <= go.LM_MARGIN * max(own_l, ao.U32 * abs(loss64))
    assert np.abs(grad_n - grad64).max() <= go.LM_MARGIN * own_g
