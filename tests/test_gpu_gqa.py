"""csrc/tnn_gqa.hip on the MI355X: grouped-query attention against the float64 oracle (tests/gqa_oracle.py) under its DERIVED
bounds and against the composed route under the sum of both; the appended row and the untouched cache rows bit for bit, NaN
beyond the live prefix never read, identical bits on a repeated call, the ragged call bit-equal to the uniform one sequence by
sequence, Hkv == H bit-equal to the multi-head entry points, and generation end to end.  Shapes are the smallest at which a
path can go wrong: one element, sizes around the 64-row block and the 64-key chunk, more than one block, head dimensions on
both sides of the tiles and of the 16-byte pack, groups 1, 2, 3 (no power of two: a spare query state), 4 and 8."""

import numpy as np
import pytest

import gqa_oracle as go
import gqa_support as gs
import tinynn_autograd_amd as tn
from tinynn_autograd_amd import _lib, decoding as dc, device_array as da, generation as gen, gqa, ragged as rg

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
bits = gs.bits


@pytest.fixture(scope="module")
def golden():
    return gs.load_golden()


def test_backend_and_entry_points():
    lib = _lib.get()
    assert tn.backend_name() == "hip-gfx950" and lib.has_gqa
    assert gqa.plan_gqa_attention((1, 4, 8, 8), (1, 4, 2, 8), (1, 4, 2, 8), native=lib.has_gqa).route == "native"
    o, _ = da.gqa_attention(tn.ones((1, 4, 8, 8)), tn.ones((1, 4, 2, 8)), tn.ones((1, 4, 2, 8)))
    np.testing.assert_array_equal(np.asarray(o), np.ones((1, 4, 8, 8), dtype=np.float32))


# ---------------------------------------------------------------------- training
def check_training(shape, causal, dtype, what, unaligned=False, need=(True, True, True), scale=None, res=None, inputs=None):
    """Native under the oracle's bounds, composed under the same bounds, the two within the sum; identical bits twice."""
    tn.set_default_float(dtype)
    b, h, hkv, tq, tk, d, dv = shape
    q, k, v, do_ = inputs or go.make_inputs(np.random.RandomState(go.case_seed(what)), b, h, hkv, tq, tk, d, dv, dtype)
    res = res or go.reference(q, k, v, do_, causal, scale, dtype)
    native = gs.run_training("native", q, k, v, do_, causal, scale, dtype, unaligned, need)
    for name, wanted in zip(("dq", "dk", "dv"), need):
        assert (native[name] is not None) == wanted, "%s %s" % (what, name)
    assert native["o"].dtype == dtype
    for name in ("dk", "dv"):
        if native[name] is not None:
            assert native[name].shape == (b, tk, hkv, d if name == "dk" else dv)
    go.check(native, res, what + " native")
    again = gs.run_training("native", q, k, v, do_, causal, scale, dtype, unaligned, need)
    for name in go.FIELDS:
        if native[name] is not None:
            assert np.array_equal(bits(native[name]), bits(again[name])), "%s %s: a repeated call gives other bits" % (what, name)
    composed = gs.run_training("composed", q, k, v, do_, causal, scale, dtype, False, need)
    go.check(composed, res, what + " composed")
    for name in go.FIELDS:
        if native[name] is not None:
            diff = np.abs(native[name].astype(np.float64) - composed[name].astype(np.float64))
            assert (diff <= 2 * res.bounds[name]).all(), "%s %s: the routes differ by more than both bounds" % (what, name)
    return native, (q, k, v, do_)


# (B, H, Hkv, Tq, Tk, D, Dv), causal: groups 1, 2, 3, 4, 8 over Hkv 1 and 2; Tq / Tk of 1, 63, 64, 65, 130, causal with
# Tq != Tk in both directions; the (D, Dv) pairs (3, 5), (16, 24), (65, 64), (128, 128)
TRAINING = [
    ((1, 1, 1, 1, 1, 3, 5), False), ((2, 2, 1, 63, 64, 3, 5), True), ((1, 3, 1, 65, 63, 16, 24), True),
    ((1, 4, 2, 64, 130, 16, 24), True), ((1, 4, 1, 130, 65, 3, 5), True), ((1, 8, 1, 65, 64, 16, 24), False),
    ((1, 16, 2, 1, 65, 3, 5), True), ((1, 2, 2, 64, 63, 65, 64), True), ((1, 6, 2, 63, 1, 65, 64), False),
    ((1, 2, 1, 65, 130, 128, 128), True), ((1, 8, 1, 64, 65, 128, 128), False),
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape, causal", TRAINING)
def test_training_shapes(shape, causal, dtype):
    what = "B%d H%d Hkv%d Tq%d Tk%d D%d Dv%d causal %d" % (shape + (causal,))
    check_training(shape, causal, dtype, what, unaligned=bool(sum(shape) & 1))


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_fixtures_cases(golden, dtype):
    for name, (b, h, hkv, tq, tk, d, dv, causal, scale) in go.GQA_CASES.items():
        if h // hkv > gqa.MAX_GROUP:
            continue                                           # (test_group_nine_is_refused_natively_and_composed)
        q, k, v, do_, causal, scale = go.case_input(name)
        res = go.reference(q, k, v, do_, causal, scale, dtype)
        for field in go.FIELDS:
            np.testing.assert_array_equal(res.values[field], golden["attn.%s.%s" % (name, field)])
        check_training((b, h, hkv, tq, tk, d, dv), causal, dtype, name, scale=scale, res=res, inputs=(q, k, v, do_))


@pytest.mark.parametrize("dtype", DTYPES)
def test_null_gradients_and_exact_zeros_for_unseen_keys(dtype):
    """dq / dk / dv skipped by NULL; causal with more keys than queries: keys from Tq on are seen by no query of ANY head of
    the group and get exact zeros (not merely small values), in both key blocks."""
    shape = (2, 6, 2, 5, 70, 16, 24)
    for need in ((False, True, True), (True, False, True), (True, True, False)):
        native, _ = check_training(shape, True, dtype, "need %s" % (need,), need=need)
    native, _ = check_training(shape, True, dtype, "unseen keys")
    for name in ("dk", "dv"):
        assert not bits(native[name][:, 5:]).any(), name
        assert native[name][:, :5].any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_group_nine_is_refused_natively_and_composed(dtype):
    tn.set_default_float(dtype)
    q, k, v, do_, causal, scale = go.case_input("group9_composed")
    res = go.reference(q, k, v, do_, causal, scale, dtype)
    with pytest.raises(ValueError, match="a group <= 8"):
        gs.run_training("native", q, k, v, do_, causal, scale, dtype)
    go.check(gs.run_training(None, q, k, v, do_, causal, scale, dtype), res, "group 9, the planner's route")
    lib = _lib.get()
    qd, kd, vd = (tn.asarray(a.astype(dtype)) for a in (q, k, v))
    o, lse = tn.zeros(q.shape[:3] + (v.shape[3],), dtype), tn.zeros((1, 9, 5), dtype)
    plan = gqa.plan_gqa_attention(q.shape, k.shape, v.shape, causal, scale, native=False)
    with pytest.raises(_lib.TnnError, match="exceeds TNN_GQA_MAX_GROUP"):
        lib.gqa_fwd(qd._ptr, kd._ptr, vd._ptr, o._ptr, lse._ptr, *plan.geometry(), da._i64arr(plan.strides("q", "k", "v", "o")),
                    plan.scale, 1, o._code())
    case = gs.make_decode_case(3, "bthd", 1, 9, 1, 70, 65, 8, 8, True, dtype)
    with pytest.raises(ValueError, match="a group <= 8"):
        gs.run_decode("native", case, dtype)
    o9, _, _ = gs.run_decode(None, case, dtype)
    ref = gs.decode_reference(case, dtype, 1)
    go.assert_within(o9, ref.values["o"], ref.bounds["o"], "group 9 decode, the planner's route")


# ---------------------------------------------------------------------- decode
def check_decode(case, dtype, splits, unaligned=False, what=""):
    """Native under the oracle's bound, composed under it too, the two within the sum; the caches bit for bit."""
    tn.set_default_float(dtype)
    plan = gqa.plan_gqa_decode(case["q"].shape, case["k_cache"].shape, case["v_cache"].shape, case["length"],
                               case["k_new"] is not None, layout=case["layout"], splits=splits)
    res = gs.decode_reference(case, dtype, plan.splits)
    o, kc, vc = gs.run_decode("native", case, dtype, splits, unaligned)
    assert o.dtype == dtype and np.isfinite(o).all(), what
    go.assert_within(o, res.values["o"], res.bounds["o"], "%s native" % what)
    want_k, want_v = gs.ds.expected_caches(case, dtype)
    assert np.array_equal(bits(kc), bits(want_k)) and np.array_equal(bits(vc), bits(want_v)), what
    o2, _, _ = gs.run_decode("native", case, dtype, splits, unaligned)
    assert np.array_equal(bits(o), bits(o2)), "%s: a repeated call gives other bits" % what
    oc, kcc, vcc = gs.run_decode("composed", case, dtype, None, unaligned)
    go.assert_within(oc, res.values["o"], res.bounds["o"], "%s composed" % what)
    assert np.array_equal(bits(kcc), bits(want_k)) and np.array_equal(bits(vcc), bits(want_v)), what
    assert (np.abs(o.astype(np.float64) - oc) <= 2 * res.bounds["o"]).all(), "%s native against composed" % what
    return plan


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("length", [0, 1, 63, 64, 65, 129, 199])
def test_decode_lengths_around_the_chunk(length, dtype):
    """Tmax 200; the planner's own split over B Hkv = 2 workgroup rows, both layouts, groups 2 and 3."""
    for layout, h in zip(dc.LAYOUTS, (4, 6)):
        case = gs.make_decode_case(go.case_seed("len%d%s" % (length, layout)), layout, 1, h, 2, 200, length, 16, 24, True, dtype)
        plan = check_decode(case, dtype, None, what="len %d %s" % (length, layout))
        assert plan.splits == plan.chunks == length // 64 + 1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("splits", [1, 2, 3, 5])
def test_decode_every_split_of_five_chunks(splits, dtype):
    case = gs.make_decode_case(go.case_seed("splits"), "bthd", 1, 8, 2, 320, 300, 64, 32, True, dtype)
    plan = check_decode(case, dtype, splits, what="splits %d" % splits)
    assert plan.chunks == 5 and plan.group == 4
    with pytest.raises(ValueError, match="splits 6 outside"):
        gs.run_decode("native", case, dtype, 6)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d,dv,b,h,hkv", [(1, 2, 1, 2, 1), (3, 5, 3, 3, 1), (4, 8, 1, 6, 3), (5, 3, 1, 8, 1), (16, 4, 3, 2, 1),
                                          (17, 16, 1, 12, 3), (64, 128, 1, 4, 1), (65, 64, 1, 6, 3), (128, 65, 3, 8, 1),
                                          (128, 128, 1, 8, 1)])
def test_decode_head_dimensions(d, dv, b, h, hkv, dtype):
    """The head-dimension list of tests/test_gpu_decode.py (wide accesses, element accesses with one and two packs per lane)
    plus (128, 128) at group 8, where the kernel holds the most state; 70 + 1 keys in two splits, both layouts."""
    for layout in dc.LAYOUTS:
        case = gs.make_decode_case(go.case_seed("dims%d.%d%s" % (d, dv, layout)), layout, b, h, hkv, 96, 70, d, dv, True, dtype)
        check_decode(case, dtype, 2, what="D %d Dv %d H %d Hkv %d %s" % (d, dv, h, hkv, layout))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", dc.LAYOUTS)
def test_decode_element_aligned_bases_and_no_append(layout, dtype):
    case = gs.make_decode_case(go.case_seed("unaligned" + layout), layout, 1, 6, 3, 96, 70, 16, 8, True, dtype)
    check_decode(case, dtype, 2, unaligned=True, what="unaligned %s" % layout)
    for length in (1, 64, 96):
        case = gs.make_decode_case(go.case_seed("null%d%s" % (length, layout)), layout, 3, 4, 1, 96, length, 16, 8, False, dtype)
        check_decode(case, dtype, None, what="no append, length %d %s" % (length, layout))
        check_decode(case, dtype, None, unaligned=True, what="no append, unaligned, length %d %s" % (length, layout))


@pytest.mark.parametrize("dtype", DTYPES)
def test_decode_fixture_cases(golden, dtype):
    for name in go.GQA_DECODE_CASES:
        case = go.decode_case(name)
        splits = case.pop("splits")
        check_decode(case, dtype, splits, what=name)
        np.testing.assert_array_equal(gs.decode_reference(case, dtype, splits).values["o"], golden["decode." + name])


# ---------------------------------------------------------------------- ragged
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", dc.LAYOUTS)
@pytest.mark.parametrize("splits", [1, 3])
def test_ragged_equals_the_uniform_call_per_sequence(splits, layout, dtype):
    """Every sequence bit-equal to tnn_gqa_decode_attn on that sequence alone with len = lens[b] and
    splits = min(splits, chunks_b); empty runs (a short sequence under a grid of 3 splits), invalid lengths: zeros, the
    caches untouched."""
    tn.set_default_float(dtype)
    lens = [0, 63, 64, 130, 199, -1, 200]
    case = gs.make_decode_case(go.case_seed("ragged" + layout), layout, len(lens), 6, 2, 200, 0, 16, 24, True, dtype)
    o, kc, vc = gs.run_decode("native", case, dtype, splits, lens=lens)
    o2, _, _ = gs.run_decode("native", case, dtype, splits, lens=lens)
    assert np.array_equal(bits(o), bits(o2))
    k_in, v_in = gs.ragged_poisoned(case, lens, dtype)
    for b, n in enumerate(lens):
        one = {key: (a[b:b + 1] if isinstance(a, np.ndarray) else a) for key, a in case.items()}
        if not 0 <= n < 200:
            assert not bits(o[b]).any()
            assert np.array_equal(bits(kc[b]), bits(k_in[b])) and np.array_equal(bits(vc[b]), bits(v_in[b])), \
                "an invalid length leaves the caches untouched"
            continue
        one["length"] = n
        ou, ku, vu = gs.run_decode("native", one, dtype, rg.effective_splits(n, splits))
        assert np.array_equal(bits(o[b:b + 1]), bits(ou)), "sequence %d (len %d)" % (b, n)
        assert np.array_equal(bits(kc[b:b + 1]), bits(ku)) and np.array_equal(bits(vc[b:b + 1]), bits(vu))
        res = gs.decode_reference(one, dtype, rg.effective_splits(n, splits))
        go.assert_within(o[b:b + 1], res.values["o"], res.bounds["o"], "ragged sequence %d" % b)


# ---------------------------------------------------------------------- group 1: the bits of the multi-head entry points
@pytest.mark.parametrize("dtype", DTYPES)
def test_group_one_gives_the_old_bits(dtype):
    tn.set_default_float(dtype)
    rs = np.random.RandomState(77)
    for (b, h, tq, tk, d, dv), causal in (((2, 3, 65, 70, 16, 24), True), ((1, 2, 9, 130, 65, 64), False)):
        q, k, v, do_ = go.make_inputs(rs, b, h, h, tq, tk, d, dv, dtype)
        new = gs.run_training("native", q, k, v, do_, causal, None, dtype)
        qd, kd, vd, dod = (gs.dev(a, dtype) for a in (q, k, v, do_))
        opts = dict(causal=causal, layout="bthd", route="native")
        o, lse = da.attention(qd, kd, vd, **opts)
        dq, delta = da.attention_bwd_q(qd, kd, vd, o, dod, lse, **opts)
        dk, dv_ = da.attention_bwd_kv(qd, kd, vd, dod, lse, delta, **opts)
        for name, old in (("o", o), ("lse", lse), ("dq", dq), ("dk", dk), ("dv", dv_)):
            assert np.array_equal(bits(new[name]), bits(np.asarray(old))), "tnn_gqa_* with Hkv == H: %s" % name
    for layout in dc.LAYOUTS:
        for d, dv, splits in ((16, 24, 2), (65, 3, 1), (128, 128, 3)):
            case = gs.make_decode_case(5, layout, 2, 3, 3, 200, 150, d, dv, True, dtype)
            o, kc, vc = gs.run_decode("native", case, dtype, splits)
            oo, ko, vo = gs.ds.run_decode("native", case, dtype, splits)
            assert np.array_equal(bits(o), bits(oo)) and np.array_equal(bits(kc), bits(ko)) and np.array_equal(bits(vc), bits(vo))
            lens = [150, 3]
            o, kc, vc = gs.run_decode("native", case, dtype, splits, lens=lens)
            kp, vp = gs.ragged_poisoned(case, lens, dtype)
            kd, vd = gs.dev(kp, dtype), gs.dev(vp, dtype)
            oo = da.attention_decode_ragged(gs.dev(case["q"], dtype), kd, vd, da.lengths(lens), gs.dev(case["k_new"], dtype),
                                            gs.dev(case["v_new"], dtype), layout=layout, route="native", splits=splits)
            assert np.array_equal(bits(o), bits(np.asarray(oo))) and np.array_equal(bits(kc), bits(np.asarray(kd)))
            assert np.array_equal(bits(vc), bits(np.asarray(vd)))


# ---------------------------------------------------------------------- end to end
def test_generation_with_grouped_heads(golden):
    """gqa_oracle's two-block model (4 query heads over 2 key / value heads), greedy: the ids with the cache equal the ids
    from recomputing the full forward at every step, the captured ragged ids equal the eager ragged ids, and all of them are
    the float64 oracle's — whose top-2 margin exceeds 2 x LM_MARGIN logit bounds at every step (checked when the fixture was
    generated and again here), so no float32 evaluation within LM_MARGIN bounds of it can pick another token."""
    c = go.LM
    seed, scale, bound = int(golden["lm.seed"]), float(golden["lm.head_scale"]), float(golden["lm.logit_bound"])
    params, prompt = go.lm_params(seed, scale), go.lm_prompt(seed)
    ids, steps = go.lm_generate(params, prompt, c["new"])
    srt = np.sort(steps, axis=-1)
    assert float((srt[..., -1] - srt[..., -2]).min()) > 2 * go.LM_MARGIN * bound and np.array_equal(ids, golden["lm.ids"])
    tn.set_default_float(np.float32)
    net = gs.lm_net(params, np.float32)
    for n in (0, c["new"] - 1):
        got = gs.lm_last_logits(net, ids[:, :c["prompt"] + n])
        assert np.abs(got - steps[n]).max() <= go.LM_MARGIN * bound, "step %d: %.3e" % (n, np.abs(got - steps[n]).max())
    cached = gen.generate(net, prompt, c["new"], temperature=0.0, cache=True)
    full = gen.generate(net, prompt, c["new"], temperature=0.0, cache=False)
    assert np.array_equal(cached, full) and np.array_equal(cached, ids)
    lens = np.full((c["B"],), c["prompt"], dtype=np.int64)
    eager = gen.generate(net, prompt, c["new"], temperature=0.0, prompt_lens=lens)
    captured = gen.generate(net, prompt, c["new"], temperature=0.0, prompt_lens=lens, capture=True)
    assert np.array_equal(np.asarray(eager), np.asarray(captured)) and np.array_equal(np.asarray(eager), ids)
    caches = [l.kv_heads for l in net.layers if hasattr(l, "kv_heads")]
    assert caches == [c["Hkv"]] * c["blocks"]
