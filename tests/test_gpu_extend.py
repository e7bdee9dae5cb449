"""csrc/tnn_extend.hip on the MI355X: cache-extending attention native against the float64 oracle under its derived bounds and
against the composed route under twice the bound, the appended rows bit for bit, nothing else written, NaN beyond the live
rows never read, identical bits on a repeated call — and identical bits however the rows are cut into calls.  Shapes are the
smallest at which a path can go wrong: lengths and row counts around the block of 64, every head-dimension tile, element and
unaligned accesses, every group size; then the layers and generation on the native route."""

import numpy as np
import pytest

import attn_oracle as ao
import decode_support as ds
import extend_oracle as eo
import extend_support as es
import tinynn_autograd_amd as tn
from tinynn_autograd_amd import _lib, device_array as da, extend as ex

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
EDGES = [0, 1, 63, 64, 65, 130]


@pytest.fixture(scope="module")
def golden():
    return ds.load_golden()


def check_extend(case, dtype, unaligned=False, what=""):
    """Native under the oracle's bound, composed under it too, the two within twice the bound; the caches bit for bit (the
    poisoned rows beyond length + T included); a repeated call gives the same bits."""
    tn.set_default_float(dtype)
    res = es.reference(case, dtype)
    o, kc, vc = es.run_extend("native", case, dtype, unaligned)
    assert o.dtype == dtype and o.shape == res.values["o"].shape and np.isfinite(o).all(), what
    ao.assert_within(o, res.values["o"], res.bounds["o"], "%s native" % what)
    want_k, want_v = es.expected_caches(case, dtype)
    assert np.array_equal(es.bits(kc), es.bits(want_k)) and np.array_equal(es.bits(vc), es.bits(want_v)), what
    o2, _, _ = es.run_extend("native", case, dtype, unaligned)
    assert np.array_equal(es.bits(o), es.bits(o2)), "%s: a repeated call gives other bits" % what
    oc, kcc, vcc = es.run_extend("composed", case, dtype, unaligned)
    ao.assert_within(oc, res.values["o"], res.bounds["o"], "%s composed" % what)
    assert np.array_equal(es.bits(kcc), es.bits(want_k)) and np.array_equal(es.bits(vcc), es.bits(want_v)), what
    assert (np.abs(o.astype(np.float64) - oc) <= 2 * res.bounds["o"]).all(), "%s native against composed" % what
    return o


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ex.LAYOUTS)
@pytest.mark.parametrize("length", EDGES)
def test_lengths_and_rows_around_the_block(length, layout, dtype):
    """len x T over {0, 1, 63, 64, 65, 130}^2 at B H = 3, D 16, Dv 24; (130, 130) fills its cache exactly."""
    for t in EDGES[1:] + [2]:
        tmax = length + t + (0 if (length, t) == (130, 130) else 3)
        b, h = (3, 1) if layout == "bthd" else (1, 3)
        case = es.make_case(eo.case_seed("edge%d.%d%s" % (length, t, layout)), layout, b, h, h, tmax, length, t, 16, 24, dtype)
        check_extend(case, dtype, what="len %d T %d %s" % (length, t, layout))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d,dv", [(5, 3), (16, 24), (72, 40), (128, 128)])
def test_head_dimensions(d, dv, dtype):
    """Every NT of the float32 kernel (1, 2, 8 by 5, 24, 72 and 128 columns; 4 by 40 x 40 below), odd widths on the element
    path; len 70, T 70: a block that straddles `len`, one wholly new, a second query block."""
    for layout in ex.LAYOUTS:
        case = es.make_case(eo.case_seed("dims%d.%d%s" % (d, dv, layout)), layout, 1, 2, 2, 150, 70, 70, d, dv, dtype)
        check_extend(case, dtype, what="D %d Dv %d %s" % (d, dv, layout))
    if (d, dv) == (72, 40):
        case = es.make_case(eo.case_seed("dims40"), "bthd", 1, 2, 2, 150, 70, 70, 40, 40, dtype)
        check_extend(case, dtype, what="D 40 Dv 40")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ex.LAYOUTS)
def test_element_aligned_bases(layout, dtype):
    """Every operand at an address that is only element-aligned: the element accesses, the same results."""
    case = es.make_case(eo.case_seed("unaligned" + layout), layout, 1, 2, 2, 150, 70, 70, 16, 24, dtype)
    a = check_extend(case, dtype, unaligned=True, what="unaligned %s" % layout)
    b = check_extend(case, dtype, what="aligned %s" % layout)
    assert np.array_equal(es.bits(a), es.bits(b))                    # the access width changes no bit


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("h,hkv", [(2, 2), (4, 2), (4, 1), (8, 1)])
def test_groups(h, hkv, dtype):
    """H / Hkv in {1, 2, 4} and 8 heads over one: B 2, len 65, T 66.  The caches hold Hkv heads; the result is that of the
    plain call on explicitly repeated k and v, within the bounds (in fact bit for bit: a group only changes the head index)."""
    for layout in ex.LAYOUTS:
        case = es.make_case(eo.case_seed("group%d.%d%s" % (h, hkv, layout)), layout, 2, h, hkv, 140, 65, 66, 16, 24, dtype)
        o = check_extend(case, dtype, what="H %d Hkv %d %s" % (h, hkv, layout))
        axis = eo.AXES[layout][1]
        assert case["k_cache"].shape[axis] == hkv
        rep = dict(case, **{n: np.repeat(case[n], h // hkv, axis=axis) for n in ("k_cache", "v_cache", "k_new", "v_new")})
        res = es.reference(rep, dtype)
        o_rep, _, _ = es.run_extend("native", rep, dtype)
        ao.assert_within(o_rep, res.values["o"], res.bounds["o"], "repeated heads")
        assert (np.abs(o.astype(np.float64) - o_rep) <= 2 * res.bounds["o"]).all()
        print("H %d Hkv %d %s: grouped == repeated bit for bit: %s" % (h, hkv, layout, np.array_equal(es.bits(o), es.bits(o_rep))))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("h,hkv", [(1, 1), (4, 2)])
def test_chunk_invariance_bit_for_bit(h, hkv, dtype):
    """150 rows from an empty cache as one call, cut (64, 64, 22) and cut (1, 63, 86); 37 cached rows followed by (27, 1, 100)
    against one call of 128: the o rows and both caches identical in bits()."""
    tn.set_default_float(dtype)
    case = es.make_case(eo.case_seed("invariance%d" % h), "bthd", 2, h, hkv, 160, 0, 150, 16, 24, dtype)
    whole = es.run_chunks("native", case, dtype, (150,))
    for cuts in ((64, 64, 22), (1, 63, 86)):
        for got, want in zip(es.run_chunks("native", case, dtype, cuts), whole):
            assert np.array_equal(es.bits(got), es.bits(want)), cuts
    later = es.make_case(eo.case_seed("invariance37.%d" % h), "bhtd", 1, h, hkv, 170, 37, 128, 40, 40, dtype)
    whole = es.run_chunks("native", later, dtype, (128,))
    for got, want in zip(es.run_chunks("native", later, dtype, (27, 1, 100)), whole):
        assert np.array_equal(es.bits(got), es.bits(want))
    ao.assert_within(whole[0], es.reference(later, dtype).values["o"], es.reference(later, dtype).bounds["o"], "len 37")


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_prefill_into_the_cache_agrees_with_tnn_attn_fwd(dtype):
    """len == 0 against tnn_attn_fwd(causal=1) on the same operands: within the sum of both bounds (twice the one bound);
    whether the bits agree is printed."""
    tn.set_default_float(dtype)
    case = es.make_case(eo.case_seed("fwd"), "bthd", 2, 3, 3, 140, 0, 130, 16, 24, dtype)
    res = es.reference(case, dtype)
    o, _, _ = es.run_extend("native", case, dtype)
    fwd, _ = da.attention(tn.asarray(case["q"]), tn.asarray(case["k_new"]), tn.asarray(case["v_new"]), True, None, "bthd", "native")
    fwd = np.asarray(fwd)
    ao.assert_within(fwd, res.values["o"], res.bounds["o"], "tnn_attn_fwd")
    assert (np.abs(o.astype(np.float64) - fwd) <= 2 * res.bounds["o"]).all()
    print("%s: tnn_extend_attn(len 0) == tnn_attn_fwd(causal) bit for bit: %s" % (np.dtype(dtype).name, np.array_equal(es.bits(o), es.bits(fwd))))


def test_the_library_refuses_what_the_planner_refuses():
    """The raw entry point, past the planner — only refusals its own validation makes before any launch: an overflowing cache,
    T < 1, H no multiple of Hkv, a head dimension beyond 128, k_new that is a cache."""
    lib = _lib.get()
    q, k, v, o = (tn.zeros(s, np.float32) for s in ((1, 2, 1, 4), (1, 8, 1, 4), (1, 8, 1, 4), (1, 2, 1, 4)))
    strides = da._i64arr((8, 4, 4) * 3 + (32, 4, 4) * 2 + (8, 4, 4))
    base = dict(k_new=q, B=1, H=1, Hkv=1, T=2, len=3, Tmax=8, D=4, Dv=4, dtype=0)
    for change, msg in ((dict(len=7), "len 7 \\+ T 2 new rows overflow a cache of 8 rows"), (dict(T=0), "T = 0 new rows"),
                        (dict(H=3, Hkv=2), "H 3 is no multiple of Hkv 2"), (dict(D=129), "head dimensions D = 129, Dv = 4 outside 1 .. 128"),
                        (dict(dtype=2), "dtype 2"), (dict(k_new=k), "alias a cache")):
        a = dict(base, **change)
        with pytest.raises(_lib.TnnError, match="tnn_extend_attn: .*" + msg):
            lib.extend_attn(q._ptr, a["k_new"]._ptr, q._ptr, k._ptr, v._ptr, o._ptr, a["B"], a["H"], a["Hkv"], a["T"], a["len"],
                            a["Tmax"], a["D"], a["Dv"], strides, 0.5, a["dtype"])
    assert not np.asarray(k).any() and not np.asarray(o).any()                          # nothing ran
    with pytest.raises(ValueError, match="overflow a cache of 8 rows"):
        da.attention_extend(q, k, v, 7, q, q)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,kv_heads,rope", [("mha", None, False), ("mha", 2, True), ("block", None, True), ("block", 2, False)])
def test_layers_on_the_native_route(monkeypatch, kind, kv_heads, rope, dtype):
    """tests/test_extend_host.py's prefill-plus-extension check with fused layers: ONE tnn_extend_attn call in the extension."""
    calls = []
    lib = _lib.get()
    real = lib.extend_attn
    monkeypatch.setattr(lib, "extend_attn", lambda *a: (calls.append(a[6:14]), real(*a))[1])
    es.check_layer(monkeypatch, kind, True, kv_heads, rope, dtype)
    assert calls == [(2, 4, kv_heads or 4, 7, 5, 12, 4, 4)]                            # B, H, Hkv, T, len, Tmax, D, Dv


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_model_on_the_native_route(golden, dtype):
    es.check_model_logits(golden, True, dtype)
    es.check_generate(golden, True, dtype)
