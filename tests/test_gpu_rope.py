"""tnn_rope_apply on an MI355X (csrc/tnn_rope.hip) against the long-double oracle's derived bound (tests/rope_oracle.py) and
against the composed route under twice that; bit-identity across the access paths, in place, forced workgroup counts and
repeated calls; device positions; and the rotary language model end to end.

Cases (B, T, Ha, Hb, D, R), float32 and float64, both pairings:
    (1,1,1,0,2,2)      one pair, single tensor
    (2,5,3,1,3,2)      odd D, partial rotary, element path
    (1,5,2,2,8,8)      R / 2 is exactly one float32 vector; float64 has two
    (3,1,4,2,16,8)     partial rotary with an aligned tail
    (1,65,4,1,24,12)   R / 2 = 6: wide for float64, element for float32
    (2,3,8,1,64,64), (1,2,2,2,128,128), (1,2,1,1,130,128)    full-size head dimensions
"""

import ctypes

import numpy as np
import pytest

import gqa_oracle as go
import rope_oracle as ro
import rope_support as rsup
import tinynn_autograd_amd as tn
from tinynn_autograd_amd import _lib, device_array as da, generation as gen, rope as rp

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
bits = rsup.bits


@pytest.fixture(scope="module")
def golden():
    return rsup.load_golden()


def same(a, b):
    return all((x is None and y is None) or np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


# the access path of the aligned call, (half, interleaved) per dtype: what the header's rule gives for dense operands
WIDE = {
    "one_pair": {4: (False, False), 8: (False, True)},
    "odd_d_partial": {4: (False, False), 8: (False, False)},
    "one_f32_vector": {4: (True, True), 8: (True, True)},
    "aligned_tail": {4: (True, True), 8: (True, True)},
    "half_six": {4: (False, True), 8: (True, True)},
    "d64": {4: (True, True), 8: (True, True)},
    "d128": {4: (True, True), 8: (True, True)},
    "d130": {4: (False, False), 8: (True, True)},
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pairing", ro.PAIRINGS)
@pytest.mark.parametrize("name", list(ro.CASES))
def test_cases(golden, name, pairing, dtype):
    B, T, Ha, Hb, D, R = ro.CASES[name]
    rot = rsup.rotary(R, pairing)
    item = np.dtype(dtype).itemsize
    xa0, xb0 = ro.case_input(name, dtype)
    plan = rp.plan_rope(xa0.shape, None if xb0 is None else xb0.shape, R, ro.P, pairing=pairing, itemsize=item)
    assert plan.wide is WIDE[name][item][ro.PAIRINGS.index(pairing)]
    for layout in ro.LAYOUTS:
        xa, xb = ro.case_input(name, dtype, layout)
        for inverse in (False, True):
            for offset in (0, 7, ro.P - T):
                what = "%s %s %s %s inverse %d offset %d" % (name, pairing, np.dtype(dtype).name, layout, inverse, offset)
                args = (xa, xb, rot, dtype, offset, None, layout, inverse)
                got = rsup.run("native", *args)
                refs = rsup.references(xa, xb, rot, dtype, offset, None, layout, inverse)
                for y, r, which in zip(got, refs, "ab"):
                    if r is not None:
                        ro.assert_within(y, r, what + " " + which)
                assert same(got, rsup.run("native", *args)), what + ": a repeated call"
                assert same(got, rsup.run("native", *args, unaligned=True)), what + ": element path at a moved base"
                assert same(got, rsup.run("native", *args, inplace=True)), what + ": in place"
                assert same(got, rsup.run("native", *args, inplace=True, unaligned=True)), what + ": in place, element path"
                for blocks in (1, 3):
                    assert same(got, rsup.run("native", *args, blocks=blocks)), what + ": blocks %d" % blocks
                if offset == 7:
                    comp = rsup.run("composed", *args)
                    for y, cy, r in zip(got, comp, refs):
                        if r is not None:
                            assert (np.abs(y.astype(np.longdouble) - cy.astype(np.longdouble)) <= 2 * r.bounds).all(), what
    if dtype == np.float32:                                                 # the fixture: the oracle's values, rounded to float64
        ya, _ = rsup.run("native", xa0, xb0, rot, dtype, ro.GOLDEN_OFFSET)
        fwd, _ = rsup.references(xa0, xb0, rot, dtype, ro.GOLDEN_OFFSET)
        assert (np.abs(ya - golden["%s.%s.a" % (pairing, name)]) <= fwd.bounds * (1 + 2.0 ** -20)).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pairing", ro.PAIRINGS)
def test_a_row_of_a_long_call_is_the_single_row_call(pairing, dtype):
    """Row p of the T = 65 call is bit-equal to the T = 1 call at offset p (and rows walk the table in order)."""
    B, T, Ha, Hb, D, R = ro.CASES["half_six"]
    rot = rsup.rotary(R, pairing)
    xa, xb = ro.case_input("half_six", dtype)
    for offset in (0, ro.P - T):
        ya, yb = rsup.run("native", xa, xb, rot, dtype, offset)
        for p in (0, 1, 33, 64):
            oa, ob = rsup.run("native", xa[:, p:p + 1], xb[:, p:p + 1], rot, dtype, offset + p)
            assert same((ya[:, p:p + 1], yb[:, p:p + 1]), (oa, ob)), "row %d at offset %d" % (p, offset)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pairing", ro.PAIRINGS)
@pytest.mark.parametrize("name", ["aligned_tail", "odd_d_partial"])
def test_device_positions(name, pairing, dtype):
    """positions [0, P - 1, 5]: every sequence bit-equal to the offset call at its position; [-1, P, 2]: exact zeros for the
    first two (the tail included, in place too) and the third right — with tables that sit between NaN-filled neighbours, so
    a read outside [0, P) would show."""
    B, _, Ha, Hb, D, R = ro.CASES[name]
    xa, xb = (a[:3, :1] if a.shape[0] >= 3 else np.concatenate([a, a[:1]], axis=0)[:, :1] for a in ro.case_input(name, dtype))
    assert xa.shape[:2] == (3, 1)
    rot = rsup.rotary(R, pairing)
    positions = [0, ro.P - 1, 5]
    for unaligned in (False, True):
        ya, yb = rsup.run("native", xa, xb, rot, dtype, positions=positions, unaligned=unaligned)
        for b, p in enumerate(positions):
            one = rsup.run("native", xa[b:b + 1], xb[b:b + 1], rot, dtype, offset=p)
            assert same((ya[b:b + 1], yb[b:b + 1]), one), "sequence %d at position %d" % (b, p)
    # a small Rotary whose device tables are views into a NaN-filled buffer
    small = rp.Rotary(6, R, ro.BASE, pairing)
    half, dt = R // 2, np.dtype(dtype)
    n, pad = 6 * half, 8
    buf = tn.asarray(np.full((3 * pad + 2 * n + 8,), np.nan, dtype=dtype), dtype=dtype)
    cos_h, sin_h = small.host_tables(R, dtype)
    first = pad
    second = (2 * pad + n + 3) // 4 * 4                                    # 16-byte aligned for either dtype
    views = []
    for at, host in ((first, cos_h), (second, sin_h)):
        view = buf[at:at + n].reshape(6, half)
        view[...] = tn.asarray(host, dtype=dtype)
        views.append(view)
    small._device[(R, dt)] = tuple(views)
    edge = rsup.run("native", xa, xb, small, dtype, positions=[0, 5, 2])
    refs = rsup.references(xa, xb, small, dtype, positions=[0, 5, 2])
    for y, r in zip(edge, refs):
        ro.assert_within(y, r, "edge rows of tables between NaNs")
    for inplace in (False, True):
        ya, yb = rsup.run("native", xa, xb, small, dtype, positions=[-1, 6, 2], inplace=inplace)
        assert not bits(ya[:2]).any() and not bits(yb[:2]).any(), "an out-of-range position gives exact zeros"
        refs = rsup.references(xa, xb, small, dtype, positions=[-1, 6, 2])
        ro.assert_within(ya, refs[0], "bad positions a")
        ro.assert_within(yb, refs[1], "bad positions b")
        assert same((ya[2:], yb[2:]), [y[2:] for y in edge])
    assert np.isnan(np.asarray(buf)).sum() == buf.size - 2 * n              # and nothing was written around them


def test_refusals_of_the_entry_point():
    """What the host can see is refused before any launch: overlap that is not in-place, device positions with T > 1, offsets
    beyond the table, the blocks range, an odd rotary width."""
    lib = _lib.get()
    rot = rsup.rotary(4, "half", 16)
    cos_t, sin_t = da._rope_tables(rot, 4, np.dtype(np.float32))
    x, y = tn.zeros((64,)), tn.zeros((64,))
    i64 = lambda *v: (ctypes.c_int64 * len(v))(*v)
    dense = (16, 8, 4) * 4

    def call(xa=x._ptr, ya=y._ptr, xb=None, yb=None, positions=None, geometry=(2, 2, 2, 0, 4, 4, 16), strides=dense, offset=0,
             inverse=0, pairing=0, blocks=0, dtype=_lib.F32):
        lib.rope_apply(xa, ya, xb, yb, cos_t._ptr, sin_t._ptr, positions, i64(*geometry), i64(*strides), offset, inverse, pairing,
                       blocks, dtype)

    call()
    call(ya=x._ptr)                                                        # in place: equal views
    for kw, match in ((dict(ya=x._ptr + 16), "overlaps xa"), (dict(ya=x._ptr, strides=(16, 8, 4, 16, 4, 8) * 2), "overlaps xa"),
                      (dict(xb=x._ptr, yb=y._ptr + 64, geometry=(2, 2, 2, 1, 4, 4, 16), strides=(16, 8, 4) * 2 + (8, 4, 4) * 2),
                       "two tensors overlap"), (dict(ya=cos_t._ptr), "overlaps the tables"),
                      (dict(positions=y._ptr), "device positions need T == 1"), (dict(offset=15), "lie outside the table"),
                      (dict(offset=-1), "lie outside the table"), (dict(blocks=rp.MAX_BLOCKS + 1), "blocks"),
                      (dict(geometry=(2, 2, 2, 0, 4, 3, 16)), "rotary width"), (dict(geometry=(2, 2, 2, 0, 4, 6, 16)), "rotary width"),
                      (dict(pairing=2), "pairing"), (dict(dtype=_lib.I64), "float32 and float64"), (dict(xb=x._ptr), "come together")):
        with pytest.raises(_lib.TnnError, match=match):
            call(**kw)
    call(geometry=(0, 2, 2, 0, 4, 4, 16), xa=None, ya=None)                # B == 0: nothing is read or written
    call(geometry=(2, 0, 2, 0, 4, 4, 16), xa=None, ya=None)
    tn.synchronize()


@pytest.mark.parametrize("dtype", DTYPES)
def test_gradients_through_rope_and_attention(dtype, monkeypatch):
    """tests/test_rope_host.py states the bound: the summed bounds of the parts.  One rope launch forward, two backward."""
    lib = _lib.get()
    calls, real = [], lib.rope_apply
    monkeypatch.setattr(lib, "rope_apply", lambda *a: calls.append(a[10]) or real(*a))
    rs = np.random.RandomState(ro.case_seed("rope+attention"))
    q, k, v, do_ = go.make_inputs(rs, 2, 4, 2, 9, 9, 8, 8, dtype, q_amp=2.0)
    rot = rsup.rotary(8, "half", 16)
    da._rope_tables(rot, 8, np.dtype(dtype))
    dq, dk, qr, kr = rsup.attention_grads("native", q, k, v, do_, rot, dtype)
    assert calls == [0, 1, 1]
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


def test_generation_with_a_rotary(golden, monkeypatch):
    """rope_oracle's two-block model (4 query heads over 2 key / value heads, no position table, one shared Rotary), greedy:
    cached against uncached, ragged against uniform, eager against captured — all pick the float64 oracle's tokens, whose top-2
    margin exceeds 2 x LM_MARGIN logit bounds at every step.  A decoding step adds ONE rope launch per block."""
    c = ro.LM
    seed, scale, bound = int(golden["lm.seed"]), float(golden["lm.head_scale"]), float(golden["lm.logit_bound"])
    params, prompt = ro.lm_params(seed, scale), ro.lm_prompt(seed)
    ids, steps = ro.lm_generate(params, prompt, c["new"])
    srt = np.sort(steps, axis=-1)
    assert float((srt[..., -1] - srt[..., -2]).min()) > 2 * ro.LM_MARGIN * bound and np.array_equal(ids, golden["lm.ids"])
    tn.set_default_float(np.float32)
    net = rsup.lm_net(params, np.float32)
    for n in (0, c["new"] - 1):
        got = rsup.lm_last_logits(net, ids[:, :c["prompt"] + n])
        assert np.abs(got - steps[n]).max() <= ro.LM_MARGIN * bound, "step %d: %.3e" % (n, np.abs(got - steps[n]).max())
    lib = _lib.get()
    calls, real = [], lib.rope_apply
    monkeypatch.setattr(lib, "rope_apply", lambda *a: calls.append(1) or real(*a))
    cached = gen.generate(net, prompt, c["new"], temperature=0.0, cache=True)
    assert len(calls) == c["blocks"] * c["new"]                          # the prefill and new - 1 steps, one launch per block
    full = gen.generate(net, prompt, c["new"], temperature=0.0, cache=False)
    assert np.array_equal(cached, full) and np.array_equal(cached, ids)
    lens = np.full((c["B"],), c["prompt"], dtype=np.int64)
    eager = gen.generate(net, prompt, c["new"], temperature=0.0, prompt_lens=lens)
    captured = gen.generate(net, prompt, c["new"], temperature=0.0, prompt_lens=lens, capture=True)
    assert np.array_equal(np.asarray(eager), ids) and np.array_equal(np.asarray(captured), ids)
    # a ragged batch: every sequence continues as it does alone
    short = np.array([c["prompt"], c["prompt"] - 1], dtype=np.int64)
    ragged = np.asarray(gen.generate(net, prompt, 4, temperature=0.0, prompt_lens=short, capture=True))
    alone = gen.generate(net, prompt[1:, :c["prompt"] - 1], 4, temperature=0.0)
    assert np.array_equal(ragged[1, :c["prompt"] + 3], alone[0]) and np.array_equal(ragged[0], ids[0, :c["prompt"] + 4])
