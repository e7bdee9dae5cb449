"""The host path under the six training attention entry points of device_array — attention, attention_bwd_q, attention_bwd_kv
and their grouped-query forms — on the backend of the session: what each of them hands to the library and gives back, pinned
as lists, identities, texts and bits (no tolerances).

    composed traces    the grouped composed route IS _gqa_expand(k), _gqa_expand(v), the plain composed route on the expanded
                       operands in layout "bthd" and (backward-kv) the two group sums, call for call and bit for bit
    messages           every refusal in full with the entry point's own prefix, their precedence, the returns of every need_*
                       combination, the empty results
    destinations       a lent array is written only when it is dense, of the dtype and of exactly the operand's shape
    native arguments   (product library only) the extents, strides, scale, causal flag, dtype code and addresses of the ONE call

Shapes: B 2, Tq 9, Tk 12, D 5, Dv 7 — Tq != Tk and D != Dv tell q from k and "o" from "q" strides apart; (H, Hkv) = (6, 2) is a
group of three, (4, 4) group one, (3, 1) multi-query; the plain form also runs layout "bhtd" under two leading dimensions."""

import numpy as np
import pytest

import dropout_support as dsu
import tinynn_autograd_amd as tn
from tinynn_autograd_amd import _lib, device_array as da

B, TQ, TK, D, DV = 2, 9, 12, 5, 7
HEADS = [(6, 2), (4, 4), (3, 1)]
FLOATS = [np.float32, np.float64]
# A form names the entry points and the operand shapes: a pair (H, Hkv) is the grouped form; the plain form is "bthd" (six
# heads), "bhtd" (two leading dimensions, 2 x 3) or "2d" ("bhtd" without leading dimensions).
PLAIN_LEAD = {"bhtd": (2, 3), "2d": ()}


def is_grouped(form):
    return isinstance(form, tuple)


def shapes(form):
    """name -> shape of q, k, v, o and the row statistics lse / delta."""
    if form in PLAIN_LEAD:
        lead = PLAIN_LEAD[form]
        return {"q": lead + (TQ, D), "k": lead + (TK, D), "v": lead + (TK, DV), "o": lead + (TQ, DV), "lse": lead + (TQ,)}
    h, hkv = form if is_grouped(form) else (6, 6)
    return {"q": (B, TQ, h, D), "k": (B, TK, hkv, D), "v": (B, TK, hkv, DV), "o": (B, TQ, h, DV), "lse": (B, h, TQ)}


def entry_points(form):
    """(forward, backward-q, backward-kv, the layout argument they take, the prefix of their messages)."""
    if is_grouped(form):
        return da.gqa_attention, da.gqa_attention_bwd_q, da.gqa_attention_bwd_kv, {}, "gqa_attention"
    return da.attention, da.attention_bwd_q, da.attention_bwd_kv, {"layout": "bthd" if form == "bthd" else "bhtd"}, "attention"


def operands(form, dtype, seed=3):
    """name -> dense device array in `dtype`: q, k, v and the gradient do of the output."""
    rs, sh = np.random.RandomState(seed), shapes(form)
    return {n: dsu.dev(rs.randn(*sh[s]) * amp, dtype) for n, s, amp in (("q", "q", 2.0), ("k", "k", 1.0), ("v", "v", 3.0),
                                                                      ("do", "o", 1.0))}


class Calls(object):
    """dropout_support.count_calls with `run`: (result, the calls it made)."""

    def __init__(self, monkeypatch):
        self.seen = dsu.count_calls(monkeypatch)

    def run(self, fn):
        del self.seen[:]
        res = fn()
        return res, list(self.seen)


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    return tuple(a.shape) == tuple(b.shape) and a.dtype == b.dtype and np.array_equal(dsu.bits(a), dsu.bits(b))


# ---------------------------------------------------------------------- composed call traces
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("heads", HEADS)
def test_grouped_composed_route_is_expand_expand_plain_and_two_sums(monkeypatch, heads, dtype, causal):
    h, hkv = heads
    group = h // hkv
    x = operands(heads, dtype)
    q, k, v, do = x["q"], x["k"], x["v"], x["do"]
    if causal:
        da._attn_mask(TQ, TK, np.dtype(dtype))                # uploaded once, before anything is recorded
    calls = Calls(monkeypatch)
    ke, t_k = calls.run(lambda: da._gqa_expand(k, group))
    ve, t_v = calls.run(lambda: da._gqa_expand(v, group))
    assert (t_k == [] and ke is k and ve is v) if group == 1 else (t_k and ke.shape == (B, TK, h, D))
    # forward
    (o1, lse1), t_plain = calls.run(lambda: da.attention(q, ke, ve, causal, None, "bthd", "composed"))
    (o, lse), t = calls.run(lambda: da.gqa_attention(q, k, v, causal, route="composed"))
    assert t == t_k + t_v + t_plain and t_plain
    assert same_bits(o, o1) and same_bits(lse, lse1) and o.shape == (B, TQ, h, DV) and lse.shape == (B, h, TQ)
    # backward-q, with and without dq
    for need_dq in (True, False):
        (dq1, delta1), t_plain = calls.run(lambda: da.attention_bwd_q(q, ke, ve, o, do, lse, causal, None, "bthd", "composed",
                                                                      need_dq))
        (dq, delta), t = calls.run(lambda: da.gqa_attention_bwd_q(q, k, v, o, do, lse, causal, route="composed",
                                                                  need_dq=need_dq))
        assert t == t_k + t_v + t_plain and t_plain
        assert same_bits(dq, dq1) and same_bits(delta, delta1) and (dq is None) == (not need_dq)
    # backward-kv: the two group sums follow, dk's first — also for a group of one
    fold = lambda g, w: g.reshape(B, TK, hkv, group, w).sum(axis=3)
    for need_dk, need_dv in ((True, True), (True, False), (False, True)):
        (dk1, dv1), t_plain = calls.run(lambda: da.attention_bwd_kv(q, ke, ve, do, lse, delta, causal, None, "bthd", "composed",
                                                                    need_dk, need_dv))
        dk1, t_dk = calls.run(lambda: None if dk1 is None else fold(dk1, D))
        dv1, t_dv = calls.run(lambda: None if dv1 is None else fold(dv1, DV))
        (dk, dv), t = calls.run(lambda: da.gqa_attention_bwd_kv(q, k, v, do, lse, delta, causal, route="composed",
                                                                need_dk=need_dk, need_dv=need_dv))
        assert t == t_k + t_v + t_plain + t_dk + t_dv and t_plain
        assert bool(t_dk) == need_dk and bool(t_dv) == need_dv
        assert same_bits(dk, dk1) and same_bits(dv, dv1)
        assert (dk is None or dk.shape == k.shape) and (dv is None or dv.shape == v.shape)


# ---------------------------------------------------------------------- messages, precedence, returns
STATS_Q = "%s_bwd_q: do / o %s and lse %s do not match the output %s and row statistics %s of this attention"
STATS_KV = "%s_bwd_kv: lse %s / delta %s do not match the row statistics %s of this attention"
FORMS = ["bhtd", "bthd", (6, 2), (4, 4), (3, 1)]


def raised(exc, fn):
    with pytest.raises(exc) as info:
        fn()
    return str(info.value)


@pytest.mark.parametrize("form", FORMS)
def test_messages_in_full_and_their_precedence(form):
    fwd, bwd_q, bwd_kv, lay, what = entry_points(form)
    sh = shapes(form)
    x = operands(form, np.float32)
    q, k, v, do = x["q"], x["k"], x["v"], x["do"]
    o, lse = fwd(q, k, v, True, **lay)
    _, delta = bwd_q(q, k, v, o, do, lse, True, need_dq=False, **lay)
    short = tn.zeros(sh["lse"][:-1] + (TQ - 1,))              # row statistics of another attention
    o_bad = tn.zeros(sh["o"][:-1] + (DV + 1,))
    do_bad = tn.zeros(sh["o"][:-1] + (DV + 1,))               # cannot be broadcast to the output
    k_bad = tn.zeros(sh["k"][:-1] + (D + 1,))                 # refused by the planner
    # 2. the statistics-shape texts
    assert raised(ValueError, lambda: bwd_q(q, k, v, o_bad, do, lse, **lay)) == \
        STATS_Q % (what, o_bad.shape, sh["lse"], sh["o"], sh["lse"])
    assert raised(ValueError, lambda: bwd_q(q, k, v, o, do, short, **lay)) == \
        STATS_Q % (what, sh["o"], short.shape, sh["o"], sh["lse"])
    assert raised(ValueError, lambda: bwd_kv(q, k, v, do, short, delta, **lay)) == \
        STATS_KV % (what, short.shape, sh["lse"], sh["lse"])
    assert raised(ValueError, lambda: bwd_kv(q, k, v, do, lse, short, **lay)) == \
        STATS_KV % (what, sh["lse"], short.shape, sh["lse"])
    # 1. before 2.: the planner speaks first, under the forward's name
    plan_text = "%s: q has head dimension %d, k has %d" % (what, D, D + 1)
    assert raised(ValueError, lambda: fwd(q, k_bad, v, **lay)) == plan_text
    assert raised(ValueError, lambda: bwd_q(q, k_bad, v, o_bad, do_bad, short, **lay)) == plan_text
    assert raised(ValueError, lambda: bwd_kv(q, k_bad, v, do_bad, short, short, need_dk=False, need_dv=False, **lay)) == plan_text
    # 2. before 3.: the statistics are checked before do is broadcast
    assert raised(ValueError, lambda: bwd_q(q, k, v, o, do_bad, short, **lay)).startswith(what + "_bwd_q: do / o ")
    assert raised(ValueError, lambda: bwd_kv(q, k, v, do_bad, short, delta, **lay)).startswith(what + "_bwd_kv: lse ")
    # 3. before 4.: do is broadcast before "nothing needed" returns
    cannot = "operands could not be broadcast together with shapes %s %s" % (do_bad.shape, sh["o"])
    assert raised(ValueError, lambda: bwd_q(q, k, v, o, do_bad, lse, need_dq=False, **lay)) == cannot
    assert raised(ValueError, lambda: bwd_kv(q, k, v, do_bad, lse, delta, need_dk=False, need_dv=False, **lay)) == cannot


@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("form", FORMS)
def test_returns_of_every_need_combination(form, dtype):
    fwd, bwd_q, bwd_kv, lay, _ = entry_points(form)
    sh = shapes(form)
    x = operands(form, dtype)
    q, k, v, do = x["q"], x["k"], x["v"], x["do"]
    o, lse = fwd(q, k, v, True, **lay)
    dq, delta = bwd_q(q, k, v, o, do, lse, True, **lay)
    none, delta_only = bwd_q(q, k, v, o, do, lse, True, need_dq=False, **lay)
    assert none is None and same_bits(delta_only, delta) and delta.shape == sh["lse"] and dq.shape == sh["q"]
    one = tn.asarray(np.ones((1,) * len(sh["o"])), dtype=dtype)       # a gradient that is broadcast to the output
    full = tn.asarray(np.ones(sh["o"]), dtype=dtype)
    for got, want in zip(bwd_q(q, k, v, o, one, lse, True, **lay), bwd_q(q, k, v, o, full, lse, True, **lay)):
        assert same_bits(got, want)
    assert bwd_kv(q, k, v, do, lse, delta, True, need_dk=False, need_dv=False, **lay) == (None, None)
    dk, dv = bwd_kv(q, k, v, do, lse, delta, True, **lay)
    assert dk.shape == sh["k"] and dv.shape == sh["v"] and dk.dtype == dv.dtype == dtype
    dk1, none = bwd_kv(q, k, v, do, lse, delta, True, need_dv=False, **lay)
    assert none is None and same_bits(dk1, dk)
    none, dv1 = bwd_kv(q, k, v, do, lse, delta, True, need_dk=False, **lay)
    assert none is None and same_bits(dv1, dv)


@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("zero", ["B", "Tq"])
@pytest.mark.parametrize("form", ["bthd", (6, 2), (3, 1)])
def test_empty_results_make_no_library_call(monkeypatch, form, zero, dtype):
    fwd, bwd_q, bwd_kv, lay, _ = entry_points(form)
    h, hkv = form if is_grouped(form) else (6, 6)
    b, tq = (0, TQ) if zero == "B" else (B, 0)
    sh = {"q": (b, tq, h, D), "k": (b, TK, hkv, D), "v": (b, TK, hkv, DV), "o": (b, tq, h, DV), "lse": (b, h, tq)}
    q, k, v, do = (tn.zeros(sh[n], dtype) for n in ("q", "k", "v", "o"))
    calls = Calls(monkeypatch)

    def check(a, shape):
        assert type(a) is da.DeviceArray and a.shape == shape and a.dtype == dtype and not np.asarray(a).any()

    (o, lse), t = calls.run(lambda: fwd(q, k, v, True, **lay))
    assert t == []
    check(o, sh["o"]), check(lse, sh["lse"])
    (dq, delta), t = calls.run(lambda: bwd_q(q, k, v, o, do, lse, True, **lay))
    assert t == []
    check(dq, sh["q"]), check(delta, sh["lse"])
    (dq, delta), t = calls.run(lambda: bwd_q(q, k, v, o, do, lse, True, need_dq=False, **lay))
    assert t == [] and dq is None
    check(delta, sh["lse"])                                   # backward-q has no "nothing needed" return: delta is still there
    # no query at all (Tq = 0) still leaves keys: dk and dv are zeros of k's and v's shape, one fill each and nothing else
    fills = ["fill"] if zero == "Tq" else []
    (dk, dv), t = calls.run(lambda: bwd_kv(q, k, v, do, lse, delta, True, **lay))
    assert t == fills * 2
    check(dk, sh["k"]), check(dv, sh["v"])
    (dk, dv), t = calls.run(lambda: bwd_kv(q, k, v, do, lse, delta, True, need_dk=False, **lay))
    assert t == fills and dk is None
    check(dv, sh["v"])
    assert bwd_kv(q, k, v, do, lse, delta, True, need_dk=False, need_dv=False, **lay) == (None, None)


# ---------------------------------------------------------------------- the destination rule
def lent(kind, shape, dtype):
    """A destination the caller lends, filled with sevens: (array, whether the launch may write it)."""
    other = np.float64 if dtype == np.float32 else np.float32
    size = int(np.prod(shape))
    if kind == "exact":
        return da.full(shape, 7.0, dtype), True
    if kind == "flat":                                          # the same number of elements, another shape
        return da.full((size,), 7.0, dtype), False
    if kind == "dtype":
        return da.full(shape, 7.0, other), False
    assert kind == "transposed"                                 # the lazy transpose of a 2-D array
    return da.full((size // shape[0], shape[0]) if len(shape) == 2 else (shape[-1], size // shape[-1]), 7.0, dtype).T, False


def untouched(a):
    return bool((np.asarray(a) == 7.0).all())


DEST_FORMS = ["2d"] + FORMS


def dest_case(form, dtype, route):
    """(the three entry points with their options bound, shapes, operands, o, lse, delta) — or a skip where the session's
    library has no native route."""
    fwd, bwd_q, bwd_kv, lay, _ = entry_points(form)
    sh, x = shapes(form), operands(form, dtype)
    q, k, v = x["q"], x["k"], x["v"]
    plan = da._gqa_plan(q, k, v, True, None, None) if is_grouped(form) else da._attn_plan(q, k, v, True, None, lay["layout"], None)
    if route == "native" and plan.route != "native":
        pytest.skip("the session's library has no native attention route (the CPU test twin)")
    lay = dict(lay, route=route, causal=True)
    o, lse = fwd(q, k, v, **lay)
    _, delta = bwd_q(q, k, v, o, x["do"], lse, need_dq=False, **lay)
    return bwd_q, bwd_kv, lay, sh, x, o, lse, delta


@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("kind", ["exact", "flat", "dtype", "transposed"])
@pytest.mark.parametrize("form", DEST_FORMS)
def test_native_route_writes_a_lent_destination_only_of_exactly_the_operands_shape(form, kind, dtype):
    bwd_q, bwd_kv, lay, sh, x, o, lse, delta = dest_case(form, dtype, "native")
    q, k, v, do = x["q"], x["k"], x["v"], x["do"]
    want_dq, _ = bwd_q(q, k, v, o, do, lse, **lay)
    want_dk, want_dv = bwd_kv(q, k, v, do, lse, delta, **lay)
    (dq_out, ok), (dk_out, _), (dv_out, _) = (lent(kind, sh[n], dtype) for n in "qkv")
    dq, _ = bwd_q(q, k, v, o, do, lse, dq_out=dq_out, **lay)
    dk, dv = bwd_kv(q, k, v, do, lse, delta, dk_out=dk_out, dv_out=dv_out, **lay)
    for got, out, want in ((dq, dq_out, want_dq), (dk, dk_out, want_dk), (dv, dv_out, want_dv)):
        assert same_bits(got, want)                             # repeated launches give identical bits
        assert (got is out) if ok else (got is not out and untouched(out))
    # a destination that is not needed is neither returned nor written
    (dq_out, _), (dk_out, _), (dv_out, _) = (lent("exact", sh[n], dtype) for n in "qkv")
    assert bwd_q(q, k, v, o, do, lse, need_dq=False, dq_out=dq_out, **lay)[0] is None and untouched(dq_out)
    dk, dv = bwd_kv(q, k, v, do, lse, delta, need_dk=False, dk_out=dk_out, dv_out=dv_out, **lay)
    assert dk is None and untouched(dk_out) and dv is dv_out
    dk, dv = bwd_kv(q, k, v, do, lse, delta, need_dv=False, dk_out=dk_out, dv_out=lent("exact", sh["v"], dtype)[0], **lay)
    assert dv is None and dk is dk_out


@pytest.mark.parametrize("form", DEST_FORMS)
def test_composed_route_ignores_lent_destinations(form):
    bwd_q, bwd_kv, lay, sh, x, o, lse, delta = dest_case(form, np.float32, "composed")
    q, k, v, do = x["q"], x["k"], x["v"], x["do"]
    (dq_out, _), (dk_out, _), (dv_out, _) = (lent("exact", sh[n], np.float32) for n in "qkv")
    dq, _ = bwd_q(q, k, v, o, do, lse, dq_out=dq_out, **lay)
    dk, dv = bwd_kv(q, k, v, do, lse, delta, dk_out=dk_out, dv_out=dv_out, **lay)
    for got, out, name in ((dq, dq_out, "q"), (dk, dk_out, "k"), (dv, dv_out, "v")):
        assert got is not out and untouched(out) and got.shape == sh[name]


# ---------------------------------------------------------------------- the native call's arguments (product library only)
# Written out by hand from B 2, Tq 9, Tk 12, D 5, Dv 7.  (batch, head, row) element strides of a dense operand with T rows of
# W elements: layout "bthd" with H heads (T H W, W, H W); layout "bhtd" (H = 1, the two leading dimensions 2 x 3 fold into the
# batch) (T W, T W, W).
NATIVE = {
    # plain, "bhtd" under (2, 3): six extents
    "bhtd": dict(extents=(6, 1, 9, 12, 5, 7), q=(45, 45, 5), k=(60, 60, 5), v=(84, 84, 7), o=(63, 63, 7)),
    # grouped, H 6 over Hkv 2: seven extents; k and v hold two heads
    (6, 2): dict(extents=(2, 6, 2, 9, 12, 5, 7), q=(270, 5, 30), k=(120, 5, 10), v=(168, 7, 14), o=(378, 7, 42)),
}
DTYPE_CODE = {np.float32: 0, np.float64: 1}                     # TNN_F32, TNN_F64


def record(monkeypatch, name):
    """Wrap the ONE entry point `name` of the loaded library: the list its argument tuples are appended to."""
    lib, rec = _lib.get(), []
    real = getattr(lib, name)

    def call(*args):
        rec.append(args)
        return real(*args)
    monkeypatch.setattr(lib, name, call)
    return rec


@pytest.mark.parametrize("causal, scale", [(False, None), (True, 0.375)])
@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("form", ["bhtd", (6, 2)])
def test_native_call_arguments(monkeypatch, form, dtype, causal, scale):
    if tn.backend_name() != "hip-gfx950":
        pytest.skip("the native route needs the product library")
    fwd, bwd_q, bwd_kv, lay, _ = entry_points(form)
    prefix = "gqa_" if is_grouped(form) else "attn_"
    want = NATIVE[form]
    n_ext = len(want["extents"])
    x = operands(form, dtype)
    q, k, v, do = x["q"], x["k"], x["v"], x["do"]
    lay = dict(lay, causal=causal, scale=scale)
    tail = (5.0 ** -0.5 if scale is None else 0.375, int(causal), DTYPE_CODE[dtype])

    def one_call(name, fn):
        with monkeypatch.context() as patch:
            rec = record(patch, prefix + name)
            res = fn()
        assert len(rec) == 1
        return res, rec[0]

    def check(args, pointers, stride_names):
        n = len(pointers)
        assert len(args) == n + n_ext + 4
        assert tuple(args[:n]) == tuple(pointers)
        assert tuple(args[n:n + n_ext]) == want["extents"]
        assert list(args[n + n_ext]) == [s for name in stride_names for s in want[name]]
        assert tuple(args[n + n_ext + 1:]) == tail

    ptr = lambda a: None if a is None else a._ptr
    (o, lse), args = one_call("fwd", lambda: fwd(q, k, v, **lay))
    check(args, [ptr(a) for a in (q, k, v, o, lse)], "qkvo")
    for need_dq in (True, False):
        (dq, delta), args = one_call("bwd_q", lambda: bwd_q(q, k, v, o, do, lse, need_dq=need_dq, **lay))
        assert (dq is None) == (not need_dq)
        check(args, [ptr(a) for a in (q, k, v, o, do, lse, dq, delta)], "qkvooq")
    for need_dk, need_dv in ((True, True), (True, False), (False, True)):
        (dk, dv), args = one_call("bwd_kv", lambda: bwd_kv(q, k, v, do, lse, delta, need_dk=need_dk, need_dv=need_dv, **lay))
        assert (dk is None) == (not need_dk) and (dv is None) == (not need_dv)
        check(args, [ptr(a) for a in (q, k, v, do, lse, delta, dk, dv)], "qkvokv")
    # a lent destination of exactly the operand's shape is the address the launch gets
    dq_out, dk_out, dv_out = (tn.zeros(a.shape, dtype) for a in (q, k, v))
    _, args = one_call("bwd_q", lambda: bwd_q(q, k, v, o, do, lse, dq_out=dq_out, **lay))
    assert args[6] == dq_out._ptr
    _, args = one_call("bwd_kv", lambda: bwd_kv(q, k, v, do, lse, delta, dk_out=dk_out, dv_out=dv_out, **lay))
    assert args[6:8] == (dk_out._ptr, dv_out._ptr)
