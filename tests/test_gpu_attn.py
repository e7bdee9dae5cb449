"""csrc/tnn_attn.hip on the MI355X against the float64 oracle (tests/attn_oracle.py) under its DERIVED bounds, and against
the composed route (existing kernels only) under the sum of both routes' bounds.  Shapes are the smallest at which a kernel
can still go wrong: the wave-row and block edges of the planner's constants, head dimensions around the MFMA depth, the
16-element padding and the 128 limit, both layouts, element-aligned base pointers, every NULL-gradient variant."""

import os

import numpy as np
import pytest

import attn_oracle as ao
import tinynn_autograd_amd as tn
from tinynn_autograd_amd import _lib, attention as at
from tinynn_autograd_amd import device_array as da
from tinynn_autograd_amd.core import ops
from tinynn_autograd_amd.core.layers import MultiHeadAttention
from tinynn_autograd_amd.core.losses import SquaredErrorLoss
from tinynn_autograd_amd.core.model import Model
from tinynn_autograd_amd.core.nn import Net
from tinynn_autograd_amd.core.optimizer import Adam
from tinynn_autograd_amd.core.tensor import Tensor

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_cases.npz")
W, BQ, BK = at.WAVE_ROWS, at.BLOCK_Q, at.BLOCK_K
T_EDGES = [1, W - 1, W, W + 1, BK - 1, BK, BK + 1, 2 * BQ + 1]            # {1, 15, 16, 17, 63, 64, 65, 129}
D_EDGES = [1, at.MFMA_K - 1, at.MFMA_K, at.MFMA_K + 1, 16, 17, 64, 65, at.MAX_HEAD_DIM]


@pytest.fixture(autouse=True)
def _switches():
    yield
    da.ATTN_ROUTE = None


def dev(a, dtype, unaligned=False):
    """The array on the device in `dtype`; unaligned: at an address that is only element-aligned."""
    a = np.ascontiguousarray(a, dtype=dtype)
    if not unaligned:
        return tn.asarray(a, dtype=dtype)
    buf = tn.empty((a.size + 1,), dtype)
    view = buf[1:].reshape(a.shape)
    view[...] = tn.asarray(a, dtype=dtype)
    return view


def run(route, q, k, v, do, causal, scale, layout, dtype, unaligned=False, need=(True, True, True)):
    """The three raw calls of one route -> {name: numpy array or None}."""
    qd, kd, vd, dod = (dev(a, dtype, unaligned) for a in (q, k, v, do))
    opts = dict(causal=causal, scale=scale, layout=layout, route=route)
    o, lse = da.attention(qd, kd, vd, **opts)
    dq, delta = da.attention_bwd_q(qd, kd, vd, o, dod, lse, need_dq=need[0], **opts)
    dk, dv = da.attention_bwd_kv(qd, kd, vd, dod, lse, delta, need_dk=need[1], need_dv=need[2], **opts)
    out = dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv)
    return {n: None if a is None else np.asarray(a) for n, a in out.items()}


def check_both_routes(q, k, v, do, causal, scale, layout, dtype, what, unaligned=False, need=(True, True, True), res=None):
    res = res or ao.reference(q, k, v, do, causal, scale, layout, dtype)
    native = run("native", q, k, v, do, causal, scale, layout, dtype, unaligned, need)
    for name, wanted in zip(("dq", "dk", "dv"), need):
        assert (native[name] is not None) == wanted, "%s %s" % (what, name)
    ao.check(native, res, what + " native")
    composed = run("composed", q, k, v, do, causal, scale, layout, dtype, False, need)
    for name in ao.FIELDS:
        if native[name] is None:
            continue
        diff = np.abs(native[name].astype(np.float64) - composed[name].astype(np.float64))
        assert (diff <= 2 * res.bounds[name]).all(), "%s %s: the routes differ by more than both bounds" % (what, name)
    return native


def test_backend_and_entry_points():
    lib = _lib.get()
    assert tn.backend_name() == "hip-gfx950"
    assert lib.has_attn
    assert at.plan_attention((1, 4, 8), (1, 4, 8), (1, 4, 8), native=lib.has_attn).route == "native"
    o, _ = da.attention(tn.ones((1, 4, 8)), tn.ones((1, 4, 8)), tn.ones((1, 4, 8)))
    np.testing.assert_array_equal(np.asarray(o), np.ones((1, 4, 8), dtype=np.float32))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_fixture_cases(dtype):
    with np.load(GOLDEN) as data:
        golden = dict(data)
    layouts = set()
    for name in ao.ATTN_CASES:
        q, k, v, do, causal, scale, layout = ao.case_input(name)
        layouts.add(layout)
        res = ao.reference(q, k, v, do, causal, scale, layout, dtype)
        for field in ao.FIELDS:
            res.values[field] = golden["%s.%s" % (name, field)]
        check_both_routes(q, k, v, do, causal, scale, layout, dtype, "%s %s" % (name, np.dtype(dtype).name), res=res)
    assert layouts == {"bhtd", "bthd"}


def fuzz(dtype, count, seed):
    rs = np.random.RandomState(seed)
    needs = [(True, True, True), (False, True, True), (True, False, True), (True, True, False)]
    seen = set()
    for i in range(count):
        tq, tk = (int(rs.choice(T_EDGES)) for _ in range(2))
        d, dv = (int(rs.choice(D_EDGES)) for _ in range(2))
        bh = int(rs.choice([1, 2, 3]))
        b, h = (bh, 1) if i % 2 else (1, bh)
        layout = ("bhtd", "bthd")[(i // 2) % 2]
        causal = bool((i // 4) % 2)
        need = needs[i % 4] if i % 5 == 0 else needs[0]
        q_amp = (1.0, 4.0)[(i // 8) % 2]
        scale = None if i % 3 else 0.5 / np.sqrt(d)          # (an explicit scale that keeps the median gate's condition)
        q, k, v, do = ao.make_inputs(rs, layout, b, h, tq, tk, d, dv, dtype, q_amp)
        seen.add((layout, causal, need))
        check_both_routes(q, k, v, do, causal, scale, layout, dtype, "fuzz %d %s B%d H%d Tq%d Tk%d D%d Dv%d causal %d" % (
            i, layout, b, h, tq, tk, d, dv, causal), unaligned=bool(i & 1) ^ bool((i // 16) & 1), need=need)
    assert {n for _, _, n in seen} == set(needs)
    assert {(l, c) for l, c, _ in seen} == {(l, c) for l in ("bhtd", "bthd") for c in (False, True)}


def test_fuzz_raw_calls_float32():
    fuzz(np.float32, 80, 20261)


def test_fuzz_raw_calls_float64():
    fuzz(np.float64, 40, 20262)


@pytest.mark.parametrize("causal", [False, True])
def test_online_softmax_rescale(causal):
    """Tk = 3 key blocks.  Ten rows have one score larger by about 30 in the LAST block (every earlier block is rescaled),
    ten others one in the FIRST block (later blocks contribute almost nothing), one row has all scores equal.  The first
    20 head dimensions are random; each shaped row owns one of the next 20, where only it and its key are non-zero, so a
    planted score touches no other row.  (Causal: the shaped rows are the last ones, whose last-block key is their own.)"""
    rs = np.random.RandomState(77)
    tk, dr, dv = 3 * BK, 20, 8
    tq = tk if causal else 40
    q, k, v, do = ao.make_inputs(rs, "bhtd", 1, 2, tq, tk, dr + 20, dv, np.float32, q_amp=1.0)
    q[..., dr:] = 0.0
    k[..., dr:] = 0.0
    scale = 1.0 / np.sqrt(dr + 20)
    shaped = []
    for n in range(20):
        i = tq - 1 - n
        j = tk - 1 - n if n < 10 else n - 10             # last block (causal: j = i, kept) / first block
        q[0, :, i, dr + n] = 4.0
        k[0, :, j, dr + n] = 30.0 / (4.0 * scale)
        shaped.append(i)
    q[0, :, tq - 21] = 0.0                               # all scores of this row are equal
    res = ao.reference(q, k, v, do, causal, scale, "bhtd", np.float32)
    s64 = scale * np.einsum("hid,hjd->hij", q[0].astype(np.float64), k[0].astype(np.float64))
    s64 = np.where(ao.keep_mask(tq, tk, causal)[None], s64, -np.inf)
    top = np.sort(s64[:, shaped], axis=-1)
    assert (top[..., -1] - top[..., -2] > 20).all()      # the planted score dominates its row
    assert (np.argmax(s64[:, shaped[:10]], axis=-1) >= 2 * BK).all() and (np.argmax(s64[:, shaped[10:]], axis=-1) < BK).all()
    check_both_routes(q, k, v, do, causal, scale, "bhtd", np.float32, "rescale causal %d" % causal, res=res)


@pytest.mark.parametrize("tq, tk", [(2 * BQ + 1, 2 * BK + 1), (2 * BQ + 1, BK + 5), (BQ + 5, 2 * BK + 1)])
def test_causal_geometry(tq, tk):
    """Changing k, v at keys j > i leaves row i of o and of dq bit-identical; dk, dv at a key no query sees are exactly 0."""
    rs = np.random.RandomState(tq * 1000 + tk)
    q, k, v, do = ao.make_inputs(rs, "bthd", 1, 2, tq, tk, 8, 8, np.float32, q_amp=2.0)
    first = check_both_routes(q, k, v, do, True, None, "bthd", np.float32, "causal %d x %d" % (tq, tk))
    i = min(tq, tk) // 2
    k2, v2 = k.copy(), v.copy()
    k2[:, i + 1:] = rs.randn(*k2[:, i + 1:].shape) * 3
    v2[:, i + 1:] = rs.randn(*v2[:, i + 1:].shape) * 5
    second = run("native", q, k2, v2, do, True, None, "bthd", np.float32)
    assert np.array_equal(first["o"][:, :i + 1], second["o"][:, :i + 1])
    assert np.array_equal(first["dq"][:, :i + 1], second["dq"][:, :i + 1])
    assert not np.array_equal(first["o"][:, i + 1:], second["o"][:, i + 1:])
    if tk > tq:
        assert not first["dk"][:, tq:].any() and not first["dv"][:, tq:].any()
        assert first["dk"][:, :tq].any() and first["dv"][:, :tq].any()


def test_bit_identical_run_to_run():
    rs = np.random.RandomState(3)
    q, k, v, do = ao.make_inputs(rs, "bthd", 2, 2, 2 * BQ + 1, 2 * BK + 3, 17, 20, np.float32)
    for causal in (False, True):
        a = run("native", q, k, v, do, causal, None, "bthd", np.float32)
        b = run("native", q, k, v, do, causal, None, "bthd", np.float32)
        for name in ao.FIELDS:
            assert np.array_equal(a[name], b[name]), name


def leaf(a):
    t = Tensor(a, requires_grad=True)
    t.zero_grad()
    return t


def test_autograd_through_ops_attention(monkeypatch):
    lib = _lib.get()
    calls = {"q": 0, "kv": 0}
    real_q, real_kv = lib.attn_bwd_q, lib.attn_bwd_kv
    monkeypatch.setattr(lib, "attn_bwd_q", lambda *a: (calls.__setitem__("q", calls["q"] + 1), real_q(*a))[1])
    monkeypatch.setattr(lib, "attn_bwd_kv", lambda *a: (calls.__setitem__("kv", calls["kv"] + 1), real_kv(*a))[1])
    rs = np.random.RandomState(5)
    q, k, v, do = ao.make_inputs(rs, "bhtd", 2, 2, 33, 40, 16, 12, np.float32)
    res = ao.reference(q, k, v, do, True, None, "bhtd", np.float32)
    qt, kt, vt = leaf(q), leaf(k), leaf(v)
    out = ops.attention(qt, kt, vt, causal=True)
    out.backward(do)
    assert calls == {"q": 1, "kv": 1}                      # dq from one launch, dk + dv from one launch
    ao.check(dict(o=out.values, dq=qt.grad, dk=kt.grad, dv=vt.grad), res, "ops.attention")
    kt2, vt2 = leaf(k), leaf(v)
    ops.attention(Tensor(q), kt2, vt2, causal=True).backward(do)       # q without a gradient: delta only
    assert calls == {"q": 2, "kv": 2}
    ao.check(dict(dk=kt2.grad, dv=vt2.grad), res, "ops.attention, q frozen")
    with pytest.raises(TypeError, match="out of scope"):
        ops.attention(qt, kt, vt, mask=np.ones((33, 40)))


def arena_leaves(q, k, v):
    """q, k, v as leaves whose gradients have pinned views of ONE flat arena as their home (what a Model's optimizer
    gives its parameters): (tensors, arena)."""
    arena = tn.zeros((q.size + k.size + v.size,))
    leaves, off = [], 0
    for a in (q, k, v):
        t = Tensor(a, requires_grad=True)
        t._grad_home = arena[off:off + a.size].reshape(a.shape)
        t.zero_grad()
        leaves.append(t)
        off += a.size
    return leaves, arena


@pytest.mark.parametrize("layout", ["bthd", "bhtd"])
def test_gradients_land_in_lent_arena_views(layout, monkeypatch):
    """q, k, v with pinned arena views as gradient homes: the two backward launches write dq, dk, dv straight into the
    views (the pointers they are handed ARE the views'), `grad is _grad_home`, the values lie inside the oracle's bounds;
    the second backward finds the homes taken, writes fresh arrays and accumulates.  A home of the right size but another
    shape is not written in place (the kernels would address it with the operand's strides) and still ends up correct."""
    lib = _lib.get()
    seen = []
    real_q, real_kv = lib.attn_bwd_q, lib.attn_bwd_kv
    monkeypatch.setattr(lib, "attn_bwd_q", lambda *a: (seen.append(("q", a[6])), real_q(*a))[1])
    monkeypatch.setattr(lib, "attn_bwd_kv", lambda *a: (seen.append(("kv", a[6], a[7])), real_kv(*a))[1])
    rs = np.random.RandomState(41)
    q, k, v, do = ao.make_inputs(rs, layout, 2, 3, BQ + 3, BK + 9, 20, 12, np.float32)
    res = ao.reference(q, k, v, do, True, None, layout, np.float32)
    (qt, kt, vt), arena = arena_leaves(q, k, v)
    out = ops.attention(qt, kt, vt, causal=True, layout=layout)
    out.backward(do)
    assert seen == [("q", qt._grad_home._ptr), ("kv", kt._grad_home._ptr, vt._grad_home._ptr)]
    flat, off = np.asarray(arena), 0
    for t, name in ((qt, "dq"), (kt, "dk"), (vt, "dv")):
        assert t.grad is t._grad_home
        ao.assert_within(t.grad, res.values[name], res.bounds[name], "%s %s" % (layout, name))
        np.testing.assert_array_equal(flat[off:off + t.grad.size].reshape(t.shape), np.asarray(t.grad))
        off += t.grad.size
    out.backward(do)                                        # the homes are taken: fresh arrays, accumulated on top
    homes = {qt._grad_home._ptr, kt._grad_home._ptr, vt._grad_home._ptr}
    assert len(seen) == 4 and not (set(seen[2][1:]) | set(seen[3][1:])) & homes
    for t, name in ((qt, "dq"), (kt, "dk"), (vt, "dv")):
        assert t.grad is t._grad_home
        ao.assert_within(t.grad, 2 * res.values[name], 2 * res.bounds[name] + ao.U32 * np.abs(2 * res.values[name]),
                         "%s %s twice" % (layout, name))
    # homes of equal size and another shape (flat): not lent to the launch, filled by the scheduler's copy
    del seen[:]
    (qt, kt, vt), arena = arena_leaves(q, k, v)
    for t in (qt, kt, vt):
        t._grad_home = t._grad_home.reshape(t._grad_home.size)
    dq, _ = da.attention_bwd_q(qt.values, kt.values, vt.values, out.values, dev(do, np.float32),
                               da.attention(qt.values, kt.values, vt.values, causal=True, layout=layout)[1], causal=True,
                               layout=layout, dq_out=qt._grad_home)
    assert dq is not qt._grad_home and dq.shape == q.shape and seen[0][1] != qt._grad_home._ptr
    ao.assert_within(dq, res.values["dq"], res.bounds["dq"], "%s dq beside a flat home" % layout)


def mha_step(fused, x, y, seed=13):
    np.random.seed(seed)
    layer = MultiHeadAttention(2, num_in=x.shape[-1], causal=True, fused=fused)
    model = Model(net=Net([layer]), loss=SquaredErrorLoss(), optimizer=Adam(lr=1e-2))
    initial = [np.asarray(p.values, dtype=np.float64) for p in model.net.parameter_tensors()]
    model.zero_grad()
    loss = SquaredErrorLoss().loss(model.forward(Tensor(x)), Tensor(y))
    loss.backward()
    grads = [np.asarray(p.grad, dtype=np.float64) for p in model.net.parameter_tensors()]
    model.step()
    after = float(SquaredErrorLoss().loss(model.forward(Tensor(x)), Tensor(y)).values)
    return initial, float(loss.values), grads, after


def test_layer_step_native_against_composed_and_float64():
    """One Adam step of a causal two-head layer, native and fused=False, against the float64 replica.  Losses: 1e-5
    relative, the tolerance smoke() uses and the host test of the same step applies.  Gradients: the same 1e-5, of the
    sum of |terms| behind every element (attn_oracle.MHA64.grad_scales) — the parameter gradients are sums over the B T rows
    of products of the attention's gradients, whose own errors the raw-call tests hold to the derived bounds; 1e-5 is
    about 170 u of float32 for sums of 2 (2 BQ + 1) = 258 terms, i.e. below the (n + 2) u of a length-n dot product alone."""
    rs = np.random.RandomState(8)
    x = rs.randn(2, 2 * BQ + 1, 16).astype(np.float32)
    y = rs.randn(2, 2 * BQ + 1, 16).astype(np.float32)
    initial, loss_n, grads_n, after_n = mha_step(True, x, y)
    _, loss_c, grads_c, after_c = mha_step(False, x, y)
    ref = ao.MHA64(initial, 2, causal=True, lr=1e-2)
    loss64, grads64 = ref.step(x, y)          # (grad_scales are those of this first evaluation)
    scales = ref.grad_scales
    after64 = ref.loss_and_grads(x, y)[0]
    np.testing.assert_allclose([loss_n, loss_c], loss64, rtol=1e-5)
    np.testing.assert_allclose([after_n, after_c], after64, rtol=1e-5)
    for gn, gc, g64, terms in zip(grads_n, grads_c, grads64, scales):
        for got in (gn, gc):                       # 1e-5 of the sum of |terms| behind every element (attn_oracle.MHA64)
            assert (np.abs(got.reshape(g64.shape) - g64) <= 1e-5 * terms).all()


def test_beyond_the_head_dimension_limit_takes_the_composed_route():
    rs = np.random.RandomState(9)
    d = at.MAX_HEAD_DIM + 1
    q, k, v, do = ao.make_inputs(rs, "bhtd", 1, 2, 20, 33, d, 8, np.float32, q_amp=1.0)
    assert at.plan_attention(q.shape, k.shape, v.shape, native=_lib.get().has_attn).route == "composed"
    with pytest.raises(ValueError, match="native attention route"):
        da.attention(dev(q, np.float32), dev(k, np.float32), dev(v, np.float32), route="native")
    got = run(None, q, k, v, do, False, None, "bhtd", np.float32)
    ao.check(got, ao.reference(q, k, v, do, False, None, "bhtd", np.float32), "D = %d" % d)
