"""tnn_gated_fwd / tnn_gated_bwd on an MI355X (csrc/tnn_gated.hip) against the oracle's derived bounds (tests/gated_oracle.py)
and against the composed route under twice the bound; bit-identity across the access paths, layouts, forced workgroup counts
and repeated calls; untouched padding; the refusals; and the nodes, the block and generation end to end.

Shapes [M, F] — the smallest at which each dispatch edge exists (V = 4 float32 / 2 float64 elements per wide access):
    F in {1, 3, 4, 5, 8} x M in {1, 2, 5}     below, at and above one access; odd F: the element path
    (3, 85), (16, 16), (1, 257)               255, 256 and 257 elements: around one workgroup of element items
    (1, 4099), (4099, 1)                      several workgroups; F = 1: the row carry fires at every step of the walk
Each in four layouts — separate dense arrays, the halves of one packed [M, 2 F], padded rows (ld = F + V: still wide; ld = F + 1:
element), every base moved by one element (element) — and with blocks 0, 1 and 3.  gate starts with 0, -0, +-10, +-40, +-100.
"""

import numpy as np
import pytest

import gated_oracle as go
import gated_support as gs
import tinynn_autograd_amd as tn
from tinynn_autograd_amd import _lib, device_array as da, gated as gt, generation as gen
from tinynn_autograd_amd.core import ops
from tinynn_autograd_amd.core.layers import BLOCK_PARAM_ORDER
from tinynn_autograd_amd.core.tensor import Tensor

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
SHAPES = [(m, f) for f in (1, 3, 4, 5, 8) for m in (1, 2, 5)] + [(3, 85), (16, 16), (1, 257), (1, 4099), (4099, 1)]
bits = gs.bits


def same(a, b):
    return np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def inputs():
    """{(M, F, dtype name): (gate, up, dy, the oracle's result with up, without up)}: computed once, never changed."""
    out = {}
    for act in go.ACTS:
        for dtype in DTYPES:
            for m, f in SHAPES:
                gate, up, dy = go.make_inputs(m, f, go.case_seed("gpu %d %d" % (m, f)), dtype)
                out[act, m, f, np.dtype(dtype).name] = (gate, up, dy, go.reference(gate, up, dy, act, dtype),
                                                       go.reference(gate, None, dy, act, dtype))
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("act", go.ACTS)
def test_shapes_layouts_and_paths(inputs, act, dtype):
    v = gt.VEC // np.dtype(dtype).itemsize
    name = np.dtype(dtype).name
    for m, f in SHAPES:
        gate, up, dy, res, res_plain = inputs[act, m, f, name]
        what = "%s %s [%d, %d]" % (act, name, m, f)
        assert gt.plan_gated(m, f, act, itemsize=np.dtype(dtype).itemsize).wide is (f % v == 0)
        # separate dense arrays, the library's workgroup count: the yardstick of everything below
        y, clean = gs.raw_fwd(act, dtype, gate, up)
        dgate, dup, clean_b = gs.raw_bwd(act, dtype, gate, up, dy)
        assert clean and clean_b, what
        go.check(dict(y=y, dgate=dgate, dup=dup), res, what)
        assert np.isfinite(y).all() and np.isfinite(dgate).all() and np.isfinite(dup).all(), what
        zero = gate == 0
        assert same(y[zero], (gate * up)[zero]), what + ": y(+-0) = +-0 * up"
        assert same(y, gs.raw_fwd(act, dtype, gate, up)[0]), what + ": a repeated call"
        again = gs.raw_bwd(act, dtype, gate, up, dy)
        assert same(dgate, again[0]) and same(dup, again[1]), what + ": a repeated call"
        # layouts and workgroup counts: the same bits, nothing written outside the rows
        variants = [dict(packed=True), dict(ld_extra=v), dict(ld_extra=1), dict(shift=1), dict(packed=True, shift=1),
                    dict(blocks=1), dict(blocks=3), dict(blocks=3, ld_extra=1), dict(blocks=3, packed=True)]
        for kw in variants:
            y2, clean = gs.raw_fwd(act, dtype, gate, up, **kw)
            assert clean and same(y, y2), "%s forward %r" % (what, kw)
            dg2, du2, clean = gs.raw_bwd(act, dtype, gate, up, dy, **kw)
            assert clean and same(dgate, dg2) and same(dup, du2), "%s backward %r" % (what, kw)
        # one output alone
        for kw in (dict(), dict(shift=1)):
            dg2, none, clean = gs.raw_bwd(act, dtype, gate, up, dy, need=(True, False), **kw)
            assert clean and none is None and same(dgate, dg2), what + ": dgate alone"
            none, du2, clean = gs.raw_bwd(act, dtype, gate, up, dy, need=(False, True), **kw)
            assert clean and none is None and same(dup, du2), what + ": dup alone"
        # up == NULL: the plain activation
        a, clean = gs.raw_fwd(act, dtype, gate, None)
        da_, none, clean_b = gs.raw_bwd(act, dtype, gate, None, dy, need=(True, False))
        assert clean and clean_b and none is None
        go.check(dict(y=a, dgate=da_), res_plain, what + " without up")
        for kw in (dict(shift=1), dict(ld_extra=1), dict(blocks=3)):
            assert same(a, gs.raw_fwd(act, dtype, gate, None, **kw)[0]), "%s without up %r" % (what, kw)
            assert same(da_, gs.raw_bwd(act, dtype, gate, None, dy, need=(True, False), **kw)[0]), "%s without up %r" % (what, kw)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("act", go.ACTS)
def test_native_against_composed(inputs, act, dtype):
    """Two implementations within the bound of the truth lie within twice the bound of each other.  The exact GELU gate has no
    composed form (no erf among the generic operations): there the composed route refuses."""
    for m, f in ((5, 8), (3, 85)):
        gate, up, dy, res, _ = inputs[act, m, f, np.dtype(dtype).name]
        if act == "gelu":
            with pytest.raises(ValueError, match="exact \\(erf\\) GELU gate needs the native route"):
                gs.composed(act, dtype, gate, up, dy)
            continue
        comp = gs.composed(act, dtype, gate, up, dy)
        g, u, d = (tn.asarray(a, dtype=dtype) for a in (gate, up, dy))
        y = np.asarray(da.gated(g, u, act=act, route="native"))
        dgate, dup = (np.asarray(a) for a in da.gated_bwd(g, u, d, act=act, route="native"))
        assert same(y, gs.raw_fwd(act, dtype, gate, up)[0])                              # device_array makes the raw call
        for field, got in (("y", y), ("dgate", dgate), ("dup", dup)):
            assert (np.abs(got.astype(np.float64) - comp[field].astype(np.float64)) <= 2 * res.bounds[field]).all(), field
        # the packed entry points: the halves in place, the packed dz
        z = tn.asarray(np.concatenate([gate, up], axis=1), dtype=dtype)
        assert same(y, np.asarray(da.gated(z, act=act, packed=True)))
        dz = np.asarray(da.gated_bwd(z, None, d, act=act, packed=True))
        assert dz.shape == (m, 2 * f) and same(dz[:, :f], dgate) and same(dz[:, f:], dup)


def test_refusals_of_the_entry_points():
    """What the host can see is refused before any launch — the output still holds its sentinel afterwards."""
    lib = _lib.get()
    M, F = 4, 8
    g, u, d = (gs.Buf(M, F, F, 0, np.float32, np.ones((M, F))) for _ in range(3))
    z = gs.Buf(M, 2 * F, 2 * F, 0, np.float32, np.ones((M, 2 * F)))
    out, out2 = gs.Buf(M, 2 * F, 2 * F, 0, np.float32), gs.Buf(M, F, F, 0, np.float32)
    i64 = da._i64arr

    def fwd(gate=g.ptr, up=u.ptr, y=out2.ptr, m=M, f=F, strides=(F, F, F), act=0, blocks=0, dtype=_lib.F32):
        lib.gated_fwd(gate, up, y, m, f, None if strides is None else i64(strides), act, blocks, dtype)

    def bwd(gate=g.ptr, up=u.ptr, dy=d.ptr, dgate=out.ptr, dup=out.column(F), m=M, f=F, strides=(F, F, F, 2 * F, 2 * F), act=0,
            blocks=0, dtype=_lib.F32):
        lib.gated_bwd(gate, up, dy, dgate, dup, m, f, None if strides is None else i64(strides), act, blocks, dtype)

    for call, cases in ((fwd, [(dict(f=0), "F 0"), (dict(m=-1), "M -1"), (dict(strides=(F - 1, F, F)), "stride 7 of gate"),
                               (dict(strides=(F, F - 1, F)), "stride 7 of up"), (dict(strides=(F, F, F - 1)), "stride 7 of y"),
                               (dict(act=3), "act 3"), (dict(act=-1), "act -1"), (dict(dtype=_lib.I64), "float32 and float64"),
                               (dict(gate=None), "null operand"), (dict(y=None), "null operand"), (dict(strides=None), "null strides"),
                               (dict(m=1 << 15, f=1 << 16, strides=(1 << 16,) * 3), "2\\^31 elements or more"),
                               (dict(blocks=gt.MAX_BLOCKS + 1), "blocks"), (dict(blocks=-1), "blocks"),
                               (dict(y=g.ptr), "y overlaps an input"), (dict(y=u.ptr + 4 * (M * F - 1)), "y overlaps an input"),
                               (dict(gate=z.ptr, up=z.column(F), strides=(2 * F, 2 * F, F), y=z.column(2 * F)), "y overlaps")]),
                        (bwd, [(dict(f=0), "F 0"), (dict(m=-1), "M -1"), (dict(strides=(F, F, F - 1, 2 * F, 2 * F)), "stride 7 of dy"),
                               (dict(strides=(F, F, F, F - 1, 2 * F)), "stride 7 of dgate"),
                               (dict(strides=(F, F, F, 2 * F, F - 1)), "stride 7 of dup"), (dict(act=3), "act 3"),
                               (dict(dtype=_lib.I64), "float32 and float64"), (dict(dy=None), "null operand"),
                               (dict(dgate=None, dup=None), "null operand"), (dict(up=None), "dup without up"),
                               (dict(dgate=d.ptr), "an output overlaps an input"), (dict(dup=g.ptr), "an output overlaps an input"),
                               (dict(dup=out.column(F - 1)), "dgate and dup share elements"),
                               (dict(dup=out.ptr), "dgate and dup share elements"),
                               (dict(strides=(F, F, F, 2 * F, 2 * F + 1)), "dgate and dup share elements"),
                               (dict(blocks=gt.MAX_BLOCKS + 1), "blocks")])):
        for kw, match in cases:
            with pytest.raises(_lib.TnnError, match=match):
                call(**kw)
    tn.synchronize()
    for buf in (out, out2, g, u, d, z):
        rows, clean = buf.read()
        assert clean and same(rows, buf.before[buf.rows].reshape(rows.shape))            # nothing was launched
    # M == 0: nothing is read or written, whatever the pointers
    fwd(m=0, gate=None, up=None, y=None)
    bwd(m=0, gate=None, up=None, dy=None, dgate=None, dup=None)
    # and the accepted forms of the output rule: halves of one dz, bases F apart
    bwd()
    tn.synchronize()
    both, clean = out.read()
    assert clean and not (both == gs.SENTINEL).any()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_nodes_launch_once(dtype, monkeypatch):
    """ops.gated_ packed and two-tensor and ops.silu_: ONE launch forward and ONE backward each, within the derived bounds."""
    tn.set_default_float(dtype)
    lib = _lib.get()
    calls = []
    for short in ("gated_fwd", "gated_bwd"):
        real = getattr(lib, short)
        monkeypatch.setattr(lib, short, lambda *a, _r=real, _s=short: calls.append(_s) or _r(*a))
    gate, up, dy = go.make_inputs(5, 8, go.case_seed("nodes"), dtype)
    res = go.reference(gate, up, dy, "silu", dtype)
    g, u = (Tensor(a, requires_grad=True, dtype=dtype) for a in (gate, up))
    y = ops.gated_(g, u)
    (y * Tensor(dy, dtype=dtype)).sum().backward()
    assert calls == ["gated_fwd", "gated_bwd"]
    go.check(dict(y=np.asarray(y.values), dgate=np.asarray(g.grad), dup=np.asarray(u.grad)), res, "two-tensor node")
    del calls[:]
    z = Tensor(np.concatenate([gate, up], axis=1), requires_grad=True, dtype=dtype)
    y2 = ops.gated_(z, packed=True)
    (y2 * Tensor(dy, dtype=dtype)).sum().backward()
    assert calls == ["gated_fwd", "gated_bwd"]
    dz = np.asarray(z.grad)
    assert same(np.asarray(y2.values), np.asarray(y.values)) and same(dz[:, :8], np.asarray(g.grad)) and same(dz[:, 8:], np.asarray(u.grad))
    del calls[:]
    x = Tensor(gate, requires_grad=True, dtype=dtype)
    s = ops.silu_(x)
    (s * Tensor(dy, dtype=dtype)).sum().backward()
    assert calls == ["gated_fwd", "gated_bwd"]
    go.check(dict(y=np.asarray(s.values), dgate=np.asarray(x.grad)), go.reference(gate, None, dy, "silu", dtype), "silu node")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("hidden", [24, 10])
@pytest.mark.parametrize("mlp", ["swiglu", "geglu"])
def test_block_against_the_float64_oracle(mlp, hidden, dtype):
    """TransformerBlock(mlp=) at E 16, B 2, T 5, forward and backward on the device against the float64 replica; hidden 24: the
    gate takes the wide path, hidden 10: the element path (float32).  Tolerances relative to the largest entry of a tensor:
    float64 1e-10 (what tests/test_gpu_norm.py asks of the plain block); float32 1e-4 — sums of at most B T hidden = 240 terms
    with relative rounding 2^-24 each through six chained products and normalisations: 240 x 6 x 6e-8 = 9e-5."""
    e, heads, b, t = 16, 2, 2, 5
    if dtype == np.float32:
        assert gt.plan_gated(b * t, hidden, lds=dict(gate=2 * hidden, up=2 * hidden),
                             addresses=dict(up=hidden * 4), itemsize=4).wide is (hidden == 24)
    rs = np.random.RandomState(go.case_seed("gpu block %s %d" % (mlp, hidden)))
    params = go.block_params(rs.randint(1 << 30), e, hidden)
    x, y = rs.randn(b, t, e), rs.randn(b, t, e)
    want_loss, want, bk_terms = go.block_loss(params, x, y, heads, True, 1e-5, mlp, grads=True, with_bk_terms=True)
    scales = {name: np.abs(want[name]).max() for name in BLOCK_PARAM_ORDER}
    scales["attn.bk"] = bk_terms.max()           # its gradient is zero: a sum of terms that cancel is judged against their sizes
    tol = 1e-10 if dtype == np.float64 else 1e-4
    blk = gs.block(params, heads, hidden, dtype, mlp=mlp)
    loss, grads = gs.block_grads(blk, x, y, dtype)
    assert abs(loss - want_loss) <= tol * abs(want_loss)
    for name in BLOCK_PARAM_ORDER:
        assert np.abs(grads[name] - want[name]).max() <= tol * scales[name], name
    slow = gs.block(params, heads, hidden, dtype, mlp=mlp, fused=False)
    loss2, grads2 = gs.block_grads(slow, x, y, dtype)
    assert abs(loss2 - want_loss) <= tol * abs(want_loss)
    for name in BLOCK_PARAM_ORDER:
        assert np.abs(grads2[name] - want[name]).max() <= tol * scales[name], "fused=False " + name


def test_captured_ragged_generation_from_a_gated_block():
    """The one-block swiglu model (E 16, hidden 24), greedy, 6 tokens: the captured ragged step picks the eager tokens; every
    step's top-2 margin is far above float32 rounding."""
    c = gs.LM
    net, prompt = gs.lm_net(np.float32)
    tn.set_default_float(np.float32)
    eager = gen.generate(net, prompt, c["new"], temperature=0.0)
    for n in range(c["new"]):
        assert gs.lm_margin(net, eager[:, :c["prompt"] + n]) > 1e-2
    lens = np.full((c["B"],), c["prompt"], dtype=np.int64)
    ragged = np.asarray(gen.generate(net, prompt, c["new"], temperature=0.0, prompt_lens=lens))
    captured = np.asarray(gen.generate(net, prompt, c["new"], temperature=0.0, prompt_lens=lens, capture=True))
    assert c["new"] == 6 and np.array_equal(ragged, eager) and np.array_equal(captured, eager)
