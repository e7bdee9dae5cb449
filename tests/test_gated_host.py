"""The gated activations above the C-ABI, on whatever backend the suite runs on (the CPU twin: the composed route): the ops
nodes ops.gated_ (packed and two-tensor) and ops.silu_ with their vjps, the SiLU layer, TransformerBlock(mlp=) with its
parameters, its full backward and its launch sequence, and generation from a gated model."""

import numpy as np
import pytest

import gated_oracle as go
import gated_support as gs
import norm_oracle as no
import tinynn_autograd_amd as tn
from tinynn_autograd_amd import device_array as da, generation as gen
from tinynn_autograd_amd.core import ops
from tinynn_autograd_amd.core.layers import BLOCK_PARAM_ORDER, SiLU, TransformerBlock
from tinynn_autograd_amd.core.tensor import Tensor

ON_TWIN = tn.backend_name() != "hip-gfx950"
COMPOSED = ("silu", "gelu_tanh")                     # the acts that have a composed form (the exact GELU gate is native only)
ACTS = COMPOSED if ON_TWIN else go.ACTS
# the twin's composed route spends one rounding more than the fixed expression (test_gated_golden.py)
FACTOR = 2.0 if ON_TWIN else 1.0


def tensors(dtype, *arrays):
    return tuple(Tensor(np.asarray(a, dtype=dtype), requires_grad=True, dtype=dtype) for a in arrays)


def central(f, x, h):
    return (f(x + h) - f(x - h)) / (2 * h)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("act", ACTS)
def test_two_tensor_node(act, dtype):
    """Values and both vjps against the oracle, and the oracle's gradients against a float64 central difference (truncation
    h^2 / 3 per unit of |dy up|, rounding 4 u64 (|g| + 1)(|up| + 1) / h)."""
    tn.set_default_float(dtype)
    gate, up, dy = go.make_inputs(5, 7, go.case_seed("two" + act), dtype)
    res = go.reference(gate, up, dy, act, dtype)
    g, u = tensors(dtype, gate, up)
    y = ops.gated_(g, u, act=act)
    (y * Tensor(dy, dtype=dtype)).sum().backward()
    got = dict(y=np.asarray(y.values), dgate=np.asarray(g.grad), dup=np.asarray(u.grad))
    assert all(v.dtype == dtype for v in got.values())
    go.check(got, res, "gated_ %s %s" % (act, np.dtype(dtype).name), factor=FACTOR)
    h = 1e-5
    g64, u64, d64 = (a.astype(np.float64) for a in (gate, up, dy))
    rounding = 4 * no.U64 * (np.abs(g64) + 1) * (np.abs(u64) + 1) / h
    cd_g = central(lambda x: go.act64(x, act)[0] * u64, g64, h)
    cd_u = central(lambda x: go.act64(g64, act)[0] * x, u64, h)
    assert (np.abs(cd_g * d64 - res.values["dgate"]) <= np.abs(d64) * (np.abs(u64) * h * h / 3 + rounding)).all()
    assert (np.abs(cd_u * d64 - res.values["dup"]) <= np.abs(d64) * rounding).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("act", ACTS)
def test_packed_node(act, dtype):
    """The packed form equals the two-tensor form bit for bit, its vjp is the packed dz [.., 2 F], leading axes are kept."""
    tn.set_default_float(dtype)
    gate, up, dy = go.make_inputs(6, 5, go.case_seed("packed" + act), dtype)
    res = go.reference(gate, up, dy, act, dtype)
    (z,) = tensors(dtype, np.concatenate([gate, up], axis=1).reshape(2, 3, 10))
    y = ops.gated_(z, act=act, packed=True)
    assert tuple(y.shape) == (2, 3, 5)
    (y * Tensor(dy.reshape(2, 3, 5), dtype=dtype)).sum().backward()
    dz = np.asarray(z.grad).reshape(6, 10)
    got = dict(y=np.asarray(y.values).reshape(6, 5), dgate=dz[:, :5], dup=dz[:, 5:])
    go.check(got, res, "packed gated_ %s %s" % (act, np.dtype(dtype).name), factor=FACTOR)
    g, u = tensors(dtype, gate, up)
    y2 = ops.gated(g, u, act=act)
    (y2 * Tensor(dy, dtype=dtype)).sum().backward()
    for a, b in ((got["y"], y2.values), (got["dgate"], g.grad), (got["dup"], u.grad)):
        assert np.array_equal(gs.bits(a), gs.bits(np.asarray(b)))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_silu_node_and_layer(dtype):
    tn.set_default_float(dtype)
    gate, _, dy = go.make_inputs(4, 9, go.case_seed("silu"), dtype)
    res = go.reference(gate, None, dy, "silu", dtype)
    for make in (ops.silu_, ops.silu, lambda t: SiLU().forward(t), lambda t: ops.gated_(t, act="silu")):
        (x,) = tensors(dtype, gate)
        y = make(x)
        (y * Tensor(dy, dtype=dtype)).sum().backward()
        go.check(dict(y=np.asarray(y.values), dgate=np.asarray(x.grad)), res, "silu %s" % np.dtype(dtype).name, factor=FACTOR)
    y = np.asarray(ops.silu_(Tensor(gate, dtype=dtype)).values).reshape(-1)
    assert np.isfinite(y).all() and y[0] == 0 and not np.signbit(y[0]) and y[1] == 0 and np.signbit(y[1])      # silu(+-0) = +-0
    h = 1e-5
    g64, d64 = gate.astype(np.float64), dy.astype(np.float64)
    cd = central(lambda x: go.act64(x, "silu")[0], g64, h)
    assert (np.abs(cd * d64 - res.values["dgate"]) <= np.abs(d64) * (h * h / 3 + 4 * no.U64 * (np.abs(g64) + 1) / h)).all()


def test_a_gradient_only_to_the_side_that_requires_it(monkeypatch):
    gate, up, dy = go.make_inputs(3, 8, 11, np.float32)
    res = go.reference(gate, up, dy, "silu", np.float32)
    for need_g, need_u in ((True, False), (False, True)):
        g = Tensor(gate, requires_grad=need_g)
        u = Tensor(up, requires_grad=need_u)
        y = ops.gated_(g, u)
        asked = []
        real = da.gated_bwd
        monkeypatch.setattr(da, "gated_bwd", lambda *a, **k: asked.append((k["need_dgate"], k["need_dup"])) or real(*a, **k))
        (y * Tensor(dy)).sum().backward()
        monkeypatch.setattr(da, "gated_bwd", real)
        assert asked == [(need_g, need_u)]                                   # ONE backward call, for that side alone
        assert (g.grad is None) == (not need_g) and (u.grad is None) == (not need_u)
        got = dict(dgate=None if not need_g else np.asarray(g.grad), dup=None if not need_u else np.asarray(u.grad))
        go.check(got, res, "one side", factor=FACTOR)
    y = ops.gated_(Tensor(gate), Tensor(up))
    assert not y.requires_grad


def test_arguments():
    x = Tensor(np.zeros((2, 4), dtype=np.float32))
    for f in (ops.gated_, ops.gated, ops.silu_, ops.silu):
        with pytest.raises(TypeError, match="unsupported arguments \\['bf16'\\]"):
            f(x, bf16=True)
    with pytest.raises(ValueError, match="act must be one of"):
        ops.gated_(x, x, act="relu")
    with pytest.raises(ValueError, match="packed=True takes ONE array"):
        ops.gated_(x, x, packed=True)
    with pytest.raises(ValueError, match="its last axis must be even"):
        ops.gated_(Tensor(np.zeros((2, 3), dtype=np.float32)), packed=True)
    with pytest.raises(ValueError, match="gate and up must have one shape"):
        ops.gated_(x, Tensor(np.zeros((2, 5), dtype=np.float32)))
    with pytest.raises(ValueError, match="exact \\(erf\\) GELU gate needs the native route"):
        ops.gated_(x, x, act="gelu", route="composed")
    with pytest.raises(ValueError, match="mlp must be one of"):
        TransformerBlock(2, mlp="relu")
    assert tuple(ops.gated_(Tensor(np.zeros((0, 4), dtype=np.float32)), packed=True).shape) == (0, 2)


# ---------------------------------------------------------------------- TransformerBlock(mlp=)
def test_block_parameters():
    np.random.seed(3)
    plain = TransformerBlock(2, num_in=8)
    np.random.seed(3)
    gated = TransformerBlock(2, num_in=8, mlp="swiglu")
    assert list(gated.params) == list(plain.params) == list(BLOCK_PARAM_ORDER)
    assert plain.hidden == 32 and gated.hidden == 24                          # 4 E; 8 E / 3 rounded up to a multiple of 8
    want = dict(no.block_shapes(8, 24), **{"fc1.w": (8, 48), "fc1.b": (1, 48)})
    assert {k: tuple(v.shape) for k, v in gated.params.items()} == want
    assert {k: tuple(v.shape) for k, v in plain.params.items()} == no.block_shapes(8, 32)
    # the host RNG is drawn in the same order: everything in front of fc1 is the same draw
    for name in BLOCK_PARAM_ORDER[:BLOCK_PARAM_ORDER.index("fc1.w")]:
        assert np.array_equal(np.asarray(gated.params[name].values), np.asarray(plain.params[name].values)), name
    assert tuple(TransformerBlock(2, hidden=12, num_in=8, mlp="geglu").params["fc1.w"].shape) == (8, 24)
    assert TransformerBlock(2, num_in=8, mlp="gelu").hidden == 32


@pytest.mark.parametrize("mlp", ["swiglu", "geglu"])
def test_block_backward_against_finite_differences(mlp):
    """E 8, hidden 12, heads 2, B 2, T 3 in float64: every parameter's gradient from the autograd graph against the central
    difference of the float64 replica's loss (h = 1e-5: truncation h^2 / 6 |L'''| and rounding 4 u64 |L| / h are both below
    1e-8 (|L| + max|grad|) here), and against the replica's analytic gradients."""
    e, hidden, heads, b, t = 8, 12, 2, 2, 3
    rs = np.random.RandomState(go.case_seed("block" + mlp))
    params = go.block_params(rs.randint(1 << 30), e, hidden)
    x, y = rs.randn(b, t, e), rs.randn(b, t, e)
    blk = gs.block(params, heads, hidden, np.float64, mlp=mlp)
    loss, grads = gs.block_grads(blk, x, y, np.float64)
    want_loss, want = go.block_loss(params, x, y, heads, True, 1e-5, mlp, grads=True)
    assert abs(loss - want_loss) <= 1e-12 * abs(want_loss)
    h = 1e-5
    scale = abs(want_loss) + max(np.abs(g).max() for g in want.values())
    for name in BLOCK_PARAM_ORDER:
        assert grads[name].shape == want[name].shape, name
        assert np.abs(grads[name] - want[name]).max() <= 1e-11 * scale, name
        fd = np.zeros_like(want[name])
        for idx in np.ndindex(*fd.shape):
            moved = dict(params)
            for sign in (1.0, -1.0):
                moved[name] = params[name].copy()
                moved[name][idx] += sign * h
                fd[idx] += sign * go.block_loss(moved, x, y, heads, True, 1e-5, mlp)
        fd /= 2 * h
        assert np.abs(grads[name] - fd).max() <= 1e-8 * scale, name


def test_block_set_parameters_round_trip():
    from tinynn_autograd_amd.core.nn import Net
    np.random.seed(1)
    net = Net([TransformerBlock(2, hidden=12, num_in=8, causal=True, mlp="swiglu")])
    x = Tensor(np.random.RandomState(2).randn(2, 3, 8).astype(np.float32))
    first = np.asarray(net.forward(x).values)
    params = net.get_parameters()
    assert list(params[0]) == list(BLOCK_PARAM_ORDER) and tuple(params[0]["fc1.w"].shape) == (8, 24)
    np.random.seed(9)
    other = Net([TransformerBlock(2, hidden=12, num_in=8, causal=True, mlp="swiglu")])
    assert not np.array_equal(np.asarray(other.forward(x).values), first)
    other.set_parameters(params)
    assert np.array_equal(np.asarray(other.forward(x).values), first)


def test_default_block_issues_the_launches_it_did(monkeypatch):
    """TransformerBlock() and TransformerBlock(mlp="gelu") run one sequence of native calls, forward and backward, without a
    gated call in it; the gated block replaces the GELU pair by the gated pair and changes nothing else."""
    seen = gs.count_calls(monkeypatch)
    x = np.random.RandomState(4).randn(2, 5, 16).astype(np.float32)

    def trace(**kw):
        np.random.seed(6)
        blk = TransformerBlock(2, hidden=24, num_in=16, causal=True, **kw)
        del seen[:]
        out = blk.forward(Tensor(x, requires_grad=True))
        (out * out).sum().backward()
        return list(seen)

    trace()                                              # (the first run also uploads what later runs find cached)
    default, named, swiglu = trace(), trace(mlp="gelu"), trace(mlp="swiglu")
    assert default == named and default
    assert not [c for c in default if c.startswith("gated")]
    if not ON_TWIN:
        assert default.count("gelu_fwd") == 1 and default.count("gelu_bwd") == 1
        assert swiglu.count("gated_fwd") == 1 and swiglu.count("gated_bwd") == 1
        assert [c.replace("gated", "gelu") for c in swiglu] == default


def test_generation_from_a_gated_model():
    """A one-block swiglu model, greedy: the uniform path (cached and uncached) and the ragged path at uniform lengths pick the
    same tokens; every step's top-2 logit margin is far above float32 rounding, so the comparison is not a coin toss."""
    c = gs.LM
    net, prompt = gs.lm_net(np.float32)
    tn.set_default_float(np.float32)
    eager = gen.generate(net, prompt, c["new"], temperature=0.0)
    assert eager.shape == (c["B"], c["prompt"] + c["new"]) and np.array_equal(eager[:, :c["prompt"]], prompt)
    for n in range(c["new"]):
        assert gs.lm_margin(net, eager[:, :c["prompt"] + n]) > 1e-2
    assert np.array_equal(gen.generate(net, prompt, c["new"], temperature=0.0, cache=False), eager)
    lens = np.full((c["B"],), c["prompt"], dtype=np.int64)
    assert np.array_equal(np.asarray(gen.generate(net, prompt, c["new"], temperature=0.0, prompt_lens=lens)), eager)
