"""Layer norm, RMS norm, GELU and the TransformerBlock on the CPU test twin, where everything takes the composed route: the
raw calls within the oracle's derived bounds on every fixture case, the ops-level vjps in all their optional-operand forms,
the layers' parameter bookkeeping, and the block against the fixture that torch produced in float64."""

import numpy as np
import pytest

import norm_oracle as no
import norm_support as ns
import tinynn_autograd_amd as tn
from tinynn_autograd_amd import device_array as da
from tinynn_autograd_amd.core import ops
from tinynn_autograd_amd.core.layers import (BLOCK_PARAM_ORDER, GELU, MHA_PARAM_ORDER, NORM_PARAM_ORDER, Dense, LayerNorm,
                                             RMSNorm, TransformerBlock)
from tinynn_autograd_amd.core.nn import Net
from tinynn_autograd_amd.core.tensor import Tensor


@pytest.fixture(scope="module")
def golden():
    return ns.load_golden()


@pytest.fixture(autouse=True)
def _switches():
    yield
    da.NORM_ROUTE = None


def leaf(a, dtype=np.float32):
    if a is None:
        return None
    t = Tensor(np.asarray(a, dtype=dtype), requires_grad=True, dtype=dtype)
    t.zero_grad()
    return t


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", sorted(no.NORM_CASES))
def test_composed_route_within_the_bounds(golden, name, dtype):
    tn.set_default_float(dtype)
    (x, gamma, beta, dy, kind, eps), res = ns.golden_result(golden, name, dtype)
    got = ns.run(None, x, gamma, beta, dy, kind, eps, dtype)
    no.check(got, res, "%s %s composed" % (name, np.dtype(dtype).name))
    assert got["y"].dtype == dtype and got["rstd"].shape == x.shape[:-1]
    for need in ((True, False, False), (False, True, False), (False, False, True)):
        part = ns.run("composed", x, gamma, beta, dy, kind, eps, dtype, need=need)
        wanted = (need[0], need[1], need[2] and kind == "layer")
        assert [part[f] is not None for f in ("dx", "dgamma", "dbeta")] == list(wanted)
        no.check(part, res, "%s %s composed %s" % (name, np.dtype(dtype).name, need))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", sorted(no.GELU_CASES))
def test_gelu_tanh_composed_and_exact_raises(golden, name, dtype):
    tn.set_default_float(dtype)
    form = no.GELU_CASES[name]
    x, dy = no.gelu_input(40, no.case_seed(name), dtype)
    if form == "none":
        with pytest.raises(ValueError, match="exact .erf. GELU needs the native route"):
            ops.gelu(x)
        return
    res = no.gelu_reference(x, dy, form, dtype)
    res.values["y"], res.values["dx"] = golden[name]
    xt = leaf(x, dtype)
    out = ops.gelu(xt, approximate=form)
    out.backward(dy)
    no.check(dict(y=out.values, dx=xt.grad), res, "gelu %s" % form, fields=("y", "dx"))
    np.testing.assert_array_equal(np.asarray(out.values)[:2], [0.0, 0.0])


@pytest.mark.parametrize("kind", ["layer", "rms"])
def test_ops_vjps_in_every_optional_form(kind):
    """gamma / beta present or None, each input with or without requires_grad: every gradient that is asked for lies within
    the oracle's bounds, nothing else gets one, and the per-edge vjps agree with the fused one."""
    rs = np.random.RandomState(11)
    x, gamma, beta, dy = no.make_inputs(rs, (3, 2, 7))
    node = ops.layer_norm_ if kind == "layer" else ops.rms_norm_
    for has_gamma in (True, False):
        for has_beta in ((True, False) if kind == "layer" else (False,)):
            g, b = (gamma if has_gamma else None), (beta if has_beta else None)
            res = no.reference(x, g, b, dy, kind, 1e-5)
            for grads in ((True, True, True), (False, True, True), (True, False, False), (False, False, True)):
                xt = leaf(x) if grads[0] else Tensor(x)
                gt = None if g is None else (leaf(g.reshape(1, 7)) if grads[1] else Tensor(g.reshape(1, 7)))
                bt = None if b is None else (leaf(b) if grads[2] else Tensor(b))
                args = (xt, gt, bt) if kind == "layer" else (xt, gt)
                out = node(*args, eps=1e-5)
                assert out.requires_grad == any(t is not None and t.requires_grad for t in (xt, gt, bt))
                assert len(out.dependency) == sum(t is not None and t.requires_grad for t in (xt, gt, bt))
                no.assert_within(out.values, res.values["y"], res.bounds["y"], "%s y" % kind)
                if not out.requires_grad:
                    continue
                out.backward(dy)
                for t, field in ((xt, "dx"), (gt, "dgamma"), (bt, "dbeta")):
                    if t is None:
                        continue
                    if not t.requires_grad:
                        assert t.grad is None
                        continue
                    assert tuple(t.grad.shape) == tuple(t.shape)
                    no.assert_within(np.asarray(t.grad).reshape(res.values[field].shape), res.values[field],
                                     res.bounds[field], "%s %s" % (kind, field))
                for dep in out.dependency:                              # the per-edge forms
                    single = np.asarray(dep["grad_fn"](tn.asarray(dy)))
                    np.testing.assert_array_equal(single.reshape(dep["tensor"].shape), np.asarray(dep["tensor"].grad))


def test_rejected_arguments_and_promotion():
    x = Tensor(np.ones((2, 4), dtype=np.float32))
    for fn in (ops.layer_norm_, ops.layer_norm, ops.rms_norm_, ops.rms_norm, ops.gelu_, ops.gelu):
        with pytest.raises(TypeError, match="unsupported arguments"):
            fn(x, dropout=0.1)
    with pytest.raises(TypeError, match="unsupported arguments"):
        ops.rms_norm(x, None, beta=np.zeros(4))
    with pytest.raises(ValueError, match="gamma must hold"):
        ops.layer_norm(x, np.ones(3))
    with pytest.raises(ValueError, match="eps must be"):
        ops.layer_norm(x, eps=-1.0)
    with pytest.raises(ValueError, match="route must be"):
        ops.layer_norm_(x, route="quick")
    with pytest.raises(ValueError, match="approximate must be"):
        ops.gelu(x, approximate="fast")
    assert ops.layer_norm(np.arange(8).reshape(2, 4)).values.dtype == np.float32          # integers are promoted
    mixed = da.layer_norm(tn.asarray(np.ones((2, 4), dtype=np.float32)), tn.asarray(np.ones(4), dtype=np.float64))
    assert mixed[0].dtype == np.float64 and mixed[1].dtype == np.float64
    xt = leaf(np.zeros((0, 4)))
    gt = leaf(np.ones((1, 4)))
    out = ops.layer_norm_(xt, gt)
    assert out.shape == (0, 4)
    out.backward(np.zeros((0, 4), dtype=np.float32))
    assert gt.grad.shape == (1, 4) and not np.asarray(gt.grad).any()


def test_layers_lazy_width_order_and_shapes():
    assert NORM_PARAM_ORDER == ("gamma", "beta")
    x = Tensor(np.random.RandomState(0).randn(2, 3, 5, 6).astype(np.float32))
    for cls, names in ((LayerNorm, ("gamma", "beta")), (RMSNorm, ("gamma",))):
        lazy = cls()
        assert not lazy.is_init and list(lazy.params) == list(names) and all(p is None for p in lazy.params.values())
        out = lazy.forward(x)
        assert lazy.is_init and out.shape == x.shape and list(lazy.params) == list(names)
        for name in names:
            assert tuple(lazy.params[name].shape) == (1, 6) and lazy.params[name].requires_grad
            np.testing.assert_array_equal(np.asarray(lazy.params[name].values), np.full((1, 6), float(name == "gamma")))
        eager = cls(num_in=6, eps=1e-3, fused=False)
        assert eager.is_init and eager.eps == 1e-3
        assert eager.forward(Tensor(np.ones((6,), dtype=np.float32))).shape == (6,)           # rank 1
        with pytest.raises(ValueError, match="differs from the layer's"):
            eager.forward(Tensor(np.ones((2, 5), dtype=np.float32)))
        res = no.reference(np.asarray(x.values), kind="layer" if cls is LayerNorm else "rms", eps=1e-5)
        no.assert_within(out.values, res.values["y"], res.bounds["y"], cls.__name__)
    assert GELU("tanh").forward(Tensor(np.zeros((2, 2), dtype=np.float32))).shape == (2, 2)
    assert GELU().approximate == "none"
    with pytest.raises(ValueError, match="approximate must be"):
        GELU("quick")


def test_block_parameter_order_shapes_and_rng_draws():
    assert BLOCK_PARAM_ORDER == (("ln1.gamma", "ln1.beta") + tuple("attn." + n for n in MHA_PARAM_ORDER)
                                 + ("ln2.gamma", "ln2.beta", "fc1.w", "fc1.b", "fc2.w", "fc2.b"))
    assert BLOCK_PARAM_ORDER == no.BLOCK_NAMES
    np.random.seed(4)
    lazy = TransformerBlock(2)
    assert not lazy.is_init and list(lazy.params) == list(BLOCK_PARAM_ORDER) and all(p is None for p in lazy.params.values())
    np.random.seed(4)
    eager = TransformerBlock(2, num_in=8)
    shapes = no.block_shapes(8, 32)                                              # hidden defaults to 4 E
    assert eager.hidden == 32
    x = Tensor(np.random.RandomState(0).randn(2, 5, 8).astype(np.float32))
    np.random.seed(4)
    out = lazy.forward(x)
    assert lazy.is_init and out.shape == (2, 5, 8)
    for name in BLOCK_PARAM_ORDER:
        assert tuple(lazy.params[name].shape) == shapes[name], name
        np.testing.assert_array_equal(np.asarray(lazy.params[name].values), np.asarray(eager.params[name].values))
    # the host RNG is drawn in BLOCK_PARAM_ORDER: the same seed gives the weights of the parts built one after the other
    np.random.seed(4)
    from tinynn_autograd_amd.core.layers import MultiHeadAttention
    attn, fc1, fc2 = MultiHeadAttention(2, num_in=8), Dense(32, num_in=8), Dense(8, num_in=32)
    np.testing.assert_array_equal(np.asarray(attn.params["wo"].values), np.asarray(eager.params["attn.wo"].values))
    np.testing.assert_array_equal(np.asarray(fc1.params["w"].values), np.asarray(eager.params["fc1.w"].values))
    np.testing.assert_array_equal(np.asarray(fc2.params["w"].values), np.asarray(eager.params["fc2.w"].values))
    net = Net([Dense(8, num_in=8), eager])
    assert net.parameter_tensors()[2:] == [eager.params[n] for n in BLOCK_PARAM_ORDER]
    assert net.num_parameters() == 72 + sum(int(np.prod(s)) for s in shapes.values())
    assert TransformerBlock(2, hidden=12, num_in=8).params["fc1.w"].shape == (8, 12)
    with pytest.raises(ValueError, match="multiple of num_heads"):
        TransformerBlock(3, num_in=8)
    with pytest.raises(ValueError, match=r"\[B, T, E\]"):
        eager.forward(Tensor(np.ones((5, 8), dtype=np.float32)))
    with pytest.raises(ValueError, match="differs from the block's"):
        eager.forward(Tensor(np.ones((1, 5, 4), dtype=np.float32)))


def test_net_parameters_round_trip():
    np.random.seed(6)
    a, b = Net([TransformerBlock(2, num_in=8, hidden=12)]), Net([TransformerBlock(2, num_in=8, hidden=12)])
    x = Tensor(np.random.RandomState(1).randn(2, 4, 8).astype(np.float32))
    before = np.asarray(b.forward(x).values)
    want = np.asarray(a.forward(x).values)
    assert not np.array_equal(before, want)
    b.set_parameters(a.get_parameters())
    assert all(b.layers[0].params[n] is a.layers[0].params[n] for n in BLOCK_PARAM_ORDER)
    np.testing.assert_array_equal(np.asarray(b.forward(x).values), want)       # the parts read the dict's tensors
    with pytest.raises(AssertionError):
        b.set_parameters([{n: a.layers[0].params[n] for n in BLOCK_PARAM_ORDER[:-1]}])


@pytest.mark.parametrize("fused", [True, False])
def test_block_against_the_fixture_in_float64(golden, fused):
    """Gradients: max|diff| <= 1e-10 max|ref| per tensor.  Losses of three Adam steps: 1e-7 relative — Adam's normalisation
    amplifies float64 rounding by at most 1 / 1e-8 of lr, which leaves three orders of margin."""
    tn.set_default_float(np.float64)
    losses, grads = ns.block_run(golden, fused, np.float64, no.BLOCK_CASE["steps"])
    ns.assert_block_grads(grads, golden, 1e-10, "float64 fused=%s" % fused)
    np.testing.assert_allclose(losses, golden["block.adam_losses"], rtol=1e-7)
    np.testing.assert_allclose(losses[0], float(golden["block.loss"]), rtol=1e-12)


def test_block_in_float32_within_the_reference_gate(golden):
    losses, grads = ns.block_run(golden, True, np.float32, 1)
    ns.assert_block_grads(grads, golden, golden["block.f32_gate"], "float32")
    np.testing.assert_allclose(losses[0], float(golden["block.loss"]), rtol=1e-5)


def test_example_trains_on_the_composed_route():
    """examples/transformer_run.py, shortened, on the twin (everything composed): the mean loss falls from epoch to epoch."""
    example = ns.load_example()
    history = example.main(example.parse(["--num_ep", "2", "--n_train", "256", "--n_test", "64", "--composed"]))
    assert len(history) == 2 and history[1][0] < history[0][0]
