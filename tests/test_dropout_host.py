"""Dropout through whichever library is loaded — on the CPU test twin that is the composed route of device_array.dropout /
ops.dropout_ — against the planner's mask bit for bit, the vjps, the generator's bookkeeping, the Dropout layer and the `dropout` arguments of TransformerBlock and Embedding —
including that the defaults leave outputs and gradients bit-identical to layers built without the argument."""

import numpy as np
import pytest

import dropout_support as dsu
import tinynn_autograd_amd as tn
from tinynn_autograd_amd import _lib, dropout as dp, rng
from tinynn_autograd_amd import device_array as da
from tinynn_autograd_amd.core import ops
from tinynn_autograd_amd.core.layers import Dropout, Embedding, TransformerBlock
from tinynn_autograd_amd.core.nn import Net
from tinynn_autograd_amd.core.tensor import Tensor


def test_numpy_global_rng_is_untouched():
    """Masks, uniform fills, the layers' draws and seeding come from rng.py alone: numpy's global generator — the shuffles and
    the parameter draws of a seeded run — is where it was."""
    np.random.seed(99)
    block = TransformerBlock(2, hidden=12, num_in=8, causal=True, dropout=0.2)
    emb = Embedding(9, 8, max_len=5, dropout=0.2)
    before = np.random.get_state()
    rng.manual_seed(1)
    g = rng.Generator(2)
    x = Tensor(dsu.values(80, np.float32).reshape(2, 5, 8), requires_grad=True)
    ops.dropout_(x, 0.5).backward(np.ones((2, 5, 8), np.float32))
    ops.dropout_(x, 0.5, x, generator=g)
    g.uniform((4, 4))
    Dropout(0.3).forward(x)
    block.forward(emb.forward(Tensor(np.zeros((2, 5), np.int64)))).backward(np.ones((2, 5, 8), np.float32))
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    assert rng.state()[1] == 5 and g.state() == (2, 2)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_composed_equals_the_planners_mask(dtype, p):
    for n, first in ((1, 0), (5, 3), (257, 1), (1025, 0)):
        g = rng.Generator(21).set_state(21, 4)
        x, res = dsu.values(n, dtype, n), dsu.values(n, dtype, n + 1)
        y, mask = da.dropout(tn.asarray(x, dtype=dtype), p, generator=g, first=first)
        assert y.dtype == dtype and (mask.keep is None) == _lib.get().has_dropout      # (the ticket instead, on the kernels)
        np.testing.assert_array_equal(np.asarray(y), dp.reference(x, 21, 4, p, first=first))
        assert g.state() == (21, 5)
        y, _ = da.dropout(tn.asarray(x, dtype=dtype), p, tn.asarray(res, dtype=dtype), generator=g, first=first)
        np.testing.assert_array_equal(dsu.bits(y), dsu.bits(dp.reference(x, 21, 5, p, residual=res, first=first)))
        assert g.state() == (21, 6)


def test_backward_uses_the_forwards_mask_and_the_residual_gets_dy():
    g = rng.Generator(3)
    x = Tensor(dsu.values(40, np.float32).reshape(5, 8), requires_grad=True)
    r = Tensor(dsu.values(40, np.float32, 1).reshape(5, 8), requires_grad=True)
    y = ops.dropout_(x, 0.5, r, generator=g)
    ops.dropout_(x, 0.5, generator=g)                            # a later draw must not change the first node's backward
    dy = dsu.values(40, np.float32, 2).reshape(5, 8)
    y.backward(dy)
    np.testing.assert_array_equal(np.asarray(x.grad), dp.reference(dy, 3, 0, 0.5))
    np.testing.assert_array_equal(dsu.bits(r.grad), dsu.bits(dy))
    assert g.state() == (3, 2)
    x.zero_grad()
    z = ops.dropout(x, 0.25, generator=g)                        # the public wrapper, plain form
    z.backward(dy)
    np.testing.assert_array_equal(np.asarray(z.values), dp.reference(np.asarray(x.values), 3, 2, 0.25))
    np.testing.assert_array_equal(np.asarray(x.grad), dp.reference(dy, 3, 2, 0.25))
    with pytest.raises(TypeError, match="unsupported arguments"):
        ops.dropout_(x, 0.5, training=True)
    with pytest.raises(ValueError, match="residual must have"):
        da.dropout(x.values, 0.5, tn.asarray(np.ones(8, np.float32)), generator=g)


def test_numerical_gradient_with_the_mask_held_fixed():
    tn.set_default_float(np.float64)
    x0, r0 = dsu.values(24, np.float64).reshape(4, 6), dsu.values(24, np.float64, 1).reshape(4, 6)
    w = dsu.values(24, np.float64, 2).reshape(4, 6)

    def loss(xv, rv):
        g = rng.Generator(8)                                     # the same ticket every time: the mask is held fixed
        y = ops.dropout_(Tensor(xv, dtype=np.float64), 0.3, Tensor(rv, dtype=np.float64), generator=g)
        return float(np.sum(np.asarray(y.values) * w))

    x, r = Tensor(x0, requires_grad=True, dtype=np.float64), Tensor(r0, requires_grad=True, dtype=np.float64)
    ops.dropout_(x, 0.3, r, generator=rng.Generator(8)).backward(w)
    eps = 1e-6
    for grad, which in ((np.asarray(x.grad), 0), (np.asarray(r.grad), 1)):
        num = np.zeros_like(x0)
        for i in np.ndindex(x0.shape):
            hi, lo = [x0.copy(), r0.copy()], [x0.copy(), r0.copy()]
            hi[which][i] += eps
            lo[which][i] -= eps
            num[i] = (loss(*hi) - loss(*lo)) / (2 * eps)
        # the loss is LINEAR in x and r: the central difference is exact up to the rounding of its two evaluations,
        # |loss| * 2^-52 / eps ~ 1e-8 here
        np.testing.assert_allclose(grad, num, rtol=0, atol=1e-7)


def test_generator_bookkeeping_and_seeding():
    g = rng.Generator(12)
    x = tn.asarray(dsu.values(64, np.float32))
    first = [np.asarray(da.dropout(x, 0.5, generator=g)[0]) for _ in range(3)]
    assert g.state() == (12, 3)
    assert not np.array_equal(first[0], first[1])
    g.manual_seed(12)
    assert g.state() == (12, 0)
    again = [np.asarray(da.dropout(x, 0.5, generator=g)[0]) for _ in range(3)]
    for a, b in zip(first, again):
        np.testing.assert_array_equal(a, b)
    h = rng.Generator(12)
    np.testing.assert_array_equal(np.asarray(h.uniform((7,))), dp.uniform(12, 0, 0, 7))
    np.testing.assert_array_equal(np.asarray(h.uniform((2, 3), np.float64, first=5)), dp.uniform(12, 1, 5, 6, np.float64).reshape(2, 3))
    assert h.state() == (12, 2)
    with pytest.raises(ValueError, match="float32 or float64"):
        h.uniform((2,), np.int64)
    # p == 0: nothing is drawn
    t = Tensor(np.asarray(x), requires_grad=True)
    assert ops.dropout_(t, 0.0, generator=h) is t and h.state() == (12, 2)
    # the module default
    rng.manual_seed(40)
    y = ops.dropout_(t, 0.5)
    np.testing.assert_array_equal(np.asarray(y.values), dp.reference(np.asarray(x), 40, 0, 0.5))
    assert rng.state() == (40, 1) and rng.default_generator.state() == (40, 1)
    np.testing.assert_array_equal(np.asarray(rng.uniform((3,))), dp.uniform(40, 1, 0, 3))


def test_composed_route_raises_inside_a_capture(monkeypatch):
    x = tn.asarray(dsu.values(8, np.float32))
    monkeypatch.setattr(_lib, "capturing", True)
    with pytest.raises(RuntimeError, match="cannot be captured"):
        da.dropout(x, 0.5, generator=rng.Generator(1), route="composed")


def test_dropout_layer_phases():
    x = Tensor(dsu.values(30, np.float32).reshape(5, 6), requires_grad=True)
    g = rng.Generator(2)
    layer = Dropout(0.5, generator=g)
    y = layer.forward(x)
    np.testing.assert_array_equal(np.asarray(y.values), dp.reference(np.asarray(x.values), 2, 0, 0.5))
    layer.set_phase("TEST")
    assert layer.forward(x) is x and g.state() == (2, 1)
    layer.set_phase("TRAIN")
    assert layer.forward(x) is not x and g.state() == (2, 2)
    off = Dropout(0.0, generator=g)
    assert off.forward(x) is x and g.state() == (2, 2)
    assert Dropout().p == 0.5
    for bad in (-0.5, 1.0, 2):
        with pytest.raises(ValueError, match="p must be"):
            Dropout(bad)
    net = Net([Dropout(0.5, generator=g)])
    net.set_phase("TEST")
    assert net.forward(x) is x
    net.set_phase("TRAIN")
    assert net.forward(x) is not x


def block_run(make, ids_or_x, dy):
    """(output, {name: gradient}) of one forward / backward of the layer `make()` builds from numpy seed 5."""
    np.random.seed(5)
    layer = make()
    x = Tensor(ids_or_x) if ids_or_x.dtype.kind == "i" else Tensor(ids_or_x, requires_grad=True)
    out = layer.forward(x)
    out.backward(dy)
    grads = {name: np.asarray(t.grad) for name, t in layer.params.items()}
    if x.requires_grad:
        grads["x"] = np.asarray(x.grad)
    return layer, np.asarray(out.values), grads


def test_block_and_embedding_defaults_are_bit_identical(monkeypatch):
    rs = np.random.RandomState(1)
    x, dy = rs.standard_normal((2, 5, 8)).astype(np.float32), rs.standard_normal((2, 5, 8)).astype(np.float32)
    seen = dsu.count_calls(monkeypatch)
    _, want, want_g = block_run(lambda: TransformerBlock(2, hidden=12, num_in=8, causal=True), x, dy)
    calls_without = list(seen)
    del seen[:]
    _, got, got_g = block_run(lambda: TransformerBlock(2, hidden=12, num_in=8, causal=True, dropout=0.0), x, dy)
    assert seen == calls_without                                  # the same launch sequence
    np.testing.assert_array_equal(dsu.bits(got), dsu.bits(want))
    assert sorted(got_g) == sorted(want_g)
    for name in want_g:
        np.testing.assert_array_equal(dsu.bits(got_g[name]), dsu.bits(want_g[name]))

    ids = rs.randint(0, 9, (2, 5))
    del seen[:]
    _, want, want_g = block_run(lambda: Embedding(9, 8, max_len=5), ids, dy)
    calls_without = list(seen)
    del seen[:]
    _, got, got_g = block_run(lambda: Embedding(9, 8, max_len=5, dropout=0.0), ids, dy)
    assert seen == calls_without
    np.testing.assert_array_equal(dsu.bits(got), dsu.bits(want))
    for name in want_g:
        np.testing.assert_array_equal(dsu.bits(got_g[name]), dsu.bits(want_g[name]))


def test_block_and_embedding_with_dropout():
    rs = np.random.RandomState(1)
    x, dy = rs.standard_normal((2, 5, 8)).astype(np.float32), rs.standard_normal((2, 5, 8)).astype(np.float32)
    _, plain, _ = block_run(lambda: TransformerBlock(2, hidden=12, num_in=8, causal=True), x, dy)
    g = rng.Generator(6)
    block, dropped, grads = block_run(lambda: TransformerBlock(2, hidden=12, num_in=8, causal=True, dropout=0.3, generator=g), x, dy)
    assert g.state() == (6, 2) and not np.array_equal(dropped, plain)                   # two draws per forward, none in backward
    assert all(np.isfinite(v).all() for v in grads.values())
    net = Net([block])
    net.set_phase("TEST")
    assert not block.is_training and not block.drop.is_training and not block.parts["attn"].is_training
    np.testing.assert_array_equal(dsu.bits(net.forward(Tensor(x)).values), dsu.bits(plain))
    assert g.state() == (6, 2)
    net.set_phase("TRAIN")
    g.manual_seed(6)
    np.testing.assert_array_equal(dsu.bits(net.forward(Tensor(x)).values), dsu.bits(dropped))      # a seed reproduces the run

    ids = rs.randint(0, 9, (2, 5))
    _, plain, _ = block_run(lambda: Embedding(9, 8, max_len=5), ids, dy)
    g = rng.Generator(7)
    emb, dropped, grads = block_run(lambda: Embedding(9, 8, max_len=5, dropout=0.5, generator=g), ids, dy)
    np.testing.assert_array_equal(dsu.bits(dropped), dsu.bits(dp.reference(plain, 7, 0, 0.5)))
    emb.set_phase("TEST")
    np.testing.assert_array_equal(dsu.bits(emb.forward(Tensor(ids)).values), dsu.bits(plain))
    assert g.state() == (7, 1)
    # the table's gradient is the embedding's vjp of the masked dy
    _, _, want = block_run(lambda: Embedding(9, 8, max_len=5), ids, dp.reference(dy, 7, 0, 0.5))
    for name in want:
        np.testing.assert_array_equal(dsu.bits(grads[name]), dsu.bits(want[name]))
    with pytest.raises(ValueError, match="p must be"):
        TransformerBlock(2, num_in=8, dropout=1.0)
    with pytest.raises(ValueError, match="p must be"):
        Embedding(9, 8, dropout=-0.1)


def test_generate_with_a_generator_equals_the_same_numbers_given():
    import decode_oracle as do
    import decode_support as ds
    from tinynn_autograd_amd import generation as gen
    net = ds.lm_net(ds.load_golden(), True, np.float32)
    prompt = do.lm_prompt()
    g = rng.Generator(31)
    a = gen.generate(net, prompt, do.LM_NEW, temperature=0.9, top_k=5, generator=g)
    u = dp.uniform(31, 0, 0, do.LM_NEW * prompt.shape[0], np.float32).reshape(do.LM_NEW, prompt.shape[0])
    assert np.array_equal(a, gen.generate(net, prompt, do.LM_NEW, temperature=0.9, top_k=5, u=u))
    assert g.state() == (31, 1)
    gen.generate(net, prompt, 2, temperature=0.0, generator=g)                                # greedy draws nothing
    assert g.state() == (31, 1)
    with pytest.raises(ValueError, match="excludes"):
        gen.generate(net, prompt, 2, seed=1, generator=g)
