"""AdamW and Model.clip_grad_norm through the public interface on the CPU twin, i.e. on the COMPOSED route (the same maths on
DeviceArray arithmetic, the norm read back), against the float64 oracle of tests/ostep_oracle.py.

Gradients are drawn with |g| >= 0.1: Adam's first steps are m / sqrt(v) ~ sign(g), so for a gradient near zero the update's
sign would hinge on the last bit of g and no tolerance on the parameters could hold — the reason ADAM_GATE exists in the
parity suite.  Bounds: float64 within 1e-12 of each tensor's max-norm (a few 2^-53 per operation over 4 steps), float32 within
the project's RTOL = 1e-5 of it."""

import numpy as np
import pytest

import ostep_oracle as oo
import ostep_support as su
import tinynn_autograd_amd as tn
from tinynn_autograd_amd import _lib, ostep
from tinynn_autograd_amd.core.layers import BLOCK_PARAM_ORDER, Dense, ReLU
from tinynn_autograd_amd.core.losses import SoftmaxCrossEntropyLoss
from tinynn_autograd_amd.core.model import Model
from tinynn_autograd_amd.core.nn import Net
from tinynn_autograd_amd.core.optimizer import Adam, AdamW, BaseOptimizer, default_no_decay
from tinynn_autograd_amd.core.tensor import Tensor

STEPS = 4


def run_against_oracle(kind, dtype, use_arena=True, fused=True):
    opt_kw, orc_kw = su.hyper_kwargs()
    opt = AdamW(fused=fused, **opt_kw)
    model, xshape = su.make_model(kind, opt, dtype, use_arena=use_arena)
    decay = [d for _n, d in su.names_and_decay(model)]
    want, state = su.host_params(model), None
    state = oo.new_state(want)
    rs = np.random.RandomState(11)
    for s in range(STEPS):
        grads = su.draw_grads(model, rs, dtype)
        su.backward_then_inject(model, xshape, grads, dtype, rs)
        model.step()
        want = oo.adamw_step(want, grads, state, decay, **orc_kw)
        su.assert_params(model, want, dtype, "%s %s step %d" % (kind, np.dtype(dtype).name, s + 1))
        st = opt.state()
        assert st["t"] == s + 1 and st["skipped"] == 0 and st["skip"] == 0
        np.testing.assert_allclose(st["lr"], state["lr"], rtol=1e-15)
        np.testing.assert_allclose(st["gnorm"], state["gnorm"], rtol=1e-12)
        np.testing.assert_allclose(st["coef"], state["coef"], rtol=1e-12)
        assert st["coef"] < 1.0                                    # the configuration really clips
    return model, opt


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kind", ["dense", "block"])
def test_adamw_through_model_step_against_the_oracle(kind, dtype):
    model, opt = run_against_oracle(kind, dtype)
    if tn.backend_name() != "hip-gfx950":
        assert opt.route == "composed"
    assert model._grad_arena is not None and model._pending_first is None
    assert opt.last_norm() == opt.state()["gnorm"] and opt.lr_now() == opt.state()["lr"]


def test_the_optimizer_cannot_absorb_the_first_layer():
    """Model would otherwise defer the first Dense layer's backward into a launch that cannot see the global norm."""
    assert issubclass(AdamW, BaseOptimizer) and not issubclass(AdamW, Adam)
    assert not hasattr(AdamW, "apply_with_first_layer") and not hasattr(AdamW, "take_tick")
    with pytest.raises(TypeError, match="schedule"):
        AdamW(schedule="cosine")
    with pytest.raises(ValueError, match="max_norm"):
        AdamW(max_norm=-1.0)


def test_default_no_decay_on_a_block():
    """Exactly the `b*`, `gamma` and `beta` entries of BLOCK_PARAM_ORDER are left undecayed: the four attention biases, the two
    MLP biases and the gains and offsets of the two norms — ten of the sixteen."""
    marked = tuple(n for n in BLOCK_PARAM_ORDER if default_no_decay(0, None, n))
    assert marked == su.BLOCK_NO_DECAY and len(marked) == 10
    assert [n for n in BLOCK_PARAM_ORDER if n not in marked] == ["attn.wq", "attn.wk", "attn.wv", "attn.wo", "fc1.w", "fc2.w"]
    assert default_no_decay(0, None, "b") and default_no_decay(3, None, "gamma") and not default_no_decay(0, None, "w")
    assert not default_no_decay(0, None, "tok") and not default_no_decay(0, None, "pos")
    opt = AdamW()
    model, xshape = su.make_model("block", opt, np.float32)
    rs = np.random.RandomState(0)
    su.backward_then_inject(model, xshape, su.draw_grads(model, rs, np.float32), np.float32, rs, real_backward=False)
    model.step()
    sizes = [int(np.prod(model.net.layers[0].params[n].shape)) for n in BLOCK_PARAM_ORDER]
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    starts, flags = ostep.decay_runs(list(zip(offsets, sizes)), [n not in su.BLOCK_NO_DECAY for n in BLOCK_PARAM_ORDER])
    got = opt.decay_runs()
    assert list(got[0]) == list(starts) and list(got[1]) == list(flags)
    assert len(starts) < len(BLOCK_PARAM_ORDER)                    # neighbours merged: ln1.gamma + ln1.beta, bo + ln2.* ...
    # a predicate of the user's own sees (layer_index, layer, name)
    seen = []
    opt2 = AdamW(no_decay=lambda i, layer, name: seen.append((i, type(layer).__name__, name)) or True)
    model2, _ = su.make_model("block", opt2, np.float32)
    su.backward_then_inject(model2, xshape, su.draw_grads(model2, rs, np.float32), np.float32, rs, real_backward=False)
    model2.step()
    assert seen == [(0, "TransformerBlock", n) for n in BLOCK_PARAM_ORDER]
    assert list(opt2.decay_runs()[1]) == [0]


@pytest.mark.parametrize("kind", ["dense", "block"])
def test_compute_step_route_equals_the_arena_route(kind):
    dtype = np.float64
    arena, opt_a = run_against_oracle(kind, dtype, use_arena=True)
    plain, opt_p = run_against_oracle(kind, dtype, use_arena=False)
    assert arena._grad_arena is not None and plain._grad_arena is None
    su.assert_params(plain, su.host_params(arena), dtype, "compute_step vs arena")
    assert opt_a.state()["t"] == opt_p.state()["t"] == STEPS
    assert list(opt_a.decay_runs()[0]) == list(opt_p.decay_runs()[0]) and list(opt_a.decay_runs()[1]) == list(opt_p.decay_runs()[1])


@pytest.mark.parametrize("bad", [np.inf, np.nan])
def test_a_non_finite_gradient_skips_the_step(bad):
    opt_kw, orc_kw = su.hyper_kwargs()
    opt = AdamW(**opt_kw)
    model, xshape = su.make_model("dense", opt, np.float32)
    rs = np.random.RandomState(5)
    grads = su.draw_grads(model, rs, np.float32)
    su.backward_then_inject(model, xshape, grads, np.float32, rs)
    model.step()                                                   # one good step: the state arrays exist
    before, st0 = su.param_bits(model), opt.state()
    m0, v0 = np.asarray(opt._m).tobytes(), np.asarray(opt._v).tobytes()
    grads = su.draw_grads(model, rs, np.float32)
    grads[2][1, 2] = bad
    su.backward_then_inject(model, xshape, grads, np.float32, rs)
    model.step()
    st = opt.state()
    assert su.param_bits(model) == before
    assert np.asarray(opt._m).tobytes() == m0 and np.asarray(opt._v).tobytes() == v0
    assert st["skipped"] == 1 and st["skip"] == 1 and st["t"] == st0["t"] == 1
    assert st["b1_pow"] == st0["b1_pow"] and st["b2_pow"] == st0["b2_pow"]
    # ... and from a fresh optimizer: t stays 0, and the next finite step is the oracle's FIRST step
    opt = AdamW(**opt_kw)
    model, xshape = su.make_model("dense", opt, np.float32)
    want = su.host_params(model)
    before = su.param_bits(model)
    su.backward_then_inject(model, xshape, grads, np.float32, rs)
    model.step()
    assert su.param_bits(model) == before and opt.state()["t"] == 0 and opt.state()["skipped"] == 1
    assert opt.state()["b1_pow"] == 1.0 and opt.state()["b2_pow"] == 1.0
    good = su.draw_grads(model, rs, np.float32)
    su.backward_then_inject(model, xshape, good, np.float32, rs)
    model.step()
    state = oo.new_state(want)
    want = oo.adamw_step(want, good, state, [d for _n, d in su.names_and_decay(model)], **orc_kw)
    su.assert_params(model, want, np.float32, "the step after a skipped one")
    assert opt.state()["t"] == 1 and opt.state()["skipped"] == 1 and opt.state()["skip"] == 0


def test_the_composed_route_cannot_be_captured(monkeypatch):
    opt = AdamW(fused=False)
    p, g = tn.asarray(np.ones(5, np.float32)), tn.asarray(np.full(5, 0.5, np.float32))
    assert opt.apply_flat(p, g) and opt.route == "composed"
    monkeypatch.setattr(_lib, "capturing", True)
    with pytest.raises(RuntimeError, match="graph capture"):
        opt.apply_flat(p, g)
    monkeypatch.setattr(_lib, "capturing", False)
    assert opt.state()["t"] == 1


def mnist_like(optimizer, seed=7):
    np.random.seed(seed)
    net = Net([Dense(12, num_in=20), ReLU(), Dense(8, num_in=12), ReLU(), Dense(4, num_in=8)])
    return Model(net=net, loss=SoftmaxCrossEntropyLoss(), optimizer=optimizer)


def loss_backward(model, x, y):
    model.zero_grad()
    loss = model.loss.loss(model.forward(Tensor(x)), Tensor(y))
    loss.backward()
    return loss


def test_clip_grad_norm_in_front_of_plain_adam():
    """Model.clip_grad_norm settles the deferred first-layer backward (fused Adam on one device defers it into the optimizer's
    launch), clips the arena in place and returns the norm; Adam then steps on the clipped gradients.  A twin model whose
    gradients are read back gives the oracle its input.  float32: RTOL of each tensor's max-norm."""
    rs = np.random.RandomState(2)
    x = rs.standard_normal((16, 20)).astype(np.float32)
    y = np.eye(4)[rs.randint(0, 4, 16)].astype(np.float32)
    lr, max_norm = 1e-3, 0.05
    probe, model = mnist_like(Adam(lr=lr)), mnist_like(Adam(lr=lr))
    want, state = [np.asarray(p.values).astype(np.float64) for p in probe._live_params()], None
    state = oo.new_state(want)
    for s in range(2):
        for m in (probe, model):
            loss_backward(m, x, y)
        if s > 0:                                                  # (the arenas exist from the first step on)
            assert model._pending_first is not None               # the first layer's backward is deferred ...
        grads = [np.asarray(p.grad).astype(np.float64) for p in probe._live_params()]
        clipped, gnorm = oo.clip(grads, max_norm)
        assert gnorm > max_norm
        norm = model.clip_grad_norm(max_norm)
        assert model._pending_first is None                       # ... and settled by the clip
        np.testing.assert_allclose(float(norm), gnorm, rtol=1e-6)
        for p, c in zip(model._live_params(), clipped):
            np.testing.assert_allclose(np.asarray(p.grad), c, rtol=0, atol=su.RTOL * np.abs(c).max())
        model.step()
        probe.step()
        want = oo.adam_step(want, clipped, state, lr=lr)
        # the probe took the UNCLIPPED step: bring it back in line for the next round
        for p, q in zip(probe._live_params(), model._live_params()):
            p.values[...] = q.values
        probe.optimizer._m[...] = model.optimizer._m
        probe.optimizer._v[...] = model.optimizer._v
        for p, w in zip(model._live_params(), want):
            np.testing.assert_allclose(np.asarray(p.values), w, rtol=0, atol=su.RTOL * np.abs(w).max(), err_msg="step %d" % (s + 1))
    # a max_norm above the norm changes nothing, bit for bit
    loss_backward(model, x, y)
    model.clip_grad_norm(0.0)
    assert all(not np.asarray(p.grad).any() for p in model._live_params())
    loss_backward(model, x, y)
    before = [np.asarray(p.grad).tobytes() for p in model._live_params()]
    loss_backward(model, x, y)
    model.clip_grad_norm(1e6)
    assert [np.asarray(p.grad).tobytes() for p in model._live_params()] == before


def test_the_charlm_example_trains_with_adamw(capsys):
    """examples/charlm_run.py --adamw, shortened, on the twin: decay, clipping and warm-up + cosine through the ordinary training
    loop; the loss falls, every step was applied and the schedule has run out at the last one.  Without --adamw the example
    builds the optimizer it always built."""
    import token_support as ts
    example = ts.load_example()
    args = example.parse(["--num_ep", "2", "--n_train", "256", "--n_test", "32", "--batch_size", "32", "--composed", "--adamw",
                          "--weight_decay", "0.05", "--clip", "0.5", "--warmup", "4"])
    history = example.main(args)
    assert len(history) == 2 and history[1][0] < history[0][0]
    assert "step 16, lr 0.000e+00" in capsys.readouterr().out                     # 2 epochs x 8 steps; cosine to the last step
    plain = example.make_optimizer(example.parse([]))
    assert type(plain) is Adam and plain.lr == 3e-3
    opt = example.make_optimizer(example.parse(["--adamw"]))
    assert type(opt) is AdamW and opt.max_norm == 1.0 and opt.weight_decay == 0.01 and opt.schedule.kind == ostep.SCHED_CONST
