"""TEST INFRASTRUCTURE shared by tests/test_token_host.py (CPU twin) and tests/test_gpu_token.py (MI355X): the raw calls of one
route as numpy arrays, and the fixture's language-model case as a Model."""

import os

import numpy as np

import token_oracle as to
import tinynn_autograd_amd as tn
from norm_support import dev
from tinynn_autograd_amd import device_array as da
from tinynn_autograd_amd.core.layers import BLOCK_PARAM_ORDER, Dense, Embedding, LayerNorm, TransformerBlock
from tinynn_autograd_amd.core.losses import CrossEntropyLoss
from tinynn_autograd_amd.core.model import Model
from tinynn_autograd_amd.core.nn import Net
from tinynn_autograd_amd.core.optimizer import Adam
from tinynn_autograd_amd.core.tensor import Tensor

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "token_cases.npz")


def load_example():
    """tinynn-autograd_amd/examples/charlm_run.py as a module (its main(parse([...])) returns the per-epoch history)."""
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tinynn-autograd_amd", "examples",
                        "charlm_run.py")
    spec = importlib.util.spec_from_file_location("charlm_run_example", path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def load_golden():
    with np.load(GOLDEN) as data:
        return dict(data)


def host(out):
    return {n: None if a is None else np.asarray(a) for n, a in out.items()}


def index(values, on_device):
    values = np.ascontiguousarray(values, dtype=np.int64)
    return tn.asarray(values) if on_device else values


def run_embed(route, table, ids, pos, dy, padding_idx, dtype, unaligned=False, need=(True, True), device_ids=False,
              poison=False):
    """Forward and backward raw calls of one route -> {out, dtable, dpos}; need = (dtable, dpos); poison: the gradients are
    written into buffers pre-filled with NaN."""
    td, pd, dyd = (dev(a, dtype, unaligned) for a in (table, pos, dy))
    idx = index(ids, device_ids)
    out = da.embedding(td, idx, pd, route=route)

    def dest(a):
        if not poison or a is None:
            return None
        d = dev(np.full(a.shape, np.nan), dtype, unaligned)
        return d
    t_out, p_out = dest(table if need[0] else None), dest(pos if need[1] else None)
    dtable, dpos = da.embedding_bwd(dyd, idx, table.shape, None if pos is None else pos.shape, padding_idx, need_dtable=need[0],
                                    need_dpos=need[1], dtable_out=t_out, dpos_out=p_out, route=route)
    if poison and route == "native":
        assert (dtable is None or dtable is t_out) and (dpos is None or dpos is p_out)
    return host(dict(out=out, dtable=dtable, dpos=dpos))


def run_xent(route, x, targets, ignore_index, reduction, g, dtype, unaligned=False, device_targets=False):
    xd = dev(x, dtype, unaligned)
    tg = index(targets, device_targets)
    loss, losses, lse, count = da.cross_entropy(xd, tg, ignore_index, reduction, route=route)
    dl = da.cross_entropy_bwd(xd, tg, lse, count, g, ignore_index, reduction, route=route)
    return host(dict(loss=loss, losses=losses, lse=lse, count=count, dlogits=dl))


def golden_embed(golden, name, dtype):
    """(inputs, oracle result for `dtype` with the FIXTURE's values in place of the recomputed ones)."""
    inputs = to.embed_case(name, dtype)
    res = to.embedding_reference(*inputs, dtype=dtype)
    for field, want in to.unpack(golden[name], to.embed_fields(name)).items():
        res.values[field] = want
    return inputs, res


def golden_xent(golden, name, dtype):
    inputs = to.xent_case(name, dtype)
    res = to.cross_entropy_reference(*inputs, dtype=dtype)
    for field, want in to.unpack(golden[name], to.xent_fields(name)).items():
        res.values[field] = want.reshape(np.shape(res.values[field]))
    return inputs, res


def lm_net(fused, dtype=np.float32):
    c = to.LM_CASE
    rows = load_example().Rows
    return Net([Embedding(c["V"], c["E"], max_len=c["max_len"], fused=fused),
                TransformerBlock(c["H"], hidden=c["hidden"], num_in=c["E"], causal=True, eps=c["eps"], fused=fused),
                LayerNorm(c["E"], eps=c["eps"], fused=fused), rows(), Dense(c["V"], num_in=c["E"], fused=fused)])


def lm_model(golden, fused, dtype):
    """The fixture's language model as (model, loss layer, ids, targets): parameters replaced through Net.set_parameters."""
    net = lm_net(fused, dtype)
    values = to.unpack(golden["lm.params"].astype(np.float64), to.lm_layout())
    tensor = lambda name: Tensor(values[name].astype(dtype), requires_grad=True, dtype=dtype)
    net.set_parameters([{"tok": tensor("emb.tok"), "pos": tensor("emb.pos")},
                        {name: tensor("block." + name) for name in BLOCK_PARAM_ORDER},
                        {"gamma": tensor("ln.gamma"), "beta": tensor("ln.beta")}, {},
                        {"w": tensor("head.w"), "b": tensor("head.b")}])
    loss_layer = CrossEntropyLoss(ignore_index=to.LM_IGNORE, fused=fused)
    model = Model(net=net, loss=loss_layer, optimizer=Adam(lr=to.LM_CASE["lr"]))
    return model, loss_layer, tn.asarray(golden["lm.ids"]), tn.asarray(golden["lm.targets"].reshape(-1))


def lm_grads(model):
    layers = model.net.layers
    named = [("emb.tok", layers[0], "tok"), ("emb.pos", layers[0], "pos")]
    named += [("block." + n, layers[1], n) for n in BLOCK_PARAM_ORDER]
    named += [("ln.gamma", layers[2], "gamma"), ("ln.beta", layers[2], "beta"), ("head.w", layers[4], "w"), ("head.b", layers[4], "b")]
    assert tuple(n for n, _, _ in named) == to.LM_NAMES
    return {name: np.asarray(layer.params[key].grad, dtype=np.float64) for name, layer, key in named}


def lm_step(model, loss_layer, ids, targets, read_grads=True):
    """One training step -> (loss as a device array, gradients read BEFORE the update, or None)."""
    model.zero_grad()
    loss = loss_layer.loss(model.forward(Tensor(ids)), targets)
    loss.backward()
    grads = lm_grads(model) if read_grads else None
    model.step()
    return loss.values, grads


def assert_lm_grads(grads, golden, rel, what):
    ref = to.unpack(golden["lm.grads"], to.lm_layout())
    rel = np.broadcast_to(rel, (len(to.LM_NAMES),))
    for name, scale, r in zip(to.LM_NAMES, golden["lm.grad_scale"], rel):
        worst = np.abs(grads[name].reshape(ref[name].shape) - ref[name]).max()
        assert worst <= r * scale, "%s %s: max|diff| %.3e > %.3e" % (what, name, worst, r * scale)


def assert_getitem_keeps_the_last(naive, ids, dy, want, bound):
    """The same lookup written as table[ids] (ops.getitem_): its vjp ASSIGNS, so of the gradients of a repeated id only the
    last survives — not the sum `want`."""
    from tinynn_autograd_amd.core import ops
    ops.getitem_(naive, ids).backward(dy)
    last = np.zeros(want.shape, dtype=dy.dtype)
    last[ids] = dy
    np.testing.assert_array_equal(np.asarray(naive.grad), last)
    assert not (np.abs(np.asarray(naive.grad) - want) <= bound).all()
