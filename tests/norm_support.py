"""TEST INFRASTRUCTURE shared by tests/test_norm_host.py (CPU twin) and tests/test_gpu_norm.py (MI355X): the raw calls of one
route as numpy arrays, and the fixture's TransformerBlock case as a Model."""

import os

import numpy as np

import norm_oracle as no
import tinynn_autograd_amd as tn
from tinynn_autograd_amd import device_array as da
from tinynn_autograd_amd.core.layers import BLOCK_PARAM_ORDER, TransformerBlock
from tinynn_autograd_amd.core.losses import SquaredErrorLoss
from tinynn_autograd_amd.core.model import Model
from tinynn_autograd_amd.core.nn import Net
from tinynn_autograd_amd.core.optimizer import Adam
from tinynn_autograd_amd.core.tensor import Tensor

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "norm_cases.npz")
NEED_ALL = (True, True, True)


def load_example():
    """tinynn-autograd_amd/examples/transformer_run.py as a module (its main(parse([...])) returns the per-epoch history)."""
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tinynn-autograd_amd", "examples",
                        "transformer_run.py")
    spec = importlib.util.spec_from_file_location("transformer_run_example", path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def load_golden():
    with np.load(GOLDEN) as data:
        return dict(data)


def dev(a, dtype, unaligned=False):
    """The array on the device in `dtype` (None stays None); unaligned: at an address that is only element-aligned."""
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=dtype)
    if not unaligned:
        return tn.asarray(a, dtype=dtype)
    buf = tn.empty((a.size + 1,), dtype)
    view = buf[1:].reshape(a.shape)
    view[...] = tn.asarray(a, dtype=dtype)
    return view


def run(route, x, gamma, beta, dy, kind, eps, dtype, unaligned=False, need=NEED_ALL):
    """Forward and backward raw calls of one route -> {field: numpy array or None}; need = (dx, dgamma, dbeta)."""
    xd, gd, bd, dyd = (dev(a, dtype, unaligned) for a in (x, gamma, beta, dy))
    if kind == "layer":
        y, mean, rstd = da.layer_norm(xd, gd, bd, eps=eps, route=route)
    else:
        (y, rstd), mean = da.rms_norm(xd, gd, eps=eps, route=route), None
    dx, dgamma, dbeta = da.norm_bwd(xd, dyd, gd, mean, rstd, kind=kind, route=route, need_dx=need[0], need_dgamma=need[1],
                                    need_dbeta=need[2])
    out = dict(y=y, mean=mean, rstd=rstd, dx=dx, dgamma=dgamma, dbeta=dbeta)
    return {n: None if a is None else np.asarray(a) for n, a in out.items()}


def golden_result(golden, name, dtype):
    """(inputs, oracle result for `dtype` with the FIXTURE's values in place of the recomputed ones)."""
    inputs = no.case_input(name, dtype)
    res = no.reference(*inputs[:4], kind=inputs[4], eps=inputs[5], dtype=dtype)
    for field, want in no.unpack(golden[name], no.case_fields(name)).items():
        res.values[field] = want.reshape(np.shape(res.values[field]))
    return inputs, res


def block_model(golden, fused, dtype):
    """The fixture's block case as (model, x, y): parameters replaced by the fixture's through Net.set_parameters."""
    c = no.BLOCK_CASE
    assert tuple(no.BLOCK_NAMES) == tuple(BLOCK_PARAM_ORDER)
    block = TransformerBlock(c["H"], hidden=c["hidden"], num_in=c["E"], causal=c["causal"], eps=c["eps"], fused=fused)
    net = Net([block])
    values = no.unpack(golden["block.params"].astype(np.float64), no.block_layout())
    net.set_parameters([{name: Tensor(values[name].astype(dtype), requires_grad=True, dtype=dtype) for name in BLOCK_PARAM_ORDER}])
    model = Model(net=net, loss=SquaredErrorLoss(), optimizer=Adam(lr=c["lr"]))
    x, y = no.block_data(dtype)
    return model, Tensor(x, dtype=dtype), Tensor(y, dtype=dtype)


def block_step(model, x, y, read_grads=True):
    """One training step -> (loss as a device array, {name: gradient as float64 numpy} read BEFORE the update; None with
    read_grads=False, which keeps the step free of host reads — what a graph capture needs)."""
    model.zero_grad()
    loss = SquaredErrorLoss().loss(model.forward(x), y)
    loss.backward()
    grads = None
    if read_grads:
        grads = {name: np.asarray(model.net.layers[0].params[name].grad, dtype=np.float64) for name in BLOCK_PARAM_ORDER}
    model.step()
    return loss.values, grads


def block_run(golden, fused, dtype, steps):
    """(losses of `steps` Adam steps, gradients of the first)."""
    model, x, y = block_model(golden, fused, dtype)
    losses, first = [], None
    for _ in range(steps):
        loss, grads = block_step(model, x, y)
        losses.append(float(loss))
        first = first or grads
    return np.array(losses), first


def assert_block_grads(grads, golden, rel, what):
    """max|got - ref| <= rel[i] * scale[i] per tensor (scale: max|ref|; for attn.bk, whose gradient is mathematically zero,
    the sum of |terms| — tests/gen_norm_golden.py)."""
    ref = no.unpack(golden["block.grads"], no.block_layout())
    rel = np.broadcast_to(rel, (len(no.BLOCK_NAMES),))
    for name, scale, r in zip(no.BLOCK_NAMES, golden["block.grad_scale"], rel):
        worst = np.abs(grads[name].reshape(ref[name].shape) - ref[name]).max()
        assert worst <= r * scale, "%s %s: max|diff| %.3e > %.3e" % (what, name, worst, r * scale)
