"""TEST INFRASTRUCTURE shared by tests/test_ostep_host.py (CPU twin) and tests/test_gpu_ostep.py (MI355X): tiny nets, gradients
written into the parameters' gradient buffers, and the float64 oracle (tests/ostep_oracle.py) run next to a model."""

import numpy as np

import ostep_oracle as oo
import tinynn_autograd_amd as tn
from tinynn_autograd_amd.core.layers import Dense, ReLU, TransformerBlock
from tinynn_autograd_amd.core.losses import SoftmaxCrossEntropyLoss
from tinynn_autograd_amd.core.model import Model
from tinynn_autograd_amd.core.nn import Net
from tinynn_autograd_amd.core.tensor import Tensor

RTOL = 1e-5          # the project's float32 bound (tests/parity_suite.py), of each tensor's max-norm
F64_TOL = 1e-12      # float64: a few 2^-53 per operation and step, of each tensor's max-norm

# the parameters of a TransformerBlock that the default rule does NOT decay: last name component starts with "b", or is
# "gamma" / "beta" (written out here, not derived with the rule under test)
BLOCK_NO_DECAY = ("ln1.gamma", "ln1.beta", "attn.bq", "attn.bk", "attn.bv", "attn.bo", "ln2.gamma", "ln2.beta", "fc1.b", "fc2.b")


def tol(dtype):
    return F64_TOL if np.dtype(dtype) == np.float64 else RTOL


def dense_net(seed=3):
    np.random.seed(seed)
    return Net([Dense(6, num_in=5), ReLU(), Dense(3, num_in=6)]), (4, 5)


def block_net(seed=4):
    """One TransformerBlock at width 8, sequence 4, batch 2."""
    np.random.seed(seed)
    return Net([TransformerBlock(2, num_in=8)]), (2, 4, 8)


def make_model(kind, optimizer, dtype, use_arena=True):
    tn.set_default_float(dtype)
    net, xshape = (dense_net if kind == "dense" else block_net)()
    model = Model(net=net, loss=SoftmaxCrossEntropyLoss(), optimizer=optimizer, use_arena=use_arena)
    for p in model._live_params():                   # (fresh weights are float32 whatever the default float is)
        p.values = tn.asarray(np.asarray(p.values).astype(dtype), dtype=dtype)
        assert p.values.dtype == np.dtype(dtype)
    return model, xshape


def names_and_decay(model):
    """[(name, decayed)] per live parameter, by an explicit list of names."""
    out = []
    for layer in model.net.get_parameters():
        for name in layer:
            out.append((name, name not in BLOCK_NO_DECAY and name not in ("b", "gamma", "beta")))
    return out


def host_params(model):
    return [np.asarray(p.values).astype(np.float64) for p in model._live_params()]


def param_bits(model):
    return [np.asarray(p.values).copy().tobytes() for p in model._live_params()]


def draw_grads(model, rs, dtype):
    """One gradient per parameter with |g| >= 0.1 (oo.gradients says why), already rounded to `dtype`."""
    return [oo.gradients(rs, tuple(p.shape)).astype(dtype) for p in model._live_params()]


def backward_then_inject(model, xshape, grads, dtype, rs, real_backward=True):
    """A real forward / backward (so that the model's own gradient plumbing has run), then the gradients are OVERWRITTEN in
    place with the drawn ones: the optimizer sees exactly what the oracle sees."""
    model.zero_grad()
    if real_backward:
        out = model.forward(Tensor(rs.standard_normal(xshape).astype(dtype)))
        if len(out.shape) == 2:            # the Dense net: through the loss, as a training loop does
            labels = np.eye(out.shape[1])[rs.randint(0, out.shape[1], out.shape[0])].astype(dtype)
            model.loss.loss(out, Tensor(labels)).backward()
        else:
            out.backward(np.ones(out.shape, dtype=dtype))
    for p, g in zip(model._live_params(), grads):
        p.grad[...] = tn.asarray(g, dtype=dtype)


def assert_params(model, want, dtype, what):
    for i, (p, w) in enumerate(zip(model._live_params(), want)):
        np.testing.assert_allclose(np.asarray(p.values).astype(np.float64), w, rtol=0, atol=tol(dtype) * np.abs(w).max(),
                                   err_msg="%s, parameter %d" % (what, i))


ORACLE_SCHEDULE = ("cosine", 2, 4, 1e-3)


def hyper_kwargs():
    """(AdamW keyword arguments, the oracle's) of the shared test configuration: clipping, decay and a schedule all active."""
    from tinynn_autograd_amd import ostep
    opt = dict(lr=1e-2, weight_decay=0.1, max_norm=1.0, schedule=ostep.Cosine(2, 4, 1e-3))
    orc = dict(lr=1e-2, wd=0.1, max_norm=1.0, schedule=ORACLE_SCHEDULE)
    return opt, orc
