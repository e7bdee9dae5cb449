"""Shared by the convolution tests: the LeNet of the example on the device backend and the comparison with the float64
trajectory of tests/golden/conv_cases.npz."""

import os

import numpy as np

import conv_oracle as co

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_cases.npz")
LENET_SEED = 11


def load_golden():
    with np.load(GOLDEN) as data:
        return dict(data)


def build_lenet(seed=LENET_SEED, fused=True):
    """Layers drawn in order under np.random.seed(seed); every shape explicit so that nothing waits for the first batch."""
    from tinynn_autograd_amd.core.layers import Conv2D, Dense, Flatten, MaxPool2D, ReLU
    from tinynn_autograd_amd.core.nn import Net
    np.random.seed(seed)
    return Net([Conv2D((5, 5, 1, 6), padding=2, fused=fused), ReLU(), MaxPool2D(2),
                Conv2D((5, 5, 6, 16), fused=fused), ReLU(), MaxPool2D(2), Flatten(),
                Dense(120, num_in=400, fused=fused), ReLU(), Dense(84, num_in=120, fused=fused), ReLU(),
                Dense(10, num_in=84, fused=fused)])


def build_lenet_model(seed=LENET_SEED, fused=True, lr=1e-3):
    from tinynn_autograd_amd.core.losses import SoftmaxCrossEntropyLoss
    from tinynn_autograd_amd.core.model import Model
    from tinynn_autograd_amd.core.optimizer import Adam
    net = build_lenet(seed, fused)
    loss = SoftmaxCrossEntropyLoss(fused=fused)
    return Model(net=net, loss=loss, optimizer=Adam(lr=lr, fused=fused)), loss


def train_step(model, loss_layer, x, y):
    from tinynn_autograd_amd.core.tensor import Tensor
    x, y = (a if isinstance(a, Tensor) else Tensor(a) for a in (x, y))     # (a captured step passes fixed-address Tensors)
    model.zero_grad()
    loss = loss_layer.loss(model.forward(x), y)
    loss.backward()
    model.step()
    return loss


def run_trajectory(model, loss_layer):
    """Five Adam steps on the fixture's batches -> (losses, final parameters as float64 numpy)."""
    losses = [float(train_step(model, loss_layer, x, y).values) for x, y in co.lenet_batches()]
    return np.array(losses), [np.asarray(p.values, dtype=np.float64) for p in model.net.parameter_tensors()]


def trajectory_deviation(losses, params, golden):
    """Largest deviation from the float64 fixture: (relative on the losses, absolute on the final parameters)."""
    ref = golden["lenet.losses"]
    dl = float(np.max(np.abs(losses - ref) / np.abs(ref)))
    dp = 0.0
    for i, p in enumerate(params):
        if "lenet.final%d" % i in golden:
            dp = max(dp, float(np.abs(p - golden["lenet.final%d" % i]).max()))
        else:
            at = golden["lenet.final%d_idx" % i]
            dp = max(dp, float(np.abs(p.ravel()[at] - golden["lenet.final%d_sample" % i]).max()))
    return dl, dp
