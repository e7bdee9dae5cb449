"""TEST INFRASTRUCTURE — the convolution / pooling fixture tests/golden/conv_cases.npz.

    python tests/gen_conv_golden.py

The reference has no convolution, so the fixture's numbers come from the float64 numpy oracle tests/conv_oracle.py; when
torch is importable (the build container) every number is additionally asserted against float64 CPU torch, so the fixture
has two independent parents.  Operands are rebuilt by conv_oracle.conv_case_input / pool_case_input from the case's seed
(numpy's legacy RandomState stream is frozen); the file holds results only: y, dx, dw, db per convolution case, y, idx, dx
per pooling case, and the float64 LeNet trajectory (five Adam steps on conv_oracle.lenet_batches from the package's own
initial draw under np.random.seed(LENET_SEED)): losses and final parameters (whole, or 512 sampled entries of the large
ones)."""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import conv_oracle as co          # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "conv_cases.npz")
LENET_SEED = 11
SAMPLE = 512


def lenet_initial():
    """The package's own initial parameters of the LeNet (host RNG only; the CPU test twin holds the arrays)."""
    import conftest
    from tinynn_autograd_amd import _lib
    if not _lib.is_loaded():
        _lib.install_test_twin(conftest.build_twin())
    from lenet_helpers import build_lenet
    net = build_lenet(LENET_SEED)
    return [np.asarray(p.values, dtype=np.float64) for p in net.parameter_tensors()]


def main():
    try:
        import torch
        import torch.nn.functional as fn
    except ImportError:
        torch = None
    out = {}
    for name, (xs, ws, stride, padding) in co.CONV_CASES.items():
        x, w, b, dy = co.conv_case_input(name)
        y = co.conv2d(x, w, b, stride, padding)
        dx = co.conv2d_dx(dy, w, xs, stride, padding)
        dw = co.conv2d_dw(x, dy, ws, stride, padding)
        db = co.conv2d_db(dy)
        if torch is not None:
            t = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (x, w, b)]
            ty = fn.conv2d(t[0], t[1], t[2], stride=stride, padding=padding)
            ty.backward(torch.tensor(dy, dtype=torch.float64))
            for got, want in ((y, ty.detach()), (dx, t[0].grad), (dw, t[1].grad), (db, t[2].grad)):
                np.testing.assert_allclose(got, want.numpy(), rtol=1e-12, atol=1e-12, err_msg=name)
        out.update({name + ".y": y, name + ".dx": dx, name + ".dw": dw, name + ".db": db})
    for name, (xs, kernel, stride, padding) in co.POOL_CASES.items():
        x, dy = co.pool_case_input(name)
        y, idx = co.max_pool2d(x, kernel, stride, padding)
        dx = co.max_pool2d_dx(dy, idx, xs)
        if torch is not None:
            tx = torch.tensor(x, dtype=torch.float64, requires_grad=True)
            ty, ti = fn.max_pool2d(tx, kernel, stride, padding, return_indices=True)
            ty.backward(torch.tensor(dy, dtype=torch.float64))
            assert np.array_equal(y, ty.detach().numpy()) and np.array_equal(idx, ti.numpy()), name
            np.testing.assert_allclose(dx, tx.grad.numpy(), rtol=1e-12, atol=1e-12, err_msg=name)
        out.update({name + ".y": y, name + ".idx": idx.astype(np.int32), name + ".dx": dx})
    model = co.LeNet64(lenet_initial())
    losses = [model.step(x, y)[0] for x, y in co.lenet_batches()]
    out["lenet.losses"] = np.array(losses)
    rs = np.random.RandomState(LENET_SEED)
    for i, p in enumerate(model.p):
        if p.size <= 4 * SAMPLE:
            out["lenet.final%d" % i] = p
        else:
            at = np.sort(rs.choice(p.size, SAMPLE, replace=False))
            out["lenet.final%d_idx" % i] = at.astype(np.int32)
            out["lenet.final%d_sample" % i] = p.ravel()[at]
    np.savez_compressed(GOLDEN, **out)
    print("wrote %s: %d arrays, %d bytes%s" % (GOLDEN, len(out), os.path.getsize(GOLDEN),
                                               "" if torch is not None else " (torch absent: not cross-checked)"))


if __name__ == "__main__":
    main()
