"""The fused linear + cross-entropy on the host side: lce.py's planner and refusals, the composed route against the float64
reference of tests/lce_oracle.py, and LinearCrossEntropyLoss against Dense + CrossEntropyLoss on the example model."""

import numpy as np
import pytest

import lce_oracle as lo
import token_support as ts
from tinynn_autograd_amd import device_array as da, lce
from tinynn_autograd_amd.core import ops
from tinynn_autograd_amd.core.losses import CrossEntropyLoss, LinearCrossEntropyLoss
from tinynn_autograd_amd.core.tensor import Tensor


def test_planner_forms_splits_chunks_and_sizes():
    """Forms and routes; split runs that cover every vocabulary block once; chunk rounding; 64-bit sizes at M V = 2^32."""
    p = lce.plan_linear_cross_entropy((2, 33, 20), (20, 516), (1, 516), (2, 33), ignore_index=-1, reduction="sum")
    assert (p.M, p.K, p.V, p.bias, p.rows_shape, p.row_blocks, p.vocab_blocks, p.route) == (66, 20, 516, True, (2, 33), 2, 3, "native")
    assert p.splits == 3 and p.chunk_rows == 128 and p.chunks() == [(0, 66)] and p.workspace_bytes() == 7 * 66 * 4 + 8
    assert lce.plan_linear_cross_entropy((5, 4), (4, 12), None, (5,)).workspace_bytes() == 0           # one block: one split
    for kw in (dict(native=False), dict(float_ok=False)):
        assert lce.plan_linear_cross_entropy((5, 4), (4, 12), None, (5,), **kw).route == "composed"
        with pytest.raises(ValueError, match="native linear \\+ cross-entropy route needs"):
            lce.plan_linear_cross_entropy((5, 4), (4, 12), None, (5,), route="native", **kw)
    for m, v in ((1, 1), (64, 516), (65, 70000), (8192, 32768), (100000, 257)):
        most = lce.most_splits(v)
        assert most == min(lce.vocab_blocks(v), lce.MAX_SPLITS) and 1 <= lce.choose_splits(m, v) <= most
        assert lce.choose_splits(m, v) == most or lce.choose_splits(m, v) * lce.row_blocks(m) >= 2 * lce.CUS
        for splits in {1, lce.choose_splits(m, v), most}:
            runs = [lce.split_range(v, splits, s) for s in range(splits)]
            assert runs[0][0] == 0 and runs[-1][1] == lce.vocab_blocks(v)
            assert all(a[0] < a[1] for a in runs) and all(a[1] == b[0] for a, b in zip(runs, runs[1:]))
    assert [lce.choose_chunk_rows(m, v) for m, v in ((8192, 32768), (8192, 1 << 21), (65, 12), (1, 1))] == [2048, 64, 128, 64]
    assert lce.plan_linear_cross_entropy((65, 4), (4, 12), None, (65,), chunk_rows=64).chunks() == [(0, 64), (64, 1)]
    big = lce.plan_linear_cross_entropy((8192, 512), (512, 524288), (524288,), (8192,))
    assert big.logits_elements() == 1 << 32 and big.chunk_rows == 128 and big.chunk_elements() == 1 << 26
    assert lce.expect_slower(8192, 1024, 32768) and not lce.expect_slower(8192, 8192, 32768)
    assert (big.splits, big.workspace_bytes(), len(big.chunks()), big.chunks()[-1]) == (4, 9 * 8192 * 4, 64, (8064, 128))


def test_refusals():
    plan = lce.plan_linear_cross_entropy
    for args, match in ((((5, 4), (3, 12), None, (5,)), r"h must be \[.., K\]"), (((5, 4), (4, 12), (11,), (5,)), "b must hold V = 12"),
                        (((5, 4), (4, 12), None, (4,)), "targets must have shape")):
        with pytest.raises(ValueError, match=match):
            plan(*args)
    for kw, match in ((dict(reduction="max"), "reduction must be one of"), (dict(splits=2), r"splits 2 outside \[1, 1\]"),
                      (dict(chunk_rows=65), "multiple of 64"), (dict(route="fast"), "route must be one of")):
        with pytest.raises(ValueError, match=match):
            plan((5, 4), (4, 12), None, (5,), **kw)
    h, w = Tensor(np.zeros((5, 4)), dtype=np.float64), Tensor(np.zeros((4, 12)), dtype=np.float64)
    with pytest.raises(ValueError, match="float32 operands"):          # float64 is the composed route's
        ops.linear_cross_entropy_(h, w, None, np.zeros(5, dtype=np.int64), route="native")
    with pytest.raises(TypeError, match="label_smoothing"):
        ops.linear_cross_entropy_(h, w, None, np.zeros(5, dtype=np.int64), label_smoothing=0.1)


@pytest.mark.parametrize("m, k, v, bias, reduction", [(1, 1, 1, True, "mean"), (17, 6, 12, False, "sum"), (65, 20, 516, True, "mean")])
def test_composed_route_against_float64(m, k, v, bias, reduction):
    rs = np.random.RandomState(m + k + v)
    h, w, b = lo.inputs(rs, m, k, v, bias)
    t = rs.randint(0, v, m)
    t[m // 2] = -7                                                    # ignored (one row: everything is)
    ref = lo.reference(h, w, b, t, ignore_index=-7, reduction=reduction, g=1.0)
    lo.check(ref.values, ref, "the reference alone")                  # the inputs meet the median gate
    th, tw = Tensor(h, requires_grad=True), Tensor(w, requires_grad=True)
    tb = Tensor(b, requires_grad=True) if bias else None
    loss = ops.linear_cross_entropy_(th, tw, tb, t, ignore_index=-7, reduction=reduction, route="composed")
    loss.backward()
    got = dict(loss=np.asarray(loss.values), dh=np.asarray(th.grad), dw=np.asarray(tw.grad), db=np.asarray(tb.grad) if bias else None)
    lo.check(got, ref, "composed M %d K %d V %d" % (m, k, v), verbose=True)


def test_loss_layer_equals_dense_and_cross_entropy_on_the_example(monkeypatch):
    """On the composed route the loss layer IS the head's forward and cross_entropy_, bit for bit (native: test_gpu_lce.py)."""
    monkeypatch.setattr(da, "LCE_ROUTE", "composed")
    ex = ts.load_example()
    argv = ["--width", "32", "--heads", "2", "--seq", "8", "--vocab", "11"]
    rs = np.random.RandomState(2)
    ids, targets = ex.make_data(rs, 4, 8, 11, 4)
    results = []
    for fused_head in (False, True):
        np.random.seed(7)
        model, loss_layer = ex.build(ex.parse(argv + (["--fused-head"] if fused_head else [])))
        assert type(loss_layer) is (LinearCrossEntropyLoss if fused_head else CrossEntropyLoss)
        loss = loss_layer.loss(model.forward(Tensor(ids), hidden=fused_head), targets.reshape(-1))
        loss.backward()
        head = model.net.layers[-1].params
        results.append([np.asarray(a, dtype=np.float64) for a in (loss.values, head["w"].grad, head["b"].grad,
                                                                  model.net.layers[0].params["tok"].grad)])
    for plain, fused in zip(*results):
        assert np.array_equal(plain, fused)
    with pytest.raises(ValueError, match="last layer must be a Dense"):
        ex.build(ex.parse(argv))[0].net.__class__(model.net.layers[:-1]).forward(Tensor(ids), hidden=True)
