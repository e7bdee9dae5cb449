"""The token embedding, the per-row cross-entropy, their layers and the language-model example on the CPU test twin, where
everything takes the composed route: raw calls, ops and layers within the oracle's derived bounds, the scatter-ADD that
`table[ids]` lacks, parameter bookkeeping, ignored rows, host range checks, and the fixture's language model."""

import numpy as np
import pytest

import token_oracle as to
import token_support as ts
import tinynn_autograd_amd as tn
from tinynn_autograd_amd import _lib, device_array as da
from tinynn_autograd_amd.core import ops
from tinynn_autograd_amd.core.initializer import ConstantInit, NormalInit
from tinynn_autograd_amd.core.layers import EMBED_PARAM_ORDER, Embedding
from tinynn_autograd_amd.core.losses import CrossEntropyLoss
from tinynn_autograd_amd.core.nn import Net
from tinynn_autograd_amd.core.tensor import Tensor


@pytest.fixture(scope="module")
def golden():
    return ts.load_golden()


@pytest.fixture(autouse=True)
def _switches():
    yield
    da.TOKEN_ROUTE = None


def leaf(a, dtype=np.float32):
    if a is None:
        return None
    t = Tensor(np.asarray(a, dtype=dtype), requires_grad=True, dtype=dtype)
    t.zero_grad()
    return t


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", sorted(to.EMBED_CASES))
def test_embedding_composed_within_the_bounds(golden, name, dtype):
    tn.set_default_float(dtype)
    (table, ids, pos, dy, padding_idx), res = ts.golden_embed(golden, name, dtype)
    for device_ids in (False, True):
        got = ts.run_embed(None, table, ids, pos, dy, padding_idx, dtype, device_ids=device_ids)
        to.check(got, res, "%s %s composed" % (name, np.dtype(dtype).name), fields=to.EMBED_FIELDS)
        assert got["out"].dtype == dtype and got["out"].shape == ids.shape + (table.shape[1],)
    if pos is None:
        np.testing.assert_array_equal(got["out"], table[ids])                      # bit-exact
    for need in ((True, False), (False, True)):
        part = ts.run_embed("composed", table, ids, pos, dy, padding_idx, dtype, need=need)
        assert [part[f] is not None for f in ("dtable", "dpos")] == [need[0], need[1] and pos is not None]
        to.check(part, res, "%s %s" % (name, need), fields=to.EMBED_FIELDS)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", sorted(to.XENT_CASES))
def test_cross_entropy_composed_within_the_bounds(golden, name, dtype):
    tn.set_default_float(dtype)
    (x, t, ignore_index, reduction, g), res = ts.golden_xent(golden, name, dtype)
    for device_targets in (False, True):
        got = ts.run_xent(None, x, t, ignore_index, reduction, g, dtype, device_targets=device_targets)
        to.check(got, res, "%s %s composed" % (name, np.dtype(dtype).name), fields=to.XENT_FIELDS)
        assert got["loss"].shape == () and got["count"].shape == () and got["lse"].shape == t.shape
        assert got["dlogits"].dtype == dtype
    if res.values["count"] == 0:
        assert got["loss"] == 0.0 and not got["dlogits"].any()


def test_embedding_gradient_accumulates_where_getitem_keeps_the_last():
    """FAILS WITHOUT THE FEATURE.  ids [3, 1, 3, 3]: the gradient of ops.embedding_ w.r.t. the table is np.add.at's; the same
    net written as table[ids] gives the last-wins gradient — which is why the op exists."""
    table, ids, _, dy, _ = to.embed_case("embed_repeat")
    assert ids.tolist() == [3, 1, 3, 3]
    want = np.zeros(table.shape)
    np.add.at(want, ids, dy.astype(np.float64))
    res = to.embedding_reference(table, ids, None, dy)
    np.testing.assert_array_equal(res.values["dtable"], want)
    tt = leaf(table)
    out = ops.embedding_(tt, ids)
    np.testing.assert_array_equal(np.asarray(out.values), table[ids])
    out.backward(dy)
    to.assert_within(np.asarray(tt.grad), want, res.bounds["dtable"], "embedding_ dtable")
    naive = leaf(table)
    if tn.backend_name() != "hip-gfx950":
        # the CPU test twin has no scatter for a key that repeats an index: there `table[ids]` cannot be differentiated at
        # all; the last-wins gradient itself is pinned on the device (tests/test_gpu_token.py)
        with pytest.raises(_lib.TnnError, match="needs libtnn_hip.so"):
            ops.getitem_(naive, ids).backward(dy)
        return
    ts.assert_getitem_keeps_the_last(naive, ids, dy, want, res.bounds["dtable"])


def test_ops_vjps_in_every_optional_form():
    rs = np.random.RandomState(5)
    table, pos, dy = to.embed_inputs(rs, 6, 5, (3, 4), 7)
    ids = rs.randint(0, 6, (3, 4))
    for has_pos in (True, False):
        p = pos if has_pos else None
        res = to.embedding_reference(table, ids, p, dy, 2)
        for grads in ((True, True), (True, False), (False, True), (False, False)):
            tt = leaf(table) if grads[0] else Tensor(table)
            pt = None if p is None else (leaf(p) if grads[1] else Tensor(p))
            for idx in (ids, tn.asarray(ids), Tensor(ids)):
                for t in (tt, pt):
                    if t is not None and t.requires_grad:
                        t.zero_grad()
                out = ops.embedding_(tt, idx, pt, padding_idx=2)
                wanted = [t for t in (tt, pt) if t is not None and t.requires_grad]
                assert out.requires_grad == bool(wanted) and len(out.dependency) == len(wanted)
                to.assert_within(out.values, res.values["out"], res.bounds["out"], "out")
                if not wanted:
                    continue
                out.backward(dy)
                for t, field in ((tt, "dtable"), (pt, "dpos")):
                    if t is None:
                        continue
                    if not t.requires_grad:
                        assert t.grad is None
                        continue
                    assert tuple(t.grad.shape) == tuple(t.shape)
                    to.assert_within(np.asarray(t.grad), res.values[field], res.bounds[field], field)
                for dep in out.dependency:                              # the per-edge forms
                    np.testing.assert_array_equal(np.asarray(dep["grad_fn"](tn.asarray(dy))), np.asarray(dep["tensor"].grad))


def test_cross_entropy_op_reductions_ignored_rows_and_upstream_gradient():
    rs = np.random.RandomState(8)
    x, t = to.xent_inputs(rs, 6, 9)
    x3, t3 = x.reshape(2, 3, 9), t.reshape(2, 3)
    for reduction in ("mean", "sum"):
        for ignore_index, rows in ((None, ()), (4, (1, 3)), (4, range(6))):
            tt = t.copy()
            if ignore_index is not None:
                tt[tt == 4] = 5
                tt[list(rows)] = 4
            res = to.cross_entropy_reference(x, tt, ignore_index, reduction, g=-1.5)
            xt = leaf(x3)
            loss = ops.cross_entropy_(xt, tt.reshape(2, 3), ignore_index=ignore_index, reduction=reduction)
            assert loss.shape == ()
            to.assert_within(loss.values, res.values["loss"], res.bounds["loss"], "loss")
            (loss * -1.5).backward()
            to.assert_within(np.asarray(xt.grad).reshape(6, 9), res.values["dlogits"], res.bounds["dlogits"], "dlogits")
            layer = CrossEntropyLoss(ignore_index=ignore_index, reduction=reduction, fused=False)
            xt2 = leaf(x)
            loss2 = layer.loss(xt2, Tensor(tt))
            to.assert_within(loss2.values, res.values["loss"], res.bounds["loss"], "CrossEntropyLoss")
            loss2.backward(-1.5)
            to.assert_within(np.asarray(xt2.grad), res.values["dlogits"], res.bounds["dlogits"], "CrossEntropyLoss dlogits")
            if len(rows) == 6:                                           # every row ignored
                assert float(loss.values) == 0.0 and not np.asarray(xt.grad).any() and not np.asarray(xt2.grad).any()
    assert not ops.cross_entropy(x, t).requires_grad                    # plain arrays: no gradient is wanted
    assert "SoftmaxCrossEntropyLoss" in CrossEntropyLoss.__doc__ and "WHOLE batch" in CrossEntropyLoss.__doc__


def test_rejected_arguments_and_host_range_checks():
    table = Tensor(np.ones((4, 3), dtype=np.float32))
    x = Tensor(np.ones((2, 4), dtype=np.float32))
    for fn, args in ((ops.embedding_, (table, [0])), (ops.embedding, (table, [0])), (ops.cross_entropy_, (x, [0, 1])),
                     (ops.cross_entropy, (x, [0, 1]))):
        with pytest.raises(TypeError, match="unsupported arguments"):
            fn(*args, label_smoothing=0.1)
    for bad in ([0, 4], [-1], np.array([[7]])):
        with pytest.raises(IndexError, match="out of bounds"):
            ops.embedding_(table, bad)
        with pytest.raises(IndexError, match="out of bounds"):
            da.embedding(table.values, bad)
    with pytest.raises(IndexError, match="out of bounds"):
        ops.cross_entropy_(x, [0, 4])
    with pytest.raises(IndexError, match="out of bounds"):
        ops.cross_entropy_(x, [0, -1])
    with pytest.raises(IndexError, match="out of bounds"):
        CrossEntropyLoss(ignore_index=-100).loss(x, np.array([0, -1]))
    assert float(CrossEntropyLoss(ignore_index=-100).loss(x, np.array([0, -100])).values) == pytest.approx(np.log(4.0), rel=1e-6)
    with pytest.raises(TypeError, match="integer ids"):
        ops.embedding_(table, np.array([0.0, 1.0]))
    with pytest.raises(ValueError, match="padding_idx"):
        ops.embedding_(table, [0], padding_idx=4)
    with pytest.raises(ValueError, match="route must be"):
        ops.embedding_(table, [0], route="quick")
    with pytest.raises(ValueError, match="reduction must be"):
        ops.cross_entropy_(x, [0, 1], reduction="none")
    with pytest.raises(ValueError, match="reduction must be"):
        CrossEntropyLoss(reduction="none")
    with pytest.raises(ValueError, match="targets must have shape"):
        ops.cross_entropy_(x, [0, 1, 2])
    assert ops.embedding(np.arange(8).reshape(4, 2), [1]).values.dtype == np.float32          # integers are promoted
    assert ops.embedding_(table, np.zeros((0, 3), dtype=np.int64)).shape == (0, 3, 3)


def test_embedding_layer_order_shapes_and_rng_draws():
    assert EMBED_PARAM_ORDER == ("tok", "pos")
    np.random.seed(3)
    layer = Embedding(7, 4, max_len=5, w_init=NormalInit(0.0, 0.5))
    np.random.seed(3)
    tok, pos = NormalInit(0.0, 0.5)(shape=[7, 4]), NormalInit(0.0, 0.5)(shape=[5, 4])       # drawn in THAT order
    assert list(layer.params) == ["tok", "pos"]
    np.testing.assert_array_equal(np.asarray(layer.params["tok"].values), np.asarray(tok.values))
    np.testing.assert_array_equal(np.asarray(layer.params["pos"].values), np.asarray(pos.values))
    assert all(p.requires_grad for p in layer.params.values())
    plain = Embedding(7, 4, padding_idx=0, fused=False)
    assert list(plain.params) == ["tok"] and plain.params["tok"].shape == (7, 4)
    ids = np.array([[1, 2, 2, 0], [6, 0, 1, 1]])
    out = layer.forward(Tensor(ids))
    assert out.shape == (2, 4, 4)
    res = to.embedding_reference(np.asarray(tok.values), ids, np.asarray(pos.values))
    to.assert_within(out.values, res.values["out"], res.bounds["out"], "Embedding")
    out.backward(np.ones((2, 4, 4), dtype=np.float32))
    assert not np.asarray(layer.params["pos"].grad)[4].any()                  # max_len 5, T 4: the unused row gets zero
    np.testing.assert_array_equal(np.asarray(layer.params["pos"].grad)[:4], np.full((4, 4), 2.0))
    np.testing.assert_array_equal(np.asarray(layer.params["tok"].grad)[:, 0], [2, 3, 2, 0, 0, 0, 1])
    plain.forward(Tensor(ids)).backward(np.ones((2, 4, 4), dtype=np.float32))
    np.testing.assert_array_equal(np.asarray(plain.params["tok"].grad)[:, 0], [0, 3, 2, 0, 0, 0, 1])     # padding_idx 0
    with pytest.raises(ValueError, match="exceed max_len"):
        layer.forward(Tensor(np.zeros((1, 6), dtype=np.int64)))
    with pytest.raises(ValueError, match=r"\[B, T\]"):
        layer.forward(Tensor(np.zeros((6,), dtype=np.int64)))
    with pytest.raises(ValueError, match="padding_idx"):
        Embedding(7, 4, padding_idx=7)
    with pytest.raises(ValueError, match=">= 1"):
        Embedding(0, 4)
    net = Net([layer])
    assert net.parameter_tensors() == [layer.params["tok"], layer.params["pos"]] and net.num_parameters() == 48
    assert np.asarray(Embedding(3, 2, w_init=ConstantInit(1.5)).params["tok"].values).tolist() == [[1.5, 1.5]] * 3


@pytest.mark.parametrize("fused", [True, False])
def test_language_model_against_the_fixture_in_float64(golden, fused):
    """Gradients: max|diff| <= 1e-10 scale per tensor; the loss to 1e-12."""
    tn.set_default_float(np.float64)
    model, loss_layer, ids, targets = ts.lm_model(golden, fused, np.float64)
    loss, grads = ts.lm_step(model, loss_layer, ids, targets)
    np.testing.assert_allclose(float(loss), float(golden["lm.loss"]), rtol=1e-12)
    ts.assert_lm_grads(grads, golden, 1e-10, "float64 fused=%s" % fused)


def test_language_model_in_float32_within_the_reference_gate(golden):
    model, loss_layer, ids, targets = ts.lm_model(golden, True, np.float32)
    loss, grads = ts.lm_step(model, loss_layer, ids, targets)
    ts.assert_lm_grads(grads, golden, golden["lm.f32_gate"], "float32")
    np.testing.assert_allclose(float(loss), float(golden["lm.loss"]), rtol=1e-5)


def test_example_trains_on_the_composed_route():
    """examples/charlm_run.py, shortened, on the twin (everything composed): the mean loss falls and the accuracy on the
    predictable positions exceeds chance, 1 / V."""
    example = ts.load_example()
    args = example.parse(["--num_ep", "2", "--n_train", "256", "--n_test", "32", "--batch_size", "32", "--composed"])
    history = example.main(args)
    assert len(history) == 2 and history[1][0] < history[0][0]
    assert history[1][1] > 1.0 / args.vocab
