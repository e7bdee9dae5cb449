"""csrc/tnn_lce.hip on the MI355X against the float64 reference and the derived bounds of tests/lce_oracle.py, at the smallest
shapes at which each path can go wrong (rows around a wave's 16 and a workgroup's 64, columns around a 256-block, K around the
staged chunk, every kind of split count, row strides with NaN padding)."""

import gc

import numpy as np
import pytest

import lce_oracle as lo
import token_support as ts
from tinynn_autograd_amd import _lib, device_array as da, lce
from tinynn_autograd_amd.core import ops
from tinynn_autograd_amd.core.tensor import Tensor

pytestmark = pytest.mark.gpu
F32, GUARD, POISON = _lib.F32, 16, np.float32(-123.25)
bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
KS = (1, 4, 6, lce.KC - 1, lce.KC, lce.KC + 4)
IGNORE = -5
UPLOADED = []


def upload(host):
    dev = da.asarray(host, dtype=host.dtype)
    UPLOADED.append(dev)
    return dev


@pytest.fixture(autouse=True)
def scrub_the_poison():
    """What a test poisoned is zeroed and every buffer goes back to the native pool when the test ends (test_gpu_wq.py)."""
    yield
    while UPLOADED:
        UPLOADED.pop().fill(0)
    gc.collect()
    da.trim_cache()


def padded(a, pad):
    """The matrix in rows of pad more elements, the padding NaN: never read, or it would show."""
    wide = np.full((a.shape[0], a.shape[1] + pad), np.nan, dtype=np.float32)
    wide[:, :a.shape[1]] = a
    return wide


def guarded(n):
    """A device buffer of n floats between two guards of poison -> (array, pointer to the n floats)."""
    dev = upload(np.full(GUARD + n + GUARD, POISON, dtype=np.float32))
    return dev, dev._ptr + 4 * GUARD


def inside(dev, n):
    got = np.asarray(dev)
    assert (got[:GUARD] == POISON).all() and (got[GUARD + n:] == POISON).all(), "a guard lost its poison"
    return got[GUARD:GUARD + n]


def targets_for(rs, m, v):
    """The last column (the last split's), an ignored row, an out-of-range value; never the column whose bias is -inf."""
    t = rs.randint(0, v, m)
    t[t == v // 2] = v - 1
    t[0] = v - 1
    if m > 1:
        t[1] = IGNORE
    if m > 2:
        t[2] = v + 3
    return t


@pytest.mark.parametrize("v", [1, 12, 255, 256, 257, 516])
@pytest.mark.parametrize("m", [1, 16, 17, 64, 65])
def test_forward_and_dlogits_against_float64(m, v):
    lib, rs = _lib.get(), np.random.RandomState(1000 * m + v)
    t = targets_for(rs, m, v)
    t_dev, one = upload(t.astype(np.int64)), upload(np.ones(1, dtype=np.float32))
    for n, k in enumerate(KS):
        bias, pad, reduction = n % 2 == 0, (0, 3, 4)[n % 3], ("mean", "sum")[n // 2 % 2]
        h, w, b = lo.inputs(rs, m, k, v, bias)
        if bias and v > 1:
            b[0, v // 2] = -np.inf
        ref = lo.reference(h, w, b, t, IGNORE, reduction)
        h_dev, w_dev, b_dev = upload(padded(h, pad)), upload(padded(w, pad)), upload(b) if bias else None
        code = {"mean": 0, "sum": 1}[reduction]                      # TNN_XENT_MEAN, TNN_XENT_SUM
        for splits in sorted({1, min(2, lce.most_splits(v)), lce.choose_splits(m, v), lce.most_splits(v)}):
            what = "M %d K %d V %d splits %d bias %s pad %d %s" % (m, k, v, splits, bias, pad, reduction)
            nws = lce.workspace_bytes(m, splits) // 4
            runs = []
            for _ in range(2):
                out = {name: upload(np.full(size, np.nan, dtype=np.float32)) for name, size in
                       (("losses", m), ("lse", m), ("loss", 1), ("count", 1))}
                ws, ws_ptr = guarded(nws)
                lib.lce_fwd(h_dev._ptr, k + pad, w_dev._ptr, v + pad, da._ptr_of(b_dev), t_dev._ptr, out["losses"]._ptr,
                            out["lse"]._ptr, out["loss"]._ptr, out["count"]._ptr, ws_ptr if nws else None, 4 * nws, m, k, v, splits,
                            IGNORE, code, F32)
                inside(ws, nws)
                runs.append({name: np.asarray(a) for name, a in out.items()})
            got = runs[0]
            assert all(np.array_equal(bits(got[name]), bits(runs[1][name])) for name in got), what
            assert got["count"][0] == ref.values["count"], what
            lo.check(dict(lse=got["lse"], losses=got["losses"], loss=got["loss"][0]), ref, what)
        m0 = 16 if m > 16 else 0                                      # dz of the rows [m0, m) into a guarded chunk
        dz, dz_ptr = guarded((m - m0) * v)
        lib.lce_dlogits(h_dev._ptr, k + pad, w_dev._ptr, v + pad, da._ptr_of(b_dev), t_dev._ptr, out["lse"]._ptr,
                        out["count"]._ptr, one._ptr, dz_ptr, m0, m - m0, m, k, v, IGNORE, code, F32)
        got_dz = inside(dz, (m - m0) * v).reshape(m - m0, v)
        lo.assert_within(got_dz, ref.values["dz"][m0:], ref.bounds["dz"][m0:], "dz M %d K %d V %d" % (m, k, v))
        assert not got_dz[t[m0:] == IGNORE].any()                     # exact zeros for a row that is not counted
        assert not (bias and v > 1 and got_dz[:, v // 2].any())       # ... and for the column whose bias is -inf


@pytest.mark.parametrize("m, k, v, chunk_rows", [(64, 16, 256, 64), (128, 15, 12, 64), (65, 20, 516, 64), (65, 6, 257, None),
                                                 (17, 6, 257, 0)])
def test_gradients_through_the_op(m, k, v, chunk_rows):
    """One chunk, two chunks, a ragged last chunk, the planner's choice; chunk_rows 0: the planner's choice, all rows ignored."""
    rs = np.random.RandomState(m + k + v)
    h, w, b = lo.inputs(rs, m, k, v)
    t = targets_for(rs, m, v) if chunk_rows != 0 else np.full(m, IGNORE)
    t[2] = t[0]                                                       # (host targets are range-checked: no out-of-range value)
    chunk_rows = chunk_rows or None
    chunks = len(lce.plan_linear_cross_entropy(h.shape, w.shape, b.shape, t.shape, chunk_rows=chunk_rows).chunks())
    ref = lo.reference(h, w, b, t, IGNORE, "mean", g=1.0, chunks=chunks)
    fold, runs = (2, m // 2) if m % 2 == 0 else (m,), []             # a leading axis of h folds into the rows
    for _ in range(2):
        th, tw, tb = Tensor(h.reshape(fold + (k,)), requires_grad=True), Tensor(w, requires_grad=True), Tensor(b, requires_grad=True)
        loss = ops.linear_cross_entropy_(th, tw, tb, t.reshape(fold), ignore_index=IGNORE, route="native", chunk_rows=chunk_rows)
        loss.backward()
        runs.append(dict(loss=np.asarray(loss.values), dh=np.asarray(th.grad).reshape(m, k), dw=np.asarray(tw.grad),
                         db=np.asarray(tb.grad)))
    assert all(np.array_equal(bits(runs[0][name]), bits(runs[1][name])) for name in runs[0])
    lo.check(runs[0], ref, "M %d K %d V %d, %d chunks" % (m, k, v, chunks), verbose=True)


def test_three_steps_of_the_example_with_the_fused_head():
    """Width 64, vocab 12: with --fused-head each step's loss is the plain run's within the oracle's bound at that step."""
    ex = ts.load_example()
    argv = ["--width", "64", "--heads", "4", "--seq", "16", "--vocab", "12", "--batch_size", "8"]
    ids, targets = ex.make_data(np.random.RandomState(1), 24, 16, 12, 4)
    runs = {}
    for fused_head in (False, True):
        np.random.seed(11)
        model, loss_layer = ex.build(ex.parse(argv + (["--fused-head"] if fused_head else [])))
        head, steps = model.net.layers[-1].params, []
        for s in range(3):
            x, y = Tensor(ids[8 * s:8 * s + 8]), targets[8 * s:8 * s + 8].reshape(-1)
            model.zero_grad()
            hidden = model.forward(x, hidden=True) if fused_head else None
            loss = loss_layer.loss(hidden if fused_head else model.forward(x), y)
            bound = lo.reference(np.asarray(hidden.values), np.asarray(head["w"].values), np.asarray(head["b"].values),
                                 y).bounds["loss"] if fused_head else None
            loss.backward()
            model.step()
            steps.append((float(loss.values), bound))
        runs[fused_head] = steps
    for s, ((plain, _), (fused, bound)) in enumerate(zip(runs[False], runs[True])):
        print("step %d: loss %.7f without, %.7f with the fused head, bound %.3e" % (s, plain, fused, bound))
        assert abs(plain - fused) <= bound, s
