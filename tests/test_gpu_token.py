"""csrc/tnn_token.hip on the MI355X against the float64 oracle (tests/token_oracle.py) under its DERIVED bounds, and against the
composed route (existing kernels only) under the sum of both routes' bounds.  Shapes are the smallest at which a kernel can
still go wrong: widths around the 16-byte access and the wave, vocabularies around one placement workgroup's range, position
counts around the placement walk's chunk and the segments of the sum, row widths around the limit between the two
cross-entropy forms and one that makes the streaming form loop with a ragged tail, element-aligned base pointers."""

import ctypes
import itertools

import numpy as np
import pytest

import token_oracle as to
import token_support as ts
import tinynn_autograd_amd as tn
from tinynn_autograd_amd import _lib, tokens as tk
from tinynn_autograd_amd import device_array as da
from tinynn_autograd_amd.core import ops
from tinynn_autograd_amd.core.tensor import Tensor

pytestmark = pytest.mark.gpu

K, RANGE, CHUNK = tk.EMBED_SEGMENT, tk.EMBED_VOCAB_PER_BLOCK, tk.EMBED_WALK_CHUNK
WMAX, RB, STEP = tk.XENT_WAVE_MAX_V, tk.XENT_ROWS_PER_BLOCK, tk.XENT_BLOCK_STEP
WIDTHS = [1, 3, 4, 5, 63, 64, 65, 256, 257]
VOCABS = [1, 2, 7, RANGE + 1]                  # the last: two placement workgroups
COUNTS = [1, 3, 4 * CHUNK + 1]
PATTERNS = ["distinct", "equal", "absent", "padding", "out_of_range"]
NEEDS = [(True, True), (True, False), (False, True)]
CLASSES = [1, 2, 3, 4, 5, 63, 64, 65, WMAX - 1, WMAX, WMAX + 1, 2 * STEP + 37]     # the last: 3 steps (float64: 5), ragged tail
FEATURES = ["plain", "offset", "neg_inf", "tail_max"]
IGNORES = ["none", "some", "all", "out_of_range"]


@pytest.fixture(scope="module")
def golden():
    return ts.load_golden()


@pytest.fixture(autouse=True)
def _switches():
    yield
    da.TOKEN_ROUTE = None


def many_rows():
    """More rows than the wave form's launch has row slots (8 workgroups per CU, RB rows each): every wave walks a second
    row, and every thread of the loss reduction adds many rows."""
    return _lib.device_props()["cus"] * 8 * RB + RB + 1


def make_ids(rs, pattern, m, v):
    """(ids [m], padding_idx, must stay on the device)."""
    if pattern == "distinct" and v >= m:
        return rs.permutation(v)[:m].astype(np.int64), None, False
    if pattern == "equal":
        return np.full(m, v - 1, dtype=np.int64), None, False
    if pattern == "absent":
        return rs.randint(0, max(1, v // 2), m).astype(np.int64), None, False        # the upper half never occurs
    ids = rs.randint(0, v, m).astype(np.int64)
    if pattern == "padding":
        return ids, int(ids[0]), False
    if pattern == "out_of_range":
        ids[::2] = [-1, v, v + 5, -(1 << 40)][m % 4]
        return ids, None, True
    return ids, None, False


def check_embed(table, ids, pos, dy, padding_idx, dtype, what, unaligned=False, need=(True, True), device_ids=False, res=None,
                composed=True):
    res = res or to.embedding_reference(table, ids, pos, dy, padding_idx, dtype)
    native = ts.run_embed("native", table, ids, pos, dy, padding_idx, dtype, unaligned, need, device_ids, poison=True)
    assert [native[f] is not None for f in ("dtable", "dpos")] == [need[0], need[1] and pos is not None], what
    to.check(native, res, what + " native", fields=to.EMBED_FIELDS)
    if pos is None:
        assert np.array_equal(native["out"], res.values["out"].astype(dtype)), what + ": the lookup is a copy"
    if composed:
        other = ts.run_embed("composed", table, ids, pos, dy, padding_idx, dtype, False, need, device_ids)
        for name in to.EMBED_FIELDS:
            if native[name] is not None:
                diff = np.abs(native[name].astype(np.float64) - other[name].astype(np.float64))
                assert (diff <= 2 * res.bounds[name]).all(), "%s %s: the routes differ by more than both bounds" % (what, name)
    return native


def check_xent(x, t, ignore_index, reduction, g, dtype, what, unaligned=False, device_targets=False, res=None):
    plan = tk.plan_cross_entropy(x.shape, t.shape)
    rescales = plan.steps(np.dtype(dtype).itemsize) + 2 if plan.form == "block" else 0
    res = res or to.cross_entropy_reference(x, t, ignore_index, reduction, g, dtype, rescales=rescales)
    native = ts.run_xent("native", x, t, ignore_index, reduction, g, dtype, unaligned, device_targets)
    to.check(native, res, what + " native", fields=to.XENT_FIELDS)
    other = ts.run_xent("composed", x, t, ignore_index, reduction, g, dtype, False, device_targets)
    for name in to.XENT_FIELDS:
        diff = np.abs(native[name].astype(np.float64) - other[name].astype(np.float64))
        assert (diff <= 2 * res.bounds[name]).all(), "%s %s: the routes differ by more than both bounds" % (what, name)
    return native


def test_backend_and_entry_points():
    lib = _lib.get()
    assert tn.backend_name() == "hip-gfx950" and lib.has_token
    assert tk.plan_embedding((4, 8), (3,), native=lib.has_token).route == "native"
    assert tk.plan_cross_entropy((4, 8), (4,), native=lib.has_token).route == "native"
    table = np.arange(12, dtype=np.float32).reshape(4, 3)
    np.testing.assert_array_equal(np.asarray(da.embedding(tn.asarray(table), [3, 1, 3])), table[[3, 1, 3]])
    loss, _, lse, count = da.cross_entropy(tn.asarray(np.zeros((2, 4), dtype=np.float32)), [0, 3])
    assert float(count) == 2.0 and abs(float(loss) - np.log(4.0)) < 1e-6


def test_table_gradient_accumulates_where_getitem_keeps_the_last():
    """ids [3, 1, 3, 3]: ops.embedding_ gives np.add.at's gradient; table[ids] through ops.getitem_ keeps the last one."""
    table, ids, _, dy, _ = to.embed_case("embed_repeat")
    res = to.embedding_reference(table, ids, None, dy)
    want = np.zeros(table.shape)
    np.add.at(want, ids, dy.astype(np.float64))
    tt = Tensor(table, requires_grad=True)
    ops.embedding_(tt, ids).backward(dy)
    to.assert_within(np.asarray(tt.grad), want, res.bounds["dtable"], "embedding_ dtable")
    ts.assert_getitem_keeps_the_last(Tensor(table, requires_grad=True), ids, dy, want, res.bounds["dtable"])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_fixture_cases(golden, dtype):
    for name in to.EMBED_CASES:
        (table, ids, pos, dy, padding_idx), res = ts.golden_embed(golden, name, dtype)
        for unaligned in (False, True):
            check_embed(table, ids, pos, dy, padding_idx, dtype, "%s unaligned %d" % (name, unaligned), unaligned, res=res)
    for name in to.XENT_CASES:
        (x, t, ignore_index, reduction, g), res = ts.golden_xent(golden, name, dtype)
        for unaligned in (False, True):
            check_xent(x, t, ignore_index, reduction, g, dtype, "%s unaligned %d" % (name, unaligned), unaligned, res=res)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_embedding_sweep(dtype):
    """Every width, vocabulary, position count, id pattern, gradient combination and alignment at least once, with and
    without positions; the gradients land in buffers pre-filled with NaN, so every row is proven written."""
    seen = {k: set() for k in ("e", "v", "m", "pattern", "need", "pos", "unaligned")}
    for i, e in enumerate(WIDTHS * 4):
        rs = np.random.RandomState(1000 * np.dtype(dtype).itemsize + i)
        v, m, pattern = VOCABS[i % 4], COUNTS[i % 3], PATTERNS[i % 5]
        need, with_pos, unaligned = NEEDS[(i // 2) % 3], i % 2 == 0, (i // 3) % 2 == 1
        ids, padding_idx, on_device = make_ids(rs, pattern, m, v)
        shape = (m, 1) if i % 4 < 2 else (1, m)
        table, pos, dy = to.embed_inputs(rs, v, e, shape, (shape[1] + (i // 2) % 2) if with_pos else None, dtype)
        what = "case %d E%d V%d M%d %s need %s pos %d unaligned %d" % (i, e, v, m, pattern, need, with_pos, unaligned)
        # (a device id outside [0, V) has no defined meaning for the row gather of the composed forward: native only)
        check_embed(table, ids.reshape(shape), pos, dy, padding_idx, dtype, what, unaligned, need, on_device, composed=not on_device)
        for key, value in zip(sorted(seen), (e, m, need, pattern, with_pos, unaligned, v)):
            seen[key].add(value)
    assert seen["e"] == set(WIDTHS) and seen["v"] == set(VOCABS) and seen["m"] == set(COUNTS)
    assert seen["pattern"] == set(PATTERNS) and seen["need"] == set(NEEDS)
    assert seen["pos"] == {True, False} and seen["unaligned"] == {True, False}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_embedding_segment_edges_and_sequences(dtype):
    """Tokens with exactly K, K + 1 and 2 K + 1 positions — the edges of the fixed segments of the sum — among others, in a
    shuffled order, over several sequences so that dpos adds up B rows; every combination of wanted gradients."""
    rs = np.random.RandomState(7)
    ids = np.concatenate([np.full(K, 2), np.full(K + 1, 4), np.full(2 * K + 1, 5), rs.randint(0, 2, 2 * K - 2)]).astype(np.int64)
    assert ids.size == 6 * K and np.bincount(ids, minlength=7)[[2, 4, 5]].tolist() == [K, K + 1, 2 * K + 1]
    for order in ("sorted", "shuffled"):
        if order == "shuffled":
            rs.shuffle(ids)
        for e, unaligned in ((5, False), (64, False), (64, True)):
            shape = (6, K)
            table, pos, dy = to.embed_inputs(rs, 7, e, shape, K, dtype)
            for need in NEEDS:
                check_embed(table, ids.reshape(shape), pos, dy, None, dtype, "%s E%d need %s" % (order, e, need), unaligned, need)


def test_embedding_workspace_agrees_with_the_planner():
    lib = _lib.get()
    for m, v, e in itertools.product((0, 1, K, K + 1, 4 * CHUNK + 1), (1, 7, RANGE + 1), (1, 5, 64)):
        for code, itemsize in ((_lib.F32, 4), (_lib.F64, 8)):
            need = ctypes.c_int64(-1)
            lib.embed_bwd_workspace(m, v, e, code, ctypes.byref(need))
            assert need.value == tk.plan_embedding((v, e), (m,)).workspace_bytes(itemsize), (m, v, e, itemsize)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_cross_entropy_sweep(dtype):
    """Every class count, row count, row feature, ignore pattern, reduction and alignment at least once; targets at 0 and
    V - 1 in every case; an upstream gradient other than 1."""
    seen = {k: set() for k in ("v", "m", "feature", "ignore", "reduction", "unaligned")}
    many = many_rows()
    for i, v in enumerate(CLASSES * 4):
        rs = np.random.RandomState(2000 * np.dtype(dtype).itemsize + i)
        m = [1, 3, RB - 1, RB + 1, many if v <= 65 else 2 * RB + 1][(i // 2) % 5]
        feature, ignore = FEATURES[i % 4], IGNORES[(i // 3) % 4]
        reduction, g, unaligned = ("mean", "sum")[(i // 4) % 2], (1.0, -0.75, 2.5)[i % 3], (i // 5) % 2 == 1
        x, t = to.xent_inputs(rs, m, v, 1000.0 if feature == "offset" else 0.0, dtype=dtype)
        if feature == "tail_max":
            x[:, v - 1] += 10.0                                  # the row maximum sits in the last (tail) column
        if feature == "neg_inf" and v > 1:
            x[:, ::3] = -np.inf                                  # masked classes; the target's own logit stays finite
            x[np.arange(m), t] = 0.5
        ignore_index, on_device = None, False
        if ignore == "some" and m > 1:
            ignore_index = int(t[1])
        elif ignore in ("all", "some"):
            ignore_index = v - 1
            t[:] = v - 1
        elif ignore == "out_of_range":                           # only device-resident targets can hold such values
            t[::2] = [v, -7, v + (1 << 33)][i % 3]
            on_device = True
        what = "case %d V%d M%d %s ignore %s %s g %g unaligned %d" % (i, v, m, feature, ignore, reduction, g, unaligned)
        got = check_xent(x, t, ignore_index, reduction, g, dtype, what, unaligned, on_device)
        if ignore == "all" or (ignore == "some" and m == 1):
            assert got["count"] == 0 and got["loss"] == 0 and not got["dlogits"].any() and not got["losses"].any(), what
        assert np.isfinite(got["lse"]).all() and np.isfinite(got["dlogits"]).all(), what
        for key, value in zip(sorted(seen), (feature, ignore, m, reduction, unaligned, v)):
            seen[key].add(value)
    assert seen["v"] == set(CLASSES) and seen["m"] == {1, 3, RB - 1, RB + 1, many, 2 * RB + 1}
    assert seen["feature"] == set(FEATURES) and seen["ignore"] == set(IGNORES)
    assert seen["reduction"] == {"mean", "sum"} and seen["unaligned"] == {True, False}


def test_streaming_form_walks_rows_and_steps():
    """More rows than the streaming form's launch has workgroups at a width of several steps would be 270 MB; its row walk
    is exercised instead through a width just past the wave limit with many rows (every workgroup takes a second row, the
    LDS slots are reused), and its step loop at few rows through the widest CLASSES entry (test_cross_entropy_sweep)."""
    m, v = _lib.device_props()["cus"] * 8 + 3, WMAX + 1
    assert tk.plan_cross_entropy((m, v), (m,)).form == "block"
    x, t = to.xent_inputs(np.random.RandomState(4), m, v)
    res = to.cross_entropy_reference(x, t, None, "mean", 1.0, np.float32, rescales=3)
    for unaligned in (False, True):
        to.check(ts.run_xent("native", x, t, None, "mean", 1.0, np.float32, unaligned), res, "block form, many rows",
                 fields=to.XENT_FIELDS)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_bit_identical_run_to_run(dtype):
    """Every backward and the loss reduction, called twice: identical bits."""
    rs = np.random.RandomState(3)
    m = 4 * CHUNK + 1
    for v, e in ((3, 65), (RANGE + 1, 64)):
        ids = rs.randint(0, v, (m, 1)).astype(np.int64)
        ids[: m // 2] = v - 1                                     # one token owns half the positions: several partial rows
        table, pos, dy = to.embed_inputs(rs, v, e, ids.shape, 1, dtype)
        a = ts.run_embed("native", table, ids, pos, dy, None, dtype, poison=True)
        b = ts.run_embed("native", table, ids, pos, dy, None, dtype, poison=True)
        assert all(np.array_equal(a[f], b[f]) for f in to.EMBED_FIELDS), (v, e)
    for rows, v in ((many_rows(), 64), (2 * RB + 1, WMAX), (7, 2 * STEP + 37)):
        x, t = to.xent_inputs(rs, rows, v, dtype=dtype)
        a = ts.run_xent("native", x, t, int(t[1]), "mean", 0.5, dtype)
        b = ts.run_xent("native", x, t, int(t[1]), "mean", 0.5, dtype)
        assert all(np.array_equal(a[f], b[f]) for f in to.XENT_FIELDS), (rows, v)


def test_autograd_issues_one_backward_call(monkeypatch):
    """ops.embedding_ through Tensor.backward: ONE tnn_embed_bwd call for table and pos together, written into lent arena
    views, NULL for a gradient nobody wants; ops.cross_entropy_: one tnn_xent_bwd launch."""
    lib = _lib.get()
    calls = []
    real_e, real_x = lib.embed_bwd, lib.xent_bwd
    monkeypatch.setattr(lib, "embed_bwd", lambda *a: (calls.append(("embed",) + a[2:4]), real_e(*a))[1])
    monkeypatch.setattr(lib, "xent_bwd", lambda *a: (calls.append(("xent", a[5])), real_x(*a))[1])
    rs = np.random.RandomState(2)
    table, pos, dy = to.embed_inputs(rs, 6, 8, (3, 4), 4)
    ids = rs.randint(0, 6, (3, 4))
    res = to.embedding_reference(table, ids, pos, dy)

    def leaf(a, home=None):
        t = Tensor(a, requires_grad=True)
        t._grad_home = home
        t.zero_grad()
        return t
    arena = tn.zeros((80,))
    tt, pt = leaf(table, arena[:48].reshape(6, 8)), leaf(pos, arena[48:].reshape(4, 8))
    out = ops.embedding_(tt, tn.asarray(ids), pt)
    out.backward(dy)
    assert calls == [("embed", tt._grad_home._ptr, pt._grad_home._ptr)]
    assert tt.grad is tt._grad_home and pt.grad is pt._grad_home
    to.check(dict(out=out.values, dtable=tt.grad, dpos=pt.grad), res, "ops.embedding_", fields=to.EMBED_FIELDS)
    pt2 = leaf(pos)
    ops.embedding_(Tensor(table), ids, pt2).backward(dy)           # only pos: dtable is NULL
    assert calls[1][0] == "embed" and calls[1][1] is None and calls[1][2] is not None
    to.check(dict(dpos=pt2.grad), res, "ops.embedding_, table frozen", fields=("dpos",))
    x, t = to.xent_inputs(rs, 5, 9)
    xt = leaf(x)
    ops.cross_entropy_(xt, t).backward()
    assert len(calls) == 3 and calls[2][0] == "xent"
    to.check(dict(dlogits=xt.grad), to.cross_entropy_reference(x, t), "ops.cross_entropy_", fields=("dlogits",))


def test_language_model_float64_against_the_fixture(golden):
    tn.set_default_float(np.float64)
    for fused in (True, False):
        model, loss_layer, ids, targets = ts.lm_model(golden, fused, np.float64)
        loss, grads = ts.lm_step(model, loss_layer, ids, targets)
        np.testing.assert_allclose(float(loss), float(golden["lm.loss"]), rtol=1e-12)
        ts.assert_lm_grads(grads, golden, 1e-10, "float64 fused=%s" % fused)


def test_language_model_float32_within_the_reference_gate(golden):
    """Every gradient tensor within f32_gate — 4 x torch's own float32 - float64 discrepancy — of the fixture; fused and
    fused=False within twice that of each other."""
    gates = golden["lm.f32_gate"]
    results = []
    for fused in (True, False):
        model, loss_layer, ids, targets = ts.lm_model(golden, fused, np.float32)
        loss, grads = ts.lm_step(model, loss_layer, ids, targets)
        np.testing.assert_allclose(float(loss), float(golden["lm.loss"]), rtol=1e-5)
        ts.assert_lm_grads(grads, golden, gates, "float32 fused=%s" % fused)
        results.append(grads)
    for name, scale, gate in zip(to.LM_NAMES, golden["lm.grad_scale"], gates):
        assert np.abs(results[0][name] - results[1][name]).max() <= 2 * gate * scale, name


def test_training_step_replayed_from_a_captured_graph(golden):
    """One eager step and three replays of the captured step (Embedding -> block -> head -> CrossEntropyLoss -> Adam) give
    the losses of four eager steps bit for bit — the tolerance of the block's own capture test."""
    def run(steps):
        model, loss_layer, ids, targets = ts.lm_model(golden, True, np.float32)
        return [float(ts.lm_step(model, loss_layer, ids, targets)[0]) for _ in range(steps)]
    eager = run(4)
    assert eager[3] < eager[0]
    model, loss_layer, ids, targets = ts.lm_model(golden, True, np.float32)
    state = {}

    def step():
        state["loss"] = ts.lm_step(model, loss_layer, ids, targets, read_grads=False)[0]
        return state["loss"]
    step()
    losses = [float(state["loss"])]
    captured = tn.capture(step, warmup=0)
    for _ in range(3):
        losses.append(float(captured()))
    assert losses == eager


def test_example_trains():
    """examples/charlm_run.py, shortened, on the native kernels: the mean loss falls and the accuracy on the predictable
    positions exceeds chance, 1 / V."""
    example = ts.load_example()
    args = example.parse(["--num_ep", "2", "--n_train", "512", "--n_test", "64"])
    history = example.main(args)
    assert len(history) == 2 and history[1][0] < history[0][0]
    assert history[1][1] > 1.0 / args.vocab
