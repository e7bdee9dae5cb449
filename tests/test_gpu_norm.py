"""csrc/tnn_norm.hip on the MI355X against the float64 oracle (tests/norm_oracle.py) under its DERIVED bounds, and against the
composed route (existing kernels only) under the sum of both routes' bounds.  Shapes are the smallest at which a kernel can
still go wrong: row widths around the 16-byte access, the wave and the two register-capacity limits of the planner, row
counts around the rows of a workgroup and one that makes a wave walk several rows and the parameter gradients need several
partial rows, element-aligned base pointers, every combination of absent operands and gradients."""

import ctypes
import itertools

import numpy as np
import pytest

import norm_oracle as no
import norm_support as ns
import tinynn_autograd_amd as tn
from tinynn_autograd_amd import _lib, norm as nm
from tinynn_autograd_amd import device_array as da
from tinynn_autograd_amd.core import ops
from tinynn_autograd_amd.core.tensor import Tensor

pytestmark = pytest.mark.gpu

R, WMAX, BMAX = nm.ROWS_PER_BLOCK, nm.WAVE_MAX_N, nm.BLOCK_MAX_N
# the three kernel instantiations by row width (csrc/tnn_norm.hip: 4 or 16 elements per lane of a wave, 16 per thread of a block)
FORM_WIDTHS = {"wave4": [1, 3, 4, 5, 63, 64, 65, 255, 256], "wave16": [257, WMAX - 1, WMAX], "block": [WMAX + 1, BMAX]}
# the backward launch that computes a parameter gradient has at most MAX_PARTIALS workgroups: with this many rows a wave of
# the wave form walks two rows THERE and MAX_PARTIALS partial rows are reduced.  (The forward and the dx-only backward
# launch up to 8 workgroups per CU and walk nothing at this count: test_grid_stride_of_every_launch.)
MANY_ROWS = R * nm.MAX_PARTIALS + R + 1
FIELDS3 = ("dx", "dgamma", "dbeta")


@pytest.fixture(scope="module")
def golden():
    return ns.load_golden()


@pytest.fixture(autouse=True)
def _switches():
    yield
    da.NORM_ROUTE = None


def check_both_routes(x, gamma, beta, dy, kind, eps, dtype, what, unaligned=False, need=ns.NEED_ALL, res=None):
    res = res or no.reference(x, gamma, beta, dy, kind, eps, dtype)
    native = ns.run("native", x, gamma, beta, dy, kind, eps, dtype, unaligned, need)
    wanted = (need[0], need[1], need[2] and kind == "layer")
    assert [native[f] is not None for f in FIELDS3] == list(wanted), what
    no.check(native, res, what + " native")
    composed = ns.run("composed", x, gamma, beta, dy, kind, eps, dtype, False, need)
    for name in no.FIELDS:
        if native[name] is None:
            continue
        diff = np.abs(native[name].astype(np.float64) - composed[name].astype(np.float64)).reshape(np.shape(res.bounds[name]))
        assert (diff <= 2 * res.bounds[name]).all(), "%s %s: the routes differ by more than both bounds" % (what, name)
    return native


def test_backend_and_entry_points():
    lib = _lib.get()
    assert tn.backend_name() == "hip-gfx950"
    assert lib.has_norm
    assert nm.plan_norm((4, 8), native=lib.has_norm).route == "native"
    assert nm.gelu_route("none", native=lib.has_norm) == "native"
    y, mean, rstd = da.layer_norm(tn.asarray(np.array([[1.0, 3.0]], dtype=np.float32)), eps=0.0)
    np.testing.assert_array_equal(np.asarray(y), [[-1.0, 1.0]])
    np.testing.assert_array_equal(np.asarray(mean), [2.0])
    np.testing.assert_array_equal(np.asarray(rstd), [1.0])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_fixture_cases(golden, dtype):
    for name in no.NORM_CASES:
        (x, gamma, beta, dy, kind, eps), res = ns.golden_result(golden, name, dtype)
        for unaligned in (False, True):
            check_both_routes(x, gamma, beta, dy, kind, eps, dtype, "%s %s unaligned %d" % (name, np.dtype(dtype).name, unaligned),
                              unaligned=unaligned, res=res)


def combos():
    """(kind, has_gamma, has_beta, (need dx, dgamma, dbeta)) — every combination of absent operands and gradients that
    computes something."""
    out = []
    for has_gamma, has_beta in itertools.product((True, False), repeat=2):
        for need in itertools.product((True, False), repeat=3):
            if any(need):
                out.append(("layer", has_gamma, has_beta, need))
    for has_gamma in (True, False):
        for need in itertools.product((True, False), repeat=2):
            if any(need):
                out.append(("rms", has_gamma, False, need + (False,)))
    return out


def fuzz_plan(seed):
    """The cases of one fuzz run: every (form, kind, absent-operand combination) once, the widths of the form in turn, row
    counts and alignment drawn from a seeded generator."""
    rs = np.random.RandomState(seed)
    table, cases = combos(), []
    assert len(table) == 4 * 7 + 2 * 3
    for i in range(3 * len(table)):
        form = ("wave4", "wave16", "block")[i % 3]
        kind, has_gamma, has_beta, need = table[i // 3]
        n = FORM_WIDTHS[form][(i // 3) % len(FORM_WIDTHS[form])]
        rows = [1, 3, R - 1, R + 1]
        if n <= 65:
            rows.append(MANY_ROWS)                   # about 1 MB at N = 64
        elif n <= WMAX:
            rows.append(4 * R + 1)
        m = int(rs.choice(rows))
        cases.append((form, kind, has_gamma, has_beta, need, m, n, bool(rs.randint(2))))
    return cases


def fuzz(dtype, seed):
    seen, widths, counts, alignments = set(), set(), set(), set()
    for i, (form, kind, has_gamma, has_beta, need, m, n, unaligned) in enumerate(fuzz_plan(seed)):
        rs = np.random.RandomState(seed * 1000 + i)
        # (rows of 0.5 + 1.5 normal: a row mean that happens to be almost 0 is itself a cancelled sum, which the tightness gate
        # of its bound refuses when there are only a few rows; drift: norm_oracle.make_inputs)
        x, gamma, beta, dy = no.make_inputs(rs, (m, n), dtype, offset=0.5, drift=0.5)
        gamma, beta = (gamma if has_gamma else None), (beta if has_beta and kind == "layer" else None)
        eps = 0.5 if (kind == "rms" and n == 1) else 1e-5         # (N = 1: norm_oracle.NORM_CASES["rms_single"])
        assert nm.plan_norm((m, n)).form == ("block" if form == "block" else "wave")
        check_both_routes(x, gamma, beta, dy, kind, eps, dtype, "fuzz %d %s %s M%d N%d gamma %d beta %d need %s unaligned %d" % (
            i, form, kind, m, n, has_gamma, has_beta, need, unaligned), unaligned=unaligned, need=need)
        seen.add((form, kind, has_gamma, has_beta, need))
        widths.add(n)
        counts.add(m)
        alignments.add((form, unaligned))
    assert seen == {(f,) + c for f in FORM_WIDTHS for c in combos()}
    assert widths == set(sum(FORM_WIDTHS.values(), []))
    assert counts == {1, 3, R - 1, R + 1, 4 * R + 1, MANY_ROWS}
    assert alignments == {(f, u) for f in FORM_WIDTHS for u in (False, True)}


def test_fuzz_raw_calls_float32():
    fuzz(np.float32, 2026)


def test_fuzz_raw_calls_float64():
    fuzz(np.float64, 2027)


def test_block_form_walks_several_rows():
    """More rows than the backward launch has workgroups at a width only the block form takes: every workgroup walks two
    rows, MAX_PARTIALS partial rows are reduced (about 4 MB per array)."""
    m, n = nm.MAX_PARTIALS + 3, WMAX + 1
    assert nm.plan_norm((m, n)).form == "block" and nm.plan_norm((m, n)).partials() == nm.MAX_PARTIALS
    x, gamma, beta, dy = no.make_inputs(np.random.RandomState(5), (m, n))
    res = no.reference(x, gamma, beta, dy, "layer", 1e-5, np.float32)
    no.check(ns.run("native", x, gamma, beta, dy, "layer", 1e-5, np.float32), res, "block form, many rows")


@pytest.mark.parametrize("form", ["wave", "block"])
@pytest.mark.parametrize("kind", ["layer", "rms"])
def test_grid_stride_of_every_launch(kind, form):
    """More rows than ANY launch has row slots, counted from the device: the forward and the dx-only backward launch at most
    8 workgroups per CU (ROWS_PER_BLOCK rows each in the wave form, one in the block form), so here every wave, or every
    workgroup, of every launch takes a second row — the grid stride, and in the block form the alternating LDS slots carried
    from one row to the next (RMS norm: ONE sum per row forward, so the parity flips from row to row).  Forward, dx-only
    backward and the backward with parameter gradients, aligned and element-aligned, against the oracle; about 2 MB per
    array in the wave form and 8 MB in the block form."""
    slots = _lib.device_props()["cus"] * 8
    m, n = (slots * R + R + 1, 64) if form == "wave" else (slots + 3, WMAX + 1)
    plan = nm.plan_norm((m, n))
    assert plan.form == form and m > slots * plan.rows_per_block() and plan.partials() == nm.MAX_PARTIALS
    x, gamma, beta, dy = no.make_inputs(np.random.RandomState(m), (m, n), offset=0.5, drift=0.5)
    beta = beta if kind == "layer" else None
    res = no.reference(x, gamma, beta, dy, kind, 1e-5, np.float32)
    for unaligned in (False, True):
        for need in ((True, False, False), ns.NEED_ALL):
            got = ns.run("native", x, gamma, beta, dy, kind, 1e-5, np.float32, unaligned, need)
            assert (got["dgamma"] is not None) == need[1]
            no.check(got, res, "%s %s M%d N%d need %s unaligned %d" % (kind, form, m, n, need, unaligned))
    if form == "wave":
        res = no.reference(x, gamma, beta, dy, kind, 1e-5, np.float64)
        for need in ((True, False, False), ns.NEED_ALL):
            no.check(ns.run("native", x, gamma, beta, dy, kind, 1e-5, np.float64, False, need), res, "%s float64 %s" % (kind, need))


def test_planner_and_library_agree_on_the_workspace():
    """norm.NormPlan.workspace_bytes is what device_array allocates, tnn_norm_bwd_workspace what the launch demands: equal at
    the planner's edge shapes, for every combination of parameter gradients and both dtypes."""
    lib = _lib.get()
    rows = [0, 1, R - 1, R, R + 1, nm.MAX_PARTIALS, nm.MAX_PARTIALS + 1, R * nm.MAX_PARTIALS, R * nm.MAX_PARTIALS + 1, MANY_ROWS]
    for m, n in itertools.product(rows, (1, 5, WMAX, WMAX + 1, BMAX)):
        plan = nm.plan_norm((m, n))
        for with_g, with_b, (code, itemsize) in itertools.product((0, 1), (0, 1), ((_lib.F32, 4), (_lib.F64, 8))):
            need = ctypes.c_int64(-1)
            lib.norm_bwd_workspace(m, n, with_g, with_b, code, ctypes.byref(need))
            assert need.value == plan.workspace_bytes(itemsize, with_g, with_b), (m, n, with_g, with_b, itemsize)


@pytest.mark.parametrize("n", [64, 257])
@pytest.mark.parametrize("kind", ["layer", "rms"])
def test_cancellation(kind, n):
    """Rows of 1000 + 1.5 normal: the variance is a millionth of E[x^2], so a one-pass E[x^2] - mean^2 loses every digit of
    it in float32 and fails these bounds; the deviations from the mean do not."""
    x, gamma, beta, dy = no.make_inputs(np.random.RandomState(n), (R + 1, n), offset=1000.0)
    beta = beta if kind == "layer" else None
    res = no.reference(x, gamma, beta, dy, kind, 1e-5, np.float32)
    if kind == "layer":
        one_pass = (x.astype(np.float32) ** 2).mean(axis=1, dtype=np.float32) - x.mean(axis=1, dtype=np.float32) ** 2
        with np.errstate(invalid="ignore", divide="ignore"):
            bad = 1.0 / np.sqrt(one_pass.astype(np.float64) + 1e-5)
        assert not (np.abs(bad - res.values["rstd"]) <= res.bounds["rstd"]).all()      # the bound does tell the two apart
    for unaligned in (False, True):
        check_both_routes(x, gamma, beta, dy, kind, 1e-5, np.float32, "offset rows %s N%d" % (kind, n), unaligned=unaligned)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [1, 5, 64, WMAX + 1])
def test_constant_rows(dtype, n):
    """A constant row with eps > 0: the mean is the constant itself (3 N is exact and so is its division by N), every
    deviation is 0 and y == beta EXACTLY.  dx of such a row is rstd (g - mean_N(g)) with g = dy gamma — the normalised row is
    0, but the centring still acts on the gradient — so dx == 0 exactly where g is constant along the row (dy constant,
    gamma absent), and it is rstd (g - mean_N(g)) within the oracle's bounds otherwise."""
    rs = np.random.RandomState(n)
    x = np.full((3, n), 3.0, dtype=dtype)
    _, gamma, beta, dy = no.make_inputs(rs, (3, n), dtype)
    for route in ("native", "composed"):
        got = ns.run(route, x, gamma, beta, dy, "layer", 1e-5, dtype)
        np.testing.assert_array_equal(got["y"], np.broadcast_to(beta, (3, n)))
        np.testing.assert_array_equal(got["mean"], np.full(3, 3.0))
        flat = ns.run(route, x, None, None, np.full((3, n), 2.0, dtype=dtype), "layer", 1e-5, dtype)
        assert not flat["y"].any() and not flat["dx"].any()
    res = no.reference(x, gamma, beta, dy, "layer", 1e-5, dtype)
    got = ns.run("native", x, gamma, beta, dy, "layer", 1e-5, dtype)
    g = dy.astype(np.float64) * gamma.astype(np.float64)
    want = (g - g.mean(axis=1, keepdims=True)) / np.sqrt(1e-5)
    np.testing.assert_allclose(res.values["dx"], want, rtol=1e-12, atol=1e-12 * np.abs(want).max() if n > 1 else 0)
    no.assert_within(got["dx"], res.values["dx"], res.bounds["dx"], "constant rows dx", gate=n > 1)
    assert not got["dgamma"].any()                           # dy * 0, summed


def test_single_column():
    """N = 1: layer norm gives beta and no gradient to x; RMS norm gives sign(x) gamma up to eps."""
    x, gamma, beta, dy = no.make_inputs(np.random.RandomState(1), (R + 1, 1))
    got = check_both_routes(x, gamma, beta, dy, "layer", 1e-5, np.float32, "layer N = 1")
    np.testing.assert_array_equal(got["y"], np.broadcast_to(beta, (R + 1, 1)))
    assert not got["dx"].any() and not got["dgamma"].any()
    check_both_routes(x, gamma, None, dy, "rms", 0.5, np.float32, "rms N = 1")


def test_beyond_the_block_limit_takes_the_composed_route():
    n = BMAX + 1
    x, gamma, beta, dy = no.make_inputs(np.random.RandomState(9), (3, n), offset=0.5)
    assert nm.plan_norm(x.shape, native=_lib.get().has_norm).route == "composed"
    with pytest.raises(ValueError, match="native normalisation route"):
        da.layer_norm(ns.dev(x, np.float32), route="native")
    with pytest.raises(ValueError, match="native normalisation route"):
        da.rms_norm(ns.dev(x, np.float32), route="native")
    no.check(ns.run(None, x, gamma, beta, dy, "layer", 1e-5, np.float32), no.reference(x, gamma, beta, dy, "layer", 1e-5),
             "N = %d" % n)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("m, n", [(MANY_ROWS, 64), (4 * R + 1, WMAX), (7, WMAX + 1)])
def test_bit_identical_run_to_run(m, n, dtype):
    x, gamma, beta, dy = no.make_inputs(np.random.RandomState(3), (m, n), dtype)
    assert nm.plan_norm((m, n)).partials() >= 3
    for kind in ("layer", "rms"):
        a = ns.run("native", x, gamma, beta if kind == "layer" else None, dy, kind, 1e-5, dtype)
        b = ns.run("native", x, gamma, beta if kind == "layer" else None, dy, kind, 1e-5, dtype)
        for name in no.FIELDS:
            if a[name] is not None:
                assert np.array_equal(a[name], b[name]), (kind, name)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("form", ["none", "tanh"])
def test_gelu(form, dtype):
    """Both forms at sizes around the 16-byte access and the workgroup, aligned and element-aligned; x holds 0, -0, +-10 and
    +-40 where it is long enough.  Forward and backward within the derived bounds; the backward also agrees with a float64
    central difference of the oracle's forward (truncation h^2 / 3, rounding 4 u64 (|x| + 1) / h, on top of the bound)."""
    h = 1e-5
    for n in (1, 255, 256, 257, 4099):
        x, dy = no.gelu_input(n, n, dtype)
        res = no.gelu_reference(x, dy, form, dtype)
        x64 = x.astype(np.float64)
        cd = (no.gelu64(x64 + h, form) - no.gelu64(x64 - h, form)) / (2 * h) * dy
        for unaligned in (False, True):
            xd, dyd = ns.dev(x, dtype, unaligned), ns.dev(dy, dtype, unaligned)
            y, dx = np.asarray(da.gelu(xd, form)), np.asarray(da.gelu_bwd(xd, dyd, form))
            what = "gelu %s %s n %d unaligned %d" % (form, np.dtype(dtype).name, n, unaligned)
            no.check(dict(y=y, dx=dx), res, what, fields=("y", "dx"))
            assert (np.abs(dx - cd) <= res.bounds["dx"] + np.abs(dy) * (h * h / 3 + 4 * no.U64 * (np.abs(x64) + 1) / h)).all(), what
            if n >= 6:
                np.testing.assert_array_equal(y[:2], [0.0, 0.0])                     # gelu(+-0) is a zero
                assert np.isfinite(y).all() and np.isfinite(dx).all()                # (+-40: nothing overflows)
        if form == "tanh":
            c = np.asarray(da.gelu(ns.dev(x, dtype), form, route="composed"))
            assert (np.abs(c - y) <= 2 * res.bounds["y"]).all()
    xt = Tensor(x, requires_grad=True, dtype=dtype)
    xt.zero_grad()
    out = ops.gelu(xt, approximate=form)
    out.backward(dy)
    no.check(dict(y=out.values, dx=xt.grad), res, "ops.gelu %s" % form, fields=("y", "dx"))


def test_autograd_issues_one_backward_call(monkeypatch):
    """ops.layer_norm_ through Tensor.backward: ONE tnn_norm_bwd call whichever of x, gamma, beta require gradients, with
    NULL for the rest; gradients land in lent arena views."""
    lib = _lib.get()
    calls = []
    real = lib.norm_bwd
    monkeypatch.setattr(lib, "norm_bwd", lambda *a: (calls.append(a[5:8]), real(*a))[1])
    x, gamma, beta, dy = no.make_inputs(np.random.RandomState(2), (2, 9, 40))
    res = no.reference(x, gamma, beta, dy, "layer", 1e-5)

    def leaf(a, home=None):
        t = Tensor(a, requires_grad=True)
        t._grad_home = home
        t.zero_grad()
        return t
    arena = tn.zeros((80,))
    xt, gt, bt = leaf(x), leaf(gamma.reshape(1, 40), arena[:40].reshape(1, 40)), leaf(beta.reshape(1, 40), arena[40:].reshape(1, 40))
    out = ops.layer_norm_(xt, gt, bt)
    out.backward(dy)
    assert len(calls) == 1 and calls[0][1:] == (gt._grad_home._ptr, bt._grad_home._ptr) and calls[0][0] is not None
    assert gt.grad is gt._grad_home and bt.grad is bt._grad_home
    no.check(dict(y=out.values, dx=xt.grad, dgamma=gt.grad, dbeta=bt.grad), res, "ops.layer_norm_")
    np.testing.assert_array_equal(np.asarray(arena), np.concatenate([np.asarray(gt.grad).ravel(), np.asarray(bt.grad).ravel()]))
    gt2 = leaf(gamma)
    ops.layer_norm_(Tensor(x), gt2, Tensor(beta)).backward(dy)          # only gamma: dx and dbeta are NULL
    assert len(calls) == 2 and calls[1][0] is None and calls[1][1] is not None and calls[1][2] is None
    no.check(dict(dgamma=gt2.grad), res, "ops.layer_norm_, x and beta frozen")


def test_block_float64_against_the_fixture(golden):
    tn.set_default_float(np.float64)
    for fused in (True, False):
        losses, grads = ns.block_run(golden, fused, np.float64, no.BLOCK_CASE["steps"])
        ns.assert_block_grads(grads, golden, 1e-10, "float64 fused=%s" % fused)
        np.testing.assert_allclose(losses, golden["block.adam_losses"], rtol=1e-7)


def test_block_float32_within_the_reference_gate(golden):
    """Every gradient tensor within f32_gate — 4 x torch's own float32 - float64 discrepancy — of the fixture; fused and
    fused=False within twice that of each other."""
    gates = golden["block.f32_gate"]
    _, native = ns.block_run(golden, True, np.float32, 1)
    _, composed = ns.block_run(golden, False, np.float32, 1)
    ns.assert_block_grads(native, golden, gates, "float32 fused")
    ns.assert_block_grads(composed, golden, gates, "float32 fused=False")
    for name, scale, gate in zip(no.BLOCK_NAMES, golden["block.grad_scale"], gates):
        assert np.abs(native[name] - composed[name]).max() <= 2 * gate * scale, name


def test_block_steps_replayed_from_a_captured_graph(golden):
    """Two eager steps and two replays of the captured step give the losses of four eager steps bit for bit; the first three
    are the fixture's."""
    eager, _ = ns.block_run(golden, True, np.float32, 4)
    np.testing.assert_allclose(eager[:3], golden["block.adam_losses"], rtol=1e-5)
    model, x, y = ns.block_model(golden, True, np.float32)
    state, losses = {}, []

    def step():
        state["loss"] = ns.block_step(model, x, y, read_grads=False)[0]
        return state["loss"]

    def eager_step():
        step()
        losses.append(float(state["loss"]))
    eager_step()
    eager_step()
    captured = tn.capture(step, warmup=0)
    for _ in range(2):
        losses.append(float(captured()))
    assert losses == list(eager)


@pytest.mark.parametrize("composed", [False, True])
def test_example_trains(composed):
    """examples/transformer_run.py, shortened: the mean loss falls from epoch to epoch on the native kernels and with
    --composed."""
    example = ns.load_example()
    history = example.main(example.parse(["--num_ep", "2", "--n_train", "512", "--n_test", "64"] + (["--composed"] if composed else [])))
    assert len(history) == 2 and history[1][0] < history[0][0]
