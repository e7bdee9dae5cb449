"""csrc/tnn_ostep.hip on the MI355X against the planner's numpy reference (tinynn-autograd_amd/ostep.py), the float64 oracle and
the composed route.  Shapes are the smallest at which the kernels can still go wrong: sizes around one 4-element block, one wave
and one workgroup, one size that makes every launch walk its grid stride once and end ragged, element-aligned base pointers
for each operand in turn, and decay-run borders at every residue mod 4.

Bounds.  gnorm: n 2^-52 relative to the float64 norm of the dtype-rounded gradient, the worst case of ANY summation order in
float64.  p, m, v: 1e-12 of the tensor's max-norm in float64, the project's RTOL = 1e-5 of it in float32, with gradients of
|g| >= 0.1 (tests/ostep_oracle.py says why).  lr: 1e-12 relative to the planner's float64 schedule — two double-precision
cosines differ by a few ulp."""

import numpy as np
import pytest

import dropout_support as dsu
import ostep_oracle as oo
import ostep_support as su
import tinynn_autograd_amd as tn
from tinynn_autograd_amd import _lib, ostep
from tinynn_autograd_amd.core.layers import Dense, ReLU
from tinynn_autograd_amd.core.losses import SoftmaxCrossEntropyLoss, SquaredErrorLoss
from tinynn_autograd_amd.core.model import Model
from tinynn_autograd_amd.core.nn import Net
from tinynn_autograd_amd.core.optimizer import Adam, AdamW
from tinynn_autograd_amd.core.tensor import Tensor

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025]
STRIDE_N = 4 * ostep.THREADS * ostep.MAX_BLOCKS + 5      # every lane of a full grid takes one block, then 5 elements remain
DTYPES = [np.float32, np.float64]
HYPER = dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, wd=0.1)


def operands(n, dtype, seed=0):
    """p, g (|g| >= 0.1), and a state as after a few steps: m of both signs, v > 0."""
    rs = np.random.RandomState(seed)
    p = rs.standard_normal(n).astype(dtype)
    g = oo.gradients(rs, (n,)).astype(dtype)
    m = (0.3 * rs.standard_normal(n)).astype(dtype)
    v = rs.uniform(0.05, 0.5, n).astype(dtype)
    return p, g, m, v


def warm_state(lr=1e-2, t=3):
    st = ostep.initial_state(lr)
    st[ostep.T], st[ostep.B1_POW], st[ostep.B2_POW] = t, 0.9 ** t, 0.999 ** t
    return st


def halves(n):
    return ostep.decay_runs([(0, n // 2), (n // 2, n - n // 2)], [True, False])


def native(p, g, m, v, state, hyper, runs, unaligned=(False,) * 4, step_out=False):
    """One step through the raw entry points.  Returns host copies (p, m, v, record, step_out or None)."""
    lib, dtype, n = _lib.get(), p.dtype, p.size
    pd, gd, md, vd = (dsu.dev(a, dtype, u) for a, u in zip((p, g, m, v), unaligned))
    rec = tn.asarray(np.asarray(state, dtype=np.float64), dtype=np.float64)
    table = tn.asarray(ostep.run_table(*runs), dtype=np.int64)
    ws = tn.empty((max(ostep.grid(n), 1),), np.float64)
    code, sch, wsp = gd._code(), hyper.schedule, None
    if hyper.need_norm() and n:
        lib.ostep_sumsq(gd._ptr, n, ws._ptr, ostep.workspace_bytes(n), code)
        wsp = ws._ptr
    lib.ostep_begin(rec._ptr, wsp, n, -1.0 if hyper.max_norm is None else hyper.max_norm, int(hyper.guard), hyper.b1, hyper.b2,
                    sch.kind, hyper.lr, sch.min_lr, sch.warmup, sch.total)
    so = tn.zeros((n,), dtype) if step_out else None
    lib.ostep_adamw(pd._ptr, gd._ptr, md._ptr, vd._ptr, so._ptr if step_out else None, n, rec._ptr, table._ptr, len(runs[0]),
                    hyper.b1, hyper.b2, hyper.eps, hyper.wd, code)
    return np.asarray(pd).copy(), np.asarray(md).copy(), np.asarray(vd).copy(), np.asarray(rec).copy(), \
        (np.asarray(so).copy() if step_out else None)


def check_against_reference(p, g, m, v, state, hyper, runs, what, **kw):
    got = native(p, g, m, v, state, hyper, runs, **kw)
    want = ostep.reference(p, g, m, v, state, hyper, runs)
    bound = su.tol(p.dtype)
    new_p = p + got[4] if kw.get("step_out") else got[0]             # (step_out: p is untouched, the step is the change)
    for name, a, b in zip("pmv", (new_p,) + got[1:3], want[:3]):
        np.testing.assert_allclose(a.astype(np.float64), b.astype(np.float64), rtol=0, atol=bound * np.abs(b).max(),
                                   err_msg="%s: %s" % (what, name))
    rec, ref = got[3], want[3]
    if hyper.need_norm():
        exact = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
        print("%s: gnorm %.17g, float64 norm %.17g" % (what, rec[ostep.GNORM], exact))
        assert abs(rec[ostep.GNORM] - exact) <= p.size * 2.0 ** -52 * exact, what
    np.testing.assert_allclose(rec[ostep.COEF], ref[ostep.COEF], rtol=max(p.size, 4) * 2.0 ** -52, err_msg=what)
    np.testing.assert_allclose(rec[ostep.LR], ref[ostep.LR], rtol=1e-12, err_msg=what)
    for i in (ostep.T, ostep.SKIPPED, ostep.SKIP, ostep.B1_POW, ostep.B2_POW):
        assert rec[i] == ref[i], (what, i)
    return got


def test_backend_and_entry_points():
    lib = _lib.get()
    assert tn.backend_name() == "hip-gfx950" and lib.has_ostep
    assert ostep.plan_ostep(100, np.float32, native=lib.has_ostep).route == "native"
    import ctypes
    for n in (0, 1, 257, STRIDE_N):
        for code in (_lib.F32, _lib.F64):
            out = ctypes.c_int64(-1)
            lib.ostep_workspace(n, code, ctypes.byref(out))
            assert out.value == ostep.workspace_bytes(n)
    with pytest.raises(_lib.TnnError, match="float32 and float64"):
        lib.ostep_scale(None, 4, None, _lib.I64)


@pytest.mark.parametrize("dtype", DTYPES)
def test_sizes(dtype):
    hyper = ostep.Hyper(max_norm=1.0, schedule=ostep.Cosine(2, 10, 1e-4), **HYPER)
    for n in SIZES:
        p, g, m, v = operands(n, dtype, n)
        check_against_reference(p, g, m, v, warm_state(), hyper, halves(n), "n %d %s" % (n, np.dtype(dtype).name))


@pytest.mark.parametrize("dtype", DTYPES)
def test_grid_stride_and_ragged_tail(dtype):
    """More blocks than MAX_BLOCKS workgroups hold: every lane walks its grid stride once and the launch ends ragged."""
    n = STRIDE_N
    assert ostep.grid(n) == ostep.MAX_BLOCKS
    p, g, m, v = operands(n, dtype, 1)
    hyper = ostep.Hyper(max_norm=1.0, **HYPER)
    runs = ostep.decay_runs([(0, 1000003), (1000003, n - 1000003 - 6), (n - 6, 6)], [True, False, True])
    check_against_reference(p, g, m, v, warm_state(), hyper, runs, "stride %s" % np.dtype(dtype).name)


@pytest.mark.parametrize("dtype", DTYPES)
def test_base_pointers_offset_by_one_element(dtype):
    hyper = ostep.Hyper(max_norm=1.0, **HYPER)
    for n in (5, 257, 1025):
        p, g, m, v = operands(n, dtype, n + 1)
        for k in range(4):
            unaligned = tuple(i == k for i in range(4))
            check_against_reference(p, g, m, v, warm_state(), hyper, halves(n), "n %d, operand %d offset" % (n, k),
                                    unaligned=unaligned)
    p, g, m, v = operands(257, dtype, 9)
    got = check_against_reference(p, g, m, v, warm_state(), hyper, halves(257), "step_out offset", unaligned=(False, True, False, False),
                                  step_out=True)
    assert got[0].tobytes() == p.tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
def test_run_borders_at_every_residue(dtype):
    hyper = ostep.Hyper(max_norm=None, **HYPER)
    sizes = [1, 2, 3, 5, 7] * 12                                  # borders at every residue mod 4, several times over
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    runs = ostep.decay_runs(list(zip(offsets, sizes)), [i % 2 == 0 for i in range(len(sizes))])
    assert len(runs[0]) == len(sizes) and {int(s) % 4 for s in runs[0]} == {0, 1, 2, 3}
    n = sum(sizes)
    check_against_reference(*operands(n, dtype, 2), warm_state(), hyper, runs, "segments 1 2 3 5 7")
    # 40 alternating runs inside 257 elements
    cuts = np.sort(np.random.RandomState(3).choice(np.arange(1, 257), 39, replace=False))
    bounds = np.concatenate([[0], cuts, [257]])
    runs = ostep.decay_runs([(int(a), int(b - a)) for a, b in zip(bounds[:-1], bounds[1:])], [i % 2 == 1 for i in range(40)])
    assert len(runs[0]) == 40
    check_against_reference(*operands(257, dtype, 4), warm_state(), hyper, runs, "40 runs")
    # a single run, decayed and not
    for flag in (True, False):
        check_against_reference(*operands(257, dtype, 5), warm_state(), hyper, ostep.decay_runs([(0, 257)], [flag]), "one run")
    # the flags matter: decayed and undecayed results differ where, and only where, the flag differs
    p, g, m, v = operands(64, dtype, 6)
    a = native(p, g, m, v, warm_state(), hyper, ostep.decay_runs([(0, 64)], [False]))[0]
    b = native(p, g, m, v, warm_state(), hyper, ostep.decay_runs([(0, 30), (30, 34)], [False, True]))[0]
    assert a[:30].tobytes() == b[:30].tobytes() and (a[30:] != b[30:]).all()


@pytest.mark.parametrize("kind", ["cosine", "linear"])
def test_lr_from_the_record_follows_the_schedule(kind):
    warmup, total, base, min_lr = 3, 8, 1e-2, 1e-4
    sched = (ostep.Cosine if kind == "cosine" else ostep.Linear)(warmup, total, min_lr)
    lib = _lib.get()
    rec = tn.asarray(ostep.initial_state(base), dtype=np.float64)
    for t in range(1, total + 4):
        lib.ostep_begin(rec._ptr, None, 0, -1.0, 1, 0.9, 0.999, sched.kind, base, min_lr, warmup, total)
        if t in (1, warmup, warmup + 1, total + 3):
            st = np.asarray(rec)
            print("%s t %d: lr %.17g, planner %.17g" % (kind, t, st[ostep.LR], sched.value(t, base)))
            assert st[ostep.T] == t and st[ostep.GNORM] == 0.0 and st[ostep.COEF] == 1.0 and st[ostep.SKIP] == 0.0
            np.testing.assert_allclose(st[ostep.LR], sched.value(t, base), rtol=1e-12, atol=0)
            np.testing.assert_allclose(st[[ostep.B1_POW, ostep.B2_POW]], [0.9 ** t, 0.999 ** t], rtol=1e-14)


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_conditions(dtype):
    n = 1025
    p, g, m, v = operands(n, dtype, 7)
    runs = halves(n)
    clip = ostep.Hyper(max_norm=1.0, **HYPER)
    # the same call twice from the same state: identical bits everywhere
    a, b = native(p, g, m, v, warm_state(), clip, runs), native(p, g, m, v, warm_state(), clip, runs)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:4], b[:4]))
    assert a[3][ostep.COEF] < 1.0
    # max_norm above the norm: coef is exactly 1 and the bits equal the unclipped call
    loose = native(p, g, m, v, warm_state(), ostep.Hyper(max_norm=1e6, **HYPER), runs)
    plain = native(p, g, m, v, warm_state(), ostep.Hyper(max_norm=None, guard=False, **HYPER), runs)
    assert loose[3][ostep.COEF] == 1.0 and plain[3][ostep.GNORM] == 0.0 and loose[3][ostep.GNORM] > 0.0
    assert all(x.tobytes() == y.tobytes() for x, y in zip(loose[:3], plain[:3]))
    # a zero gradient: gnorm 0, coef 1, no NaN anywhere
    zero = native(p, np.zeros_like(g), np.zeros_like(m), np.zeros_like(v), ostep.initial_state(1e-2), clip, runs)
    assert zero[3][ostep.GNORM] == 0.0 and zero[3][ostep.COEF] == 1.0
    assert all(np.isfinite(x).all() for x in zero[:4])
    # step_out: p untouched, p + step_out is the in-place result within one rounding of the dtype
    so = native(p, g, m, v, warm_state(), clip, runs, step_out=True)
    assert so[0].tobytes() == p.tobytes() and so[1].tobytes() == a[1].tobytes() and so[2].tobytes() == a[2].tobytes()
    assert (np.abs((p + so[4]) - a[0]) <= np.finfo(dtype).eps * np.abs(a[0])).all()


@pytest.mark.parametrize("bad", [np.inf, np.nan])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_non_finite_gradient_skips_the_step(dtype, bad):
    n = 257
    p, g, m, v = operands(n, dtype, 8)
    runs, hyper = halves(n), ostep.Hyper(max_norm=1.0, **HYPER)
    gb = g.copy()
    gb[200] = bad
    m0, v0 = np.zeros_like(m), np.zeros_like(v)
    got = native(p, gb, m0, v0, ostep.initial_state(1e-2), hyper, runs)
    assert got[0].tobytes() == p.tobytes() and got[1].tobytes() == m0.tobytes() and got[2].tobytes() == v0.tobytes()
    rec = got[3]
    assert rec[ostep.SKIPPED] == 1 and rec[ostep.SKIP] == 1 and rec[ostep.T] == 0
    assert rec[ostep.B1_POW] == 1.0 and rec[ostep.B2_POW] == 1.0
    so = native(p, gb, m0, v0, ostep.initial_state(1e-2), hyper, runs, step_out=True)
    assert so[0].tobytes() == p.tobytes() and not so[4].any()                  # (step_out was zero and stays untouched)
    # the NEXT finite step, from the record the skipped one left, is the oracle's FIRST step
    nxt = native(p, g, m0, v0, rec, hyper, runs)
    state = oo.new_state([p[:n // 2], p[n // 2:]])
    want = np.concatenate(oo.adamw_step([p[:n // 2], p[n // 2:]], [g[:n // 2], g[n // 2:]], state, [True, False], lr=1e-2, wd=0.1,
                                        max_norm=1.0))
    np.testing.assert_allclose(nxt[0].astype(np.float64), want, rtol=0, atol=su.tol(dtype) * np.abs(want).max())
    assert nxt[3][ostep.T] == 1 and nxt[3][ostep.SKIPPED] == 1 and nxt[3][ostep.SKIP] == 0
    # without the guard nothing is skipped (and nothing is promised about the values)
    loose = native(p, gb, m0, v0, ostep.initial_state(1e-2), ostep.Hyper(max_norm=None, guard=False, **HYPER), runs)
    assert loose[3][ostep.T] == 1 and loose[3][ostep.SKIP] == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_scale_is_a_stand_alone_clip(dtype):
    lib = _lib.get()
    for n, unaligned in ((5, False), (1025, False), (1025, True)):
        g = oo.gradients(np.random.RandomState(n), (n,)).astype(dtype)
        gd = dsu.dev(g, dtype, unaligned)
        rec = tn.asarray(ostep.initial_state(0.0), dtype=np.float64)
        ws = tn.empty((ostep.grid(n),), np.float64)
        for max_norm in (0.5, 1e6):
            lib.ostep_sumsq(gd._ptr, n, ws._ptr, ws.nbytes, gd._code())
            lib.ostep_begin(rec._ptr, ws._ptr, n, max_norm, 1, 1.0, 1.0, ostep.SCHED_CONST, 0.0, 0.0, 0, 0)
            lib.ostep_scale(gd._ptr, n, rec._ptr, gd._code())
            st = np.asarray(rec)
            want = g * dtype(ostep.clip_coef(float(st[ostep.GNORM]), max_norm))
            assert np.asarray(gd).tobytes() == want.tobytes()
            g = want


def test_native_and_composed_routes_agree():
    """AdamW(fused=True) and AdamW(fused=False) through Model.step on the block net, one non-finite step included."""
    for dtype in DTYPES:
        opt_kw, _ = su.hyper_kwargs()
        models = []
        for fused in (True, False):
            opt = AdamW(fused=fused, **opt_kw)
            model, xshape = su.make_model("block", opt, dtype)
            rs = np.random.RandomState(21)
            for s in range(4):
                grads = su.draw_grads(model, rs, dtype)
                if s == 1:
                    grads[2].flat[1] = np.inf
                su.backward_then_inject(model, xshape, grads, dtype, rs, real_backward=(s == 0))
                model.step()
            models.append((model, opt))
        (a, oa), (b, ob) = models
        assert oa.route == "native" and ob.route == "composed"
        su.assert_params(a, su.host_params(b), dtype, "native vs composed %s" % np.dtype(dtype).name)
        sa, sb = oa.state(), ob.state()
        assert sa["t"] == sb["t"] == 3 and sa["skipped"] == sb["skipped"] == 1
        np.testing.assert_allclose(sa["lr"], sb["lr"], rtol=1e-12)
        np.testing.assert_allclose(sa["gnorm"], sb["gnorm"], rtol=1e-6 if dtype == np.float32 else 1e-12)


def test_a_skipped_step_on_the_compute_step_route_leaves_the_parameters():
    """AdamW natively through Model.step WITHOUT an arena (compute_step, the step_out form): the update launch writes nothing
    on a skipped step, so the step the model adds must be zeros, not whatever the recycled buffer held."""
    for dtype in DTYPES:
        opt_kw, _ = su.hyper_kwargs()
        opt = AdamW(**opt_kw)
        model, xshape = su.make_model("block", opt, dtype, use_arena=False)
        rs = np.random.RandomState(23)
        for s in range(2):                                         # good steps: state exists, freed step buffers sit in the cache
            su.backward_then_inject(model, xshape, su.draw_grads(model, rs, dtype), dtype, rs, real_backward=(s == 0))
            model.step()
        assert opt.route == "native" and model._grad_arena is None
        before, st0 = su.param_bits(model), opt.state()
        m0, v0 = np.asarray(opt._m).tobytes(), np.asarray(opt._v).tobytes()
        for bad in (np.inf, np.nan):
            grads = su.draw_grads(model, rs, dtype)
            grads[2].flat[1] = bad
            su.backward_then_inject(model, xshape, grads, dtype, rs, real_backward=False)
            model.step()
            assert su.param_bits(model) == before
            assert np.asarray(opt._m).tobytes() == m0 and np.asarray(opt._v).tobytes() == v0
        st = opt.state()
        assert st["skipped"] == 2 and st["skip"] == 1 and st["t"] == st0["t"] == 2
        assert st["b1_pow"] == st0["b1_pow"] and st["b2_pow"] == st0["b2_pow"]
        su.backward_then_inject(model, xshape, su.draw_grads(model, rs, dtype), dtype, rs, real_backward=False)
        model.step()
        assert su.param_bits(model) != before and opt.state()["t"] == 3 and opt.state()["skip"] == 0


def test_a_captured_step_follows_the_schedule():
    """The test the feature exists for: the WHOLE step — forward, loss, backward, norm, clip, decay, schedule, update — captured
    once and replayed must land on the bits of eager steps.  A learning rate (or a step count, or a clip factor) baked into the
    graph fails here."""
    from tinynn_autograd_amd.core.layers import TransformerBlock
    rs = np.random.RandomState(31)
    xs = [rs.standard_normal((2, 4, 8)).astype(np.float32) for _ in range(8)]
    ys = [rs.standard_normal((2, 4, 8)).astype(np.float32) for _ in range(8)]
    sched = ostep.Cosine(3, 8)

    def build():
        np.random.seed(12)
        net = Net([TransformerBlock(2, num_in=8)])
        return Model(net=net, loss=SquaredErrorLoss(), optimizer=AdamW(lr=1e-2, weight_decay=0.1, max_norm=1e-3, schedule=sched))

    captured_model, eager_model = build(), build()
    assert su.param_bits(captured_model) == su.param_bits(eager_model)
    x_stage, y_stage = Tensor(xs[0].copy()), Tensor(ys[0].copy())

    def step_of(model, x, y):
        def step():
            model.zero_grad()
            loss = model.loss.loss(model.forward(x), y)
            loss.backward()
            model.step()
            return loss
        return step

    step = step_of(captured_model, x_stage, y_stage)
    def feed(i):
        x_stage.values[...] = tn.asarray(xs[i])
        y_stage.values[...] = tn.asarray(ys[i])

    # warm-up 2: real steps on batches 0 and 1 (tn.capture calls the function itself, so the staging is done by hand)
    feed(0); step()
    feed(1); step()
    replay = tn.capture(step, warmup=0)
    for i in range(2, 8):
        feed(i)
        replay()
    for i in range(8):
        step_of(eager_model, Tensor(xs[i]), Tensor(ys[i]))()
    st, se = captured_model.optimizer.state(), eager_model.optimizer.state()
    assert st["t"] == 8 and se["t"] == 8 and st["skipped"] == 0
    assert abs(st["lr"] - sched.value(8, 1e-2)) <= 1e-12 * 1e-2     # the schedule at 8 (= total: min_lr), not step 1's or 3's
    assert sched.value(8, 1e-2) == 0.0 and sched.value(2, 1e-2) > 0.0
    assert st["coef"] < 1.0                                        # max_norm was small enough to clip
    assert st == se
    assert su.param_bits(captured_model) == su.param_bits(eager_model)
    # the composed route says so instead of capturing garbage
    slow = Model(net=Net([Dense(3, num_in=4)]), loss=SquaredErrorLoss(), optimizer=AdamW(fused=False))
    xs4, ys4 = Tensor(np.ones((2, 4), np.float32)), Tensor(np.ones((2, 3), np.float32))
    slow_step = step_of(slow, xs4, ys4)
    slow_step()
    with pytest.raises(RuntimeError, match="graph capture"):
        tn.capture(slow_step, warmup=0)


def test_clip_grad_norm_in_front_of_adam_matches_the_composed_route(monkeypatch):
    """MNIST-shaped net at 16 rows: the native clip (arena, three launches, nothing read back) against the composed one
    (squares summed with DeviceArray arithmetic, norm read back), Adam behind both.  float32: RTOL of the max-norm."""
    rs = np.random.RandomState(41)
    x = (rs.rand(16, 784) * (rs.rand(16, 784) < 0.19)).astype(np.float32)
    y = np.eye(10)[rs.randint(0, 10, 16)].astype(np.float32)

    def build():
        np.random.seed(5)
        net = Net([Dense(256, num_in=784), ReLU(), Dense(128, num_in=256), ReLU(), Dense(10, num_in=128)])
        return Model(net=net, loss=SoftmaxCrossEntropyLoss(), optimizer=Adam(lr=1e-3))

    # both models run the same backward and the same Adam; only the clip differs.  The composed one is what a library
    # without the entry points gets.
    native_model, composed_model = build(), build()
    lib = _lib.get()
    norms = []
    for s in range(3):
        for model in (native_model, composed_model):
            model.zero_grad()
            model.loss.loss(model.forward(Tensor(x)), Tensor(y)).backward()
            monkeypatch.setattr(lib, "has_ostep", model is native_model)
            kept = model.clip_grad_norm(0.05)
            monkeypatch.setattr(lib, "has_ostep", True)
            norms.append(float(kept))
            if model is native_model:                              # the returned scalar is the caller's: a later call leaves it
                model.clip_grad_norm(1e6)
                assert float(kept) == norms[-1] and float(np.asarray(model._clip_rec)[ostep.GNORM]) < norms[-1]
            assert model._pending_first is None
            model.step()
        print("step %d: norm native %.9g composed %.9g" % (s + 1, norms[-2], norms[-1]))
        np.testing.assert_allclose(norms[-2], norms[-1], rtol=su.RTOL)
        assert norms[-1] > 0.05
    assert native_model._clip_rec is not None and composed_model._clip_rec is None
    for p, q in zip(native_model._live_params(), composed_model._live_params()):
        want = np.asarray(q.values)
        np.testing.assert_allclose(np.asarray(p.values), want, rtol=0, atol=su.RTOL * np.abs(want).max())
