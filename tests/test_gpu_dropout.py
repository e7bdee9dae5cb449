"""csrc/tnn_dropout.hip on the MI355X against the planner's numpy generator (tinynn-autograd_amd/dropout.py), BIT FOR BIT, and
against the composed route.  Shapes are the smallest at which the kernel can still go wrong: sizes around one Philox block, one
wave and one workgroup, one size that makes every launch walk its grid stride once and end in a ragged block, stream offsets
that break the 4-element block alignment, a slice across the 32-bit carry of the block counter, element-aligned base pointers
for each operand, the in-place forms, and the state / ticket rules."""

import numpy as np
import pytest

import dropout_support as dsu
import tinynn_autograd_amd as tn
from tinynn_autograd_amd import _lib, dropout as dp, rng
from tinynn_autograd_amd import device_array as da
from tinynn_autograd_amd.core import ops
from tinynn_autograd_amd.core.tensor import Tensor

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025]
STRIDE_N = 4 * dp.THREADS * dp.MAX_BLOCKS + 5        # every lane of a full grid takes one block, then 5 elements remain
FIRSTS = [0, 1, 3]
CARRY_FIRST = 2 ** 34 - 8                            # stream blocks 2^32 - 2 .. 2^32 + 1
SEED, CALLS = 1234, 5


@pytest.fixture(autouse=True)
def _switches():
    yield
    da.DROPOUT_ROUTE = None


def gen_at(seed=SEED, calls=CALLS):
    return rng.Generator().set_state(seed, calls)


def check_call(x, res, p, first, dtype, unaligned=(False, False, False), route="native", what=""):
    """One forward (and backward) call from the state (SEED, CALLS) against the planner's reference, bit for bit."""
    g = gen_at()
    xd = dsu.dev(x, dtype, unaligned[0])
    rd = None if res is None else dsu.dev(res, dtype, unaligned[1])
    out = dsu.dev(np.zeros_like(x), dtype, True) if unaligned[2] else None
    y, mask = da.dropout(xd, p, rd, generator=g, route=route, first=first, out=out)
    want = dp.reference(x, SEED, CALLS, p, residual=res, first=first)
    np.testing.assert_array_equal(dsu.bits(y), dsu.bits(want), err_msg=what)
    dx = da.dropout_bwd(xd, mask)                    # (x again as the incoming gradient)
    np.testing.assert_array_equal(dsu.bits(dx), dsu.bits(dp.reference(x, SEED, CALLS, p, first=first)), err_msg=what + " bwd")
    return np.asarray(y)


def test_backend_and_entry_points():
    lib = _lib.get()
    assert tn.backend_name() == "hip-gfx950" and lib.has_dropout
    assert dp.plan_dropout((4, 8), 0.5, np.float32, native=lib.has_dropout).route == "native"
    g = rng.Generator(3)
    assert g.state() == (3, 0)
    g.device_state()
    assert g.state() == (3, 0)
    g.set_state(2 ** 63 + 5, 2 ** 64 - 1)
    assert g.state() == (2 ** 63 + 5, 2 ** 64 - 1)
    g.uniform((1,))
    assert g.state() == (2 ** 63 + 5, 0)             # calls is a uint64 and wraps


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_sizes_and_offsets_on_both_routes(dtype, p):
    for n in SIZES:
        x, res = dsu.values(n, dtype, n), dsu.values(n, dtype, n + 7)
        for first in FIRSTS:
            what = "n %d first %d" % (n, first)
            plain = check_call(x, None, p, first, dtype, what=what)
            fused = check_call(x, res, p, first, dtype, what=what + " residual")
            np.testing.assert_array_equal(check_call(x, None, p, first, dtype, route="composed", what=what + " composed"), plain)
            np.testing.assert_array_equal(check_call(x, res, p, first, dtype, route="composed", what=what + " composed"), fused)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_grid_stride_and_ragged_tail(dtype):
    """More blocks than MAX_BLOCKS workgroups hold: the wide path (first 0) and the element path (first 1) both walk."""
    x, res = dsu.values(STRIDE_N, dtype, 1), dsu.values(STRIDE_N, dtype, 2)
    assert dp.plan_dropout(x.shape, 0.5, dtype).grid() == dp.MAX_BLOCKS
    assert dp.plan_dropout((STRIDE_N - 5,), 0.5, dtype).grid() == dp.MAX_BLOCKS
    check_call(x, res, 0.5, 0, dtype, what="stride wide")
    check_call(x, None, 0.1, 1, dtype, what="stride element")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_slice_across_the_32_bit_carry_of_the_block_counter(dtype):
    words = dp.stream_words(7, 3, CARRY_FIRST, 16)
    assert words[:4].tolist() == [2624505957, 2176703114, 2516343209, 1286663913]
    g = gen_at(7, 3)
    u = np.asarray(g.uniform((16,), dtype, first=CARRY_FIRST))
    np.testing.assert_array_equal(dsu.bits(u), dsu.bits(dp.uniform(7, 3, CARRY_FIRST, 16, dtype)))
    np.testing.assert_array_equal((u * 2.0 ** 24).astype(np.uint32), words >> 8)
    x = dsu.values(16, dtype)
    for first in (CARRY_FIRST, CARRY_FIRST + 1):
        y, _ = da.dropout(dsu.dev(x, dtype), 0.5, generator=gen_at(7, 3), first=first)
        np.testing.assert_array_equal(dsu.bits(y), dsu.bits(dp.reference(x, 7, 3, 0.5, first=first)))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_element_aligned_base_pointers(dtype, which):
    """x, the residual and y in turn one element past a 16-byte boundary: the element path, the same draws."""
    unaligned = tuple(i == which for i in range(3))
    for n in (5, 257, 1025):
        x, res = dsu.values(n, dtype, n), dsu.values(n, dtype, n + 1)
        check_call(x, res, 0.5, 0, dtype, unaligned=unaligned, what="n %d unaligned %s" % (n, unaligned))
        if which != 1:
            check_call(x, None, 0.1, 0, dtype, unaligned=unaligned, what="n %d unaligned %s plain" % (n, unaligned))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_in_place_forms(dtype):
    n = 1025
    x, res = dsu.values(n, dtype, 1), dsu.values(n, dtype, 2)
    want = dp.reference(x, SEED, CALLS, 0.5, residual=res)
    xd, rd = dsu.dev(x, dtype), dsu.dev(res, dtype)
    y, mask = da.dropout(xd, 0.5, rd, generator=gen_at(), out=xd)              # y aliases x
    assert y is xd
    np.testing.assert_array_equal(dsu.bits(xd), dsu.bits(want))
    np.testing.assert_array_equal(dsu.bits(rd), dsu.bits(res))
    xd = dsu.dev(x, dtype)
    y, _ = da.dropout(xd, 0.5, rd, generator=gen_at(), out=rd)                 # y aliases the residual
    assert y is rd
    np.testing.assert_array_equal(dsu.bits(rd), dsu.bits(want))
    np.testing.assert_array_equal(dsu.bits(xd), dsu.bits(x))
    xd = dsu.dev(x, dtype)
    y, _ = da.dropout(xd, 0.5, generator=gen_at(), out=xd)                     # the plain form in place
    np.testing.assert_array_equal(dsu.bits(xd), dsu.bits(dp.reference(x, SEED, CALLS, 0.5)))
    dy = dsu.dev(res, dtype)
    dx = da.dropout_bwd(dy, mask, dx_out=dy)                                   # dx aliases dy
    assert dx is dy
    np.testing.assert_array_equal(dsu.bits(dy), dsu.bits(dp.reference(res, SEED, CALLS, 0.5)))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_dropped_inf_and_nan_give_positive_zero(dtype):
    n = 64
    keep = dp.keep_mask(SEED, CALLS, 0, n, dp.threshold_of(0.5))
    assert 8 < keep.sum() < n - 8
    x = dsu.values(n, dtype)
    x[::3], x[1::3] = np.inf, np.nan
    x[2::6] = -np.inf
    y, mask = da.dropout(dsu.dev(x, dtype), 0.5, generator=gen_at())
    y = np.asarray(y)
    zero = np.zeros(1, dtype)
    assert (dsu.bits(y[~keep]) == dsu.bits(zero)[0]).all()
    np.testing.assert_array_equal(dsu.bits(y[keep]), dsu.bits((x * dtype(2.0))[keep]))
    dx = np.asarray(da.dropout_bwd(dsu.dev(x, dtype), mask))
    assert (dsu.bits(dx[~keep]) == dsu.bits(zero)[0]).all()
    res = dsu.values(n, dtype, 3)
    y, _ = da.dropout(dsu.dev(x, dtype), 0.5, dsu.dev(res, dtype), generator=gen_at())
    np.testing.assert_array_equal(dsu.bits(np.asarray(y)[~keep]), dsu.bits(res[~keep]))


def test_zero_rate_adds_no_launch(monkeypatch):
    x = Tensor(dsu.values(37, np.float32), requires_grad=True)
    r = Tensor(dsu.values(37, np.float32, 1), requires_grad=True)
    g = gen_at()
    tn.synchronize()
    seen = dsu.count_calls(monkeypatch)
    assert ops.dropout_(x, 0.0, generator=g) is x
    assert seen == []
    _ = r + x
    plain_add = list(seen)
    del seen[:]
    y = ops.dropout_(x, 0.0, r, generator=g)
    assert seen == plain_add and not any("dropout" in s or "rng" in s for s in seen)
    monkeypatch.undo()
    np.testing.assert_array_equal(dsu.bits(y.values), dsu.bits(np.asarray(r.values) + np.asarray(x.values)))
    assert g.state() == (SEED, CALLS)


def test_state_advances_once_per_call_and_seeds_reproduce():
    g, h = rng.Generator(77), rng.Generator(77)
    x = dsu.dev(dsu.values(100, np.float32), np.float32)
    outs = [np.asarray(da.dropout(x, 0.5, generator=g)[0]) for _ in range(4)]
    assert g.state() == (77, 4)
    for k, y in enumerate(outs):
        np.testing.assert_array_equal(dsu.bits(y), dsu.bits(dp.reference(np.asarray(x), 77, k, 0.5)))
    assert not np.array_equal(outs[0], outs[1])
    for y in outs:
        np.testing.assert_array_equal(np.asarray(da.dropout(x, 0.5, generator=h)[0]), y)
    g.manual_seed(77)
    assert g.state() == (77, 0)
    np.testing.assert_array_equal(np.asarray(da.dropout(x, 0.5, generator=g)[0]), outs[0])
    da.DROPOUT_ROUTE = "composed"                                              # the composed route leaves the same state behind
    np.testing.assert_array_equal(np.asarray(da.dropout(x, 0.5, generator=g)[0]), outs[1])
    assert g.state() == (77, 2)
    da.DROPOUT_ROUTE = None
    np.testing.assert_array_equal(np.asarray(da.dropout(x, 0.5, generator=g)[0]), outs[2])


def test_backward_uses_its_own_forwards_ticket():
    g = gen_at()
    x = Tensor(dsu.values(300, np.float32), requires_grad=True)
    r = Tensor(dsu.values(300, np.float32, 1), requires_grad=True)
    y = ops.dropout_(x, 0.5, r, generator=g)
    for _ in range(2):                                                         # two further draws move the state on
        ops.dropout_(x, 0.5, generator=g)
    dy = dsu.values(300, np.float32, 2)
    y.backward(dy)
    np.testing.assert_array_equal(dsu.bits(x.grad), dsu.bits(dp.reference(dy, SEED, CALLS, 0.5)))
    np.testing.assert_array_equal(dsu.bits(r.grad), dsu.bits(dy))
    assert g.state() == (SEED, CALLS + 3)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_uniform_fill(dtype):
    g = gen_at()
    for k, n in enumerate([1, 5, 1025]):
        u = np.asarray(g.uniform((n,), dtype))
        assert u.dtype == dtype and (u >= 0).all() and (u < 1).all()
        np.testing.assert_array_equal(dsu.bits(u), dsu.bits(dp.uniform(SEED, CALLS + k, 0, n, dtype)))
    assert g.uniform((3, 0, 2), dtype).shape == (3, 0, 2) and g.state() == (SEED, CALLS + 4)


def test_generate_draws_u_on_the_device():
    import decode_oracle as do
    import decode_support as ds
    from tinynn_autograd_amd import generation as gen
    net = ds.lm_net(ds.load_golden(), True, np.float32)
    prompt = do.lm_prompt()
    g = gen_at()
    a = gen.generate(net, prompt, do.LM_NEW, temperature=0.9, top_k=5, generator=g)
    u = dp.uniform(SEED, CALLS, 0, do.LM_NEW * prompt.shape[0], np.float32).reshape(do.LM_NEW, prompt.shape[0])
    assert np.array_equal(a, gen.generate(net, prompt, do.LM_NEW, temperature=0.9, top_k=5, u=u))
    assert g.state() == (SEED, CALLS + 1) and net.get_phase() == "TRAIN"
    assert not np.array_equal(a, gen.generate(net, prompt, do.LM_NEW, temperature=0.9, top_k=5, generator=g))
    with pytest.raises(ValueError, match="excludes"):
        gen.generate(net, prompt, 2, u=u[:2], generator=g)


def test_block_with_dropout_replayed_from_a_captured_graph():
    """Embedding(dropout) -> TransformerBlock(dropout) -> loss -> backward, captured: every replay draws anew (the state lives on
    the device and the tickets are the replay's own), equals the eager run from the same state bit for bit, and advances the
    state by the same count."""
    from tinynn_autograd_amd.core.layers import Embedding, TransformerBlock
    from tinynn_autograd_amd.core.losses import SquaredErrorLoss
    from tinynn_autograd_amd.core.nn import Net
    B, T, E, V = 3, 5, 16, 11

    def build():
        np.random.seed(3)
        g = rng.Generator(11)
        net = Net([Embedding(V, E, max_len=T, dropout=0.25, generator=g),
                   TransformerBlock(2, hidden=24, num_in=E, causal=True, dropout=0.1, generator=g)])
        rs = np.random.RandomState(4)
        ids, y = tn.asarray(rs.randint(0, V, (B, T))), Tensor(rs.standard_normal((B, T, E)).astype(np.float32))
        state = {}

        def fn():
            for layer in net.layers:
                for t in layer.params.values():
                    t.zero_grad()
            out = net.forward(Tensor(ids))
            loss = SquaredErrorLoss().loss(out, y)
            loss.backward()
            state["out"], state["loss"] = out.values, loss.values
            return loss.values

        def read():
            return (dsu.bits(state["loss"]).copy(), dsu.bits(state["out"]).copy(),
                    dsu.bits(net.layers[0].params["tok"].grad).copy(), dsu.bits(net.layers[1].params["fc2.w"].grad).copy())
        return g, fn, read

    g, fn, read = build()
    eager, states = [], []
    for _ in range(4):
        fn()
        eager.append(read())
        states.append(g.state())
    per_call = states[0][1]
    assert per_call == 3 and [s[1] for s in states] == [per_call * (k + 1) for k in range(4)]

    g, fn, read = build()
    fn()                                                                       # the first eager run: state (11, per_call)
    captured = tn.capture(fn, warmup=0)
    assert g.state() == (11, per_call)                                         # recording draws nothing
    for k in range(1, 4):
        captured()
        got = read()
        for a, b in zip(got, eager[k]):
            np.testing.assert_array_equal(a, b)
        assert g.state() == (11, per_call * (k + 1))
    assert not np.array_equal(eager[1][1], eager[2][1]) and not np.array_equal(eager[2][1], eager[3][1])
    assert not np.array_equal(eager[1][1], eager[3][1])
