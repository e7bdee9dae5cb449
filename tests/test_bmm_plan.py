"""batching.py, the host planner of N-d `a @ b`, against numpy on seeded random operand pairs (no device involved): result
shapes, numpy's refusals, plans replayed in numpy by their own strides, and the routes."""

import os

import numpy as np
import pytest

from tinynn_autograd_amd import batching as B


def _random_view(rs, shape):
    """A float64 array of `shape` holding small integers, as a random view: dense, strided along any axis, with permuted
    axes (a transposed matrix, transposed batch axes), reversed, or broadcast along an extent-1 axis."""
    kind = rs.randint(0, 6)
    nd = len(shape)
    if kind == 0 or nd == 0:
        return rs.randint(-3, 4, size=shape).astype(np.float64)
    if kind == 1:                                         # every other element along one axis
        ax = rs.randint(nd)
        big = list(shape)
        big[ax] = big[ax] * 2 + 1
        sl = [slice(None)] * nd
        sl[ax] = slice(rs.randint(0, 2), None, 2)
        return rs.randint(-3, 4, size=big).astype(np.float64)[tuple(sl)][tuple(slice(0, s) for s in shape)]
    if kind == 2 and nd >= 2:                             # the last two axes exchanged in memory
        base = rs.randint(-3, 4, size=shape[:-2] + (shape[-1], shape[-2])).astype(np.float64)
        return np.swapaxes(base, -1, -2)
    if kind == 3 and nd >= 3:                             # a permutation of all axes
        perm = rs.permutation(nd)
        base = rs.randint(-3, 4, size=[shape[i] for i in np.argsort(perm)]).astype(np.float64)
        return base.transpose(perm)
    if kind == 4:                                         # rows of a wider buffer (row stride > row length)
        big = list(shape)
        big[-1] += 3
        return rs.randint(-3, 4, size=big).astype(np.float64)[..., 1:1 + shape[-1]]
    ax = rs.randint(nd)                                   # reversed along one axis (negative stride)
    sl = [slice(None)] * nd
    sl[ax] = slice(None, None, -1)
    return rs.randint(-3, 4, size=shape).astype(np.float64)[tuple(sl)]


def _random_pair(rs):
    """Shapes of a matmul operand pair, 1-D to 5-D, with broadcast, extent-0 and extent-1 dimensions; about one in eight
    is invalid (core mismatch or batch dimensions that do not broadcast)."""
    dim = lambda: int(rs.choice([0, 1, 1, 2, 3, 4, 5, 7]))           # noqa: E731
    M, K, N = dim(), dim(), dim()
    na, nb = rs.randint(1, 6), rs.randint(1, 6)
    batch = [int(rs.choice([0, 1, 1, 2, 3, 4])) for _ in range(3)]
    a_batch = [1 if rs.rand() < 0.3 else d for d in batch][3 - max(na - 2, 0):]
    b_batch = [1 if rs.rand() < 0.3 else d for d in batch][3 - max(nb - 2, 0):]
    a = tuple(a_batch) + ((M, K) if na > 1 else (K,))
    b = tuple(b_batch) + ((K, N) if nb > 1 else (K,))
    bad = rs.rand()
    if bad < 0.06:
        b = b[:-2] + (K + 1, N) if nb > 1 else (K + 1,)
    elif bad < 0.12 and na > 2 and nb > 2:
        a = (a[0] + 2,) + a[1:]
    return a, b


def _flat(view):
    """(flat buffer, offset of the view's first element, element strides) of a numpy view"""
    base = view
    while base.base is not None:
        base = base.base
    flat = base.reshape(-1)
    off = (view.__array_interface__["data"][0] - base.__array_interface__["data"][0]) // view.itemsize
    return flat, off, tuple(s // view.itemsize for s in view.strides)


def replay(plan, a, b):
    """Execute a plan in numpy exactly as the device would: element by element through the plan's own strides."""
    if plan.copy_a:
        a = np.ascontiguousarray(a)
    if plan.copy_b:
        b = np.ascontiguousarray(b)
    fa, oa0, _ = _flat(a)
    fb, ob0, _ = _flat(b)
    M, N, K = plan.M, plan.N, plan.K
    a_rs, a_cs = (1, plan.lda) if plan.ta else (plan.lda, 1)
    b_rs, b_cs = (1, plan.ldb) if plan.tb else (plan.ldb, 1)
    m, k, n = np.arange(M), np.arange(K), np.arange(N)
    out = np.zeros((max(plan.batch_size, 0) if plan.route != "gemm2d" else 1, M, N))
    offs = B.batch_offsets(plan)
    assert len(offs) == out.shape[0]
    if fa.size == 0 or fb.size == 0 or K == 0:
        return out.reshape(plan.out_shape)
    for i, (oa, ob) in enumerate(offs):
        am = fa[oa0 + oa + m[:, None] * a_rs + k[None, :] * a_cs] if M else np.zeros((0, K))
        bm = fb[ob0 + ob + k[:, None] * b_rs + n[None, :] * b_cs] if N else np.zeros((K, 0))
        out[i] = am @ bm
    return out.reshape(plan.out_shape)


def test_random_pairs_against_numpy():
    rs = np.random.RandomState(20260101)
    valid = invalid = 0
    routes = {"gemm2d": 0, "batched": 0, "loop": 0}
    copies = 0
    for _ in range(700):
        sa, sb = _random_pair(rs)
        a, b = _random_view(rs, sa), _random_view(rs, sb)
        assert a.shape == sa and b.shape == sb
        try:
            want = np.matmul(a, b)
        except ValueError:
            with pytest.raises(ValueError):
                B.result_shape(sa, sb)
            with pytest.raises(ValueError):
                B.plan_matmul(sa, sb)
            invalid += 1
            continue
        valid += 1
        assert B.result_shape(sa, sb) == want.shape
        native = bool(rs.randint(2))
        plan = B.plan_matmul(sa, sb, _flat(a)[2], _flat(b)[2], native=native)
        assert plan.out_shape == want.shape, (sa, sb, plan)
        assert len(plan.batch) == len(plan.a_bstrides) == len(plan.b_bstrides)
        assert all(n != 1 for n in plan.batch)
        assert native or plan.route != "batched"
        assert plan.route != "batched" or len(plan.batch) <= B.MAX_BATCH_DIMS
        got = replay(plan, a, b)
        np.testing.assert_array_equal(got, want, err_msg="%s @ %s: %r" % (sa, sb, plan))
        routes[plan.route] += 1
        copies += plan.copy_a + plan.copy_b
        # the gemm2d collapses are chosen exactly for: both operands at most 2-D; a dense stack times one matrix / vector
        a_dense = a.flags.c_contiguous or plan.copy_a
        assert (plan.route == "gemm2d") == ((a.ndim <= 2 and b.ndim <= 2) or (b.ndim <= 2 and a_dense)), (sa, sb, plan)
    assert valid >= 300 and invalid >= 20
    assert min(routes.values()) > 0 and copies > 0


def test_core_mismatch_message_is_the_2d_one():
    with pytest.raises(ValueError, match=r"mismatch in its core dimension 0 \(size 4 is different from 5\)"):
        B.plan_matmul((2, 3, 5), (2, 4, 6))
    with pytest.raises(ValueError, match="broadcast"):
        B.plan_matmul((2, 3, 5), (3, 5, 6))
    with pytest.raises(ValueError, match="not have enough dimensions"):
        B.plan_matmul((), (3,))


def test_2d_call_is_todays():
    """Both operands 2-D: one tnn_gemm with the lazy transposes as flags and the stored row length as row stride — the
    arguments device_array.matmul has always passed."""
    for a_t in (False, True):
        for b_t in (False, True):
            p = B.plan_matmul((6, 5), (5, 3), a_t=a_t, b_t=b_t)
            assert p.route == "gemm2d" and not p.copy_a and not p.copy_b
            assert (p.ta, p.tb, p.M, p.N, p.K) == (int(a_t), int(b_t), 6, 3, 5)
            assert p.lda == (6 if a_t else 5) and p.ldb == (5 if b_t else 3)
            assert p.batch == () and p.out_shape == (6, 3)
    p = B.plan_matmul((5,), (5, 3))
    assert p.route == "gemm2d" and (p.M, p.N, p.K, p.lda, p.ldb, p.out_shape) == (1, 3, 5, 5, 3, (3,))
    p = B.plan_matmul((6, 5), (5,))
    assert p.route == "gemm2d" and (p.M, p.N, p.K, p.lda, p.ldb, p.out_shape) == (6, 1, 5, 5, 1, (6,))


def test_named_collapses_and_broadcasts():
    p = B.plan_matmul((3, 200, 70), (70, 30))                     # Dense form: one (600, 70) @ (70, 30)
    assert p.route == "gemm2d" and (p.M, p.N, p.K, p.lda, p.ldb) == (600, 30, 70, 70, 30) and p.batch == ()
    p = B.plan_matmul((2, 4, 10, 8), (8, 6), b_t=True)            # ... with a lazy-transposed weight
    assert p.route == "gemm2d" and (p.M, p.tb, p.ldb) == (80, 1, 8)
    p = B.plan_matmul((2, 4, 10, 8), (2, 4, 8, 10))               # dense stacks: the batch dimensions merge into one
    assert p.route == "batched" and p.batch == (8,) and p.a_bstrides == (80,) and p.b_bstrides == (80,)
    p = B.plan_matmul((2, 1, 3, 5), (1, 4, 5, 2))                 # broadcast: stride 0, nothing materialised
    assert p.route == "batched" and p.batch == (2, 4) and p.a_bstrides == (15, 0) and p.b_bstrides == (0, 10)
    p = B.plan_matmul((3, 5), (4, 5, 2))
    assert p.route == "batched" and p.batch == (4,) and p.a_bstrides == (0,) and p.b_bstrides == (10,)
    p = B.plan_matmul((4, 3, 5), (4, 2, 5), swap_b=True)          # the vjp's swap(B): a flag, not a copy
    assert p.route == "batched" and (p.tb, p.ldb, p.N, p.K) == (1, 5, 2, 5) and not p.copy_b
    p = B.plan_matmul((4, 3, 5), (4, 5, 2), native=False)         # the CPU test twin
    assert p.route == "loop" and len(B.batch_offsets(p)) == 4
    p = B.plan_matmul((2, 2048, 2048), (2, 2048, 2048))           # few large matrices: the 2-D kernel, per element
    assert p.route == "loop"
    p = B.plan_matmul((1000, 4, 4), (1000, 4, 4))
    assert p.route == "batched" and p.batch == (1000,)


def test_is_numpy_only():
    src = open(os.path.join(os.path.dirname(B.__file__), "batching.py")).read()
    assert "_lib" not in src and "device_array" not in src
