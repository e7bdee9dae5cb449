"""Host planner of `a @ b` for N-d operands (numpy only, no device import): from the shapes and element strides of the two
operands to ONE plan — result shape by numpy's matmul rules, the broadcast batch shape collapsed to at most MAX_BATCH_DIMS
dimensions with one stride per operand (0 where that operand is broadcast, so it is never materialised), transpose flags
and row strides of the per-matrix product, and the route that executes it:

    gemm2d   the product is really one 2-D GEMM and goes to tnn_gemm without a copy: both operands at most 2-D (the path
             of the 1-D / 2-D `@`), or a dense [..., M, K] @ [K, N] -> (prod(...) * M, K) @ (K, N)
    batched  tnn_gemm_batched (csrc/tnn_bmm.hip), one launch for the whole batch
    loop     one tnn_gemm per batch element: large per-matrix products with few batch elements, where the 2-D kernel fills
             the device by itself — and everything that is not gemm2d when the native batched entry point is absent (the
             CPU test twin)

An operand is described by its LOGICAL shape and the element strides of that shape over its buffer (None: dense
row-major).  `t=True` says that a 2-D operand is held as the dense transpose of its logical shape (DeviceArray's lazy
`.T`); `swap=True` asks for the operand with its last two axes exchanged (the vjps' `swap(B)` / `swap(A)`), again by
stride.  A matrix whose strides no (trans, row stride) pair can express — neither axis contiguous, a negative or a zero
stride inside the matrix — is marked `copy_a` / `copy_b`: the caller makes that operand dense (logical order) first and
the plan's strides refer to the dense copy.
"""

import math

MAX_BATCH_DIMS = 4          # TNN_BMM_MAX_BATCH_DIMS

# `loop` from this many multiply-adds per matrix: the 2-D kernel's larger tiles and deeper pipeline then beat the batched
# kernel's 64 x 64 tiles, and the per-call host cost of the loop no longer matters (kernel table: measured with
# tools/probes/bmm_vs_loop.py — the batched launch wins 2.1x at 8 x 512^3 and loses 1.45x at 2 x 2048^3)
LOOP_MIN_MNK = 1024 * 1024 * 1024


class Plan(object):
    __slots__ = ("out_shape", "M", "N", "K", "batch", "a_bstrides", "b_bstrides", "ta", "tb", "lda", "ldb",
                 "copy_a", "copy_b", "route", "batch_size")

    def __repr__(self):
        return "Plan(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.__slots__)


def dense_strides(shape):
    st, acc = [], 1
    for s in reversed(shape):
        st.append(acc)
        acc *= int(s)
    return tuple(reversed(st))


def _matrix(rows, cols, rs, cs):
    """(trans, ld) of a [rows, cols] matrix with element strides (rs, cs), or None.  trans=0: stored rows of ld elements;
    trans=1: stored as the transpose ([cols, rows], rows of ld elements).  An empty matrix is never read."""
    if rows * cols == 0:
        return 0, max(cols, 1)
    if (cols <= 1 or cs == 1) and (rows <= 1 or rs >= max(cols, 1)):
        return 0, (rs if rows > 1 else max(cols, 1))
    if (rows <= 1 or rs == 1) and (cols <= 1 or cs >= max(rows, 1)):
        return 1, (cs if cols > 1 else max(rows, 1))
    return None


def _operand(shape, strides, t, swap):
    shape = tuple(int(s) for s in shape)
    if t:
        if len(shape) != 2:
            raise ValueError("a lazy transpose is a 2-D flag")
        stored = dense_strides((shape[1], shape[0])) if strides is None else tuple(strides)
        strides = (stored[1], stored[0])
    elif strides is None:
        strides = dense_strides(shape)
    strides = tuple(int(s) for s in strides)
    if len(strides) != len(shape):
        raise ValueError("strides do not match the shape")
    if swap:
        if len(shape) < 2:
            raise ValueError("swap needs a matrix")
        shape = shape[:-2] + (shape[-1], shape[-2])
        strides = strides[:-2] + (strides[-1], strides[-2])
    return shape, strides


def result_shape(a_shape, b_shape):
    """Shape of np.matmul on operands of these shapes (raises numpy's ValueErrors)."""
    return _shapes(tuple(int(s) for s in a_shape), tuple(int(s) for s in b_shape))[0]


def _shapes(a_shape, b_shape):
    if len(a_shape) == 0 or len(b_shape) == 0:
        raise ValueError("matmul: Input operand %d does not have enough dimensions (has 0, gufunc core with signature "
                         "(n?,k),(k,m?)->(n?,m?) requires 1)" % (0 if len(a_shape) == 0 else 1))
    a2 = a_shape if len(a_shape) > 1 else (1,) + a_shape
    b2 = b_shape if len(b_shape) > 1 else b_shape + (1,)
    M, K = a2[-2], a2[-1]
    K2, N = b2[-2], b2[-1]
    if K != K2:
        raise ValueError("matmul: Input operand 1 has a mismatch in its core dimension 0 "
                         "(size %d is different from %d)" % (K2, K))
    ab, bb = a2[:-2], b2[:-2]
    nb = max(len(ab), len(bb))
    pa, pb = (1,) * (nb - len(ab)) + ab, (1,) * (nb - len(bb)) + bb
    batch = []
    for x, y in zip(pa, pb):
        if x != y and x != 1 and y != 1:
            raise ValueError("operands could not be broadcast together with remapped shapes [original->remapped]: "
                             "%s and %s (batch dimensions %s and %s)" % (a_shape, b_shape, ab, bb))
        batch.append(y if x == 1 else x)
    batch = tuple(batch)
    out = batch + (() if len(a_shape) == 1 else (M,)) + (() if len(b_shape) == 1 else (N,))
    return out, batch, pa, pb, M, N, K


def _collapse(batch, sa, sb):
    """Drop extent-1 dimensions and merge neighbours that both operands walk with one stride."""
    dims = [(n, x, y) for n, x, y in zip(batch, sa, sb) if n != 1]
    out = []
    for n, x, y in dims:
        if out:
            pn, px, py = out[-1]
            if px == x * n and py == y * n:
                out[-1] = (pn * n, x, y)
                continue
        out.append((n, x, y))
    return tuple(d[0] for d in out), tuple(d[1] for d in out), tuple(d[2] for d in out)


def plan_matmul(a_shape, b_shape, a_strides=None, b_strides=None, a_t=False, b_t=False, swap_a=False, swap_b=False,
                native=True):
    """The plan of `a @ b` (module docstring).  native=False: tnn_gemm_batched is unavailable, `batched` becomes `loop`."""
    a_shape, a_st = _operand(a_shape, a_strides, a_t, swap_a)
    b_shape, b_st = _operand(b_shape, b_strides, b_t, swap_b)
    out_shape, batch, pa, pb, M, N, K = _shapes(a_shape, b_shape)
    p = Plan()
    p.out_shape, p.M, p.N, p.K = out_shape, M, N, K

    def matrix_of(shape, st, one_d_is_row):
        if len(shape) == 1:
            rows, cols, rs, cs = (1, shape[0], 0, st[0]) if one_d_is_row else (shape[0], 1, st[0], 0)
        else:
            rows, cols, rs, cs = shape[-2], shape[-1], st[-2], st[-1]
        bst = st[:-2] if len(shape) > 1 else ()
        ok = all(s >= 0 for s in bst)
        m = _matrix(rows, cols, rs, cs) if ok else None
        if m is None:                     # dense copy in logical order
            full = dense_strides(shape)
            bst = full[:-2] if len(shape) > 1 else ()
            return True, 0, max(cols, 1), bst
        return False, m[0], m[1], bst

    p.copy_a, p.ta, p.lda, a_bst = matrix_of(a_shape, a_st, True)
    p.copy_b, p.tb, p.ldb, b_bst = matrix_of(b_shape, b_st, False)
    nb = len(batch)
    a_bst = (0,) * (nb - len(a_bst)) + tuple(a_bst)
    b_bst = (0,) * (nb - len(b_bst)) + tuple(b_bst)
    a_bst = tuple(0 if x == 1 else s for x, s in zip(pa, a_bst))      # broadcast (or single) along the dimension
    b_bst = tuple(0 if x == 1 else s for x, s in zip(pb, b_bst))
    p.batch, p.a_bstrides, p.b_bstrides = _collapse(batch, a_bst, b_bst)
    p.batch_size = math.prod(batch)

    if len(a_shape) <= 2 and len(b_shape) <= 2:
        p.route = "gemm2d"
        return p
    # a dense stack of row-major matrices against ONE matrix: the batch dimension folds into the rows
    a_dense = math.prod(a_shape) == 0 or (p.ta == 0 and p.lda == max(K, 1) and (
        p.batch == () or (len(p.batch) == 1 and p.a_bstrides[0] == M * p.lda)))
    if len(b_shape) <= 2 and a_dense:
        p.route = "gemm2d"
        p.M = p.batch_size * M
        p.batch, p.a_bstrides, p.b_bstrides, p.batch_size = (), (), (), 1
        return p
    if not native or len(p.batch) > MAX_BATCH_DIMS:
        p.route = "loop"
    elif M * N * K >= LOOP_MIN_MNK:
        p.route = "loop"
    else:
        p.route = "batched"
    return p


def batch_offsets(plan):
    """[(a offset, b offset)] in elements of every batch element in C order (the `loop` route and the tests' replay)."""
    offs = [(0, 0)]
    for n, sa, sb in zip(plan.batch, plan.a_bstrides, plan.b_bstrides):
        offs = [(oa + i * sa, ob + i * sb) for oa, ob in offs for i in range(n)]
    return offs
