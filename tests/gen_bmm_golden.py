"""TEST INFRASTRUCTURE — the batched-matmul fixture tests/golden/bmm_cases.npz, recorded from the REAL reference.

    python tests/gen_bmm_golden.py          (needs the reference checkout: TNN_REFERENCE_DIR, default /root/reference)

Every case of CASES runs through the reference's own core.ops.dot_ (imported, never copied): the forward values, and — as a
recorded RESULT — whether the reference's `backward` raised for that shape pair (its vjps transpose with `.T`, which
reverses all axes, so everything but 2-D @ 2-D raises or mis-shapes; this package follows the mathematical vjp instead,
tests/test_bmm_host.py).  Operands are small integers held in float32, so every product and partial sum is an integer far
below 2**24: float32 must reproduce the forward bit for bit, in any summation order.  The fixture holds arrays only: fwd of
each case (the integers the reference's float32 product holds, stored exactly as int16) and the flag bwd_raised; the operands are rebuilt by case_input() from the case's seed (numpy's legacy
RandomState stream is frozen), which keeps the file small.
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("TNN_REFERENCE_DIR", "/root/reference")
GOLDEN = os.path.join(HERE, "golden", "bmm_cases.npz")

# name -> (shape of a, shape of b)
CASES = {
    "stack": ((4, 3, 5), (4, 5, 2)),
    "stack_by_matrix": ((4, 3, 5), (5, 2)),
    "matrix_by_stack": ((3, 5), (4, 5, 2)),
    "broadcast_4d": ((2, 1, 3, 5), (1, 4, 5, 2)),
    "vector_by_stack": ((5,), (4, 5, 2)),
    "stack_by_vector": ((4, 3, 5), (5,)),
    "cubes": ((3, 3, 3), (3, 3, 3)),
    "plain_2d": ((7, 5), (5, 3)),
    "odd_17_19_23": ((3, 17, 23), (3, 23, 19)),
    "odd_33_65_31": ((2, 33, 31), (2, 31, 65)),
    "odd_70_66_9": ((2, 70, 9), (2, 9, 66)),
    "k_is_1": ((6, 5, 1), (6, 1, 7)),
    "m_is_1": ((6, 1, 9), (6, 9, 4)),
    "n_is_1": ((6, 4, 9), (6, 9, 1)),
    "broadcast_5d": ((2, 1, 3, 4, 6), (1, 2, 1, 6, 5)),
    "thousand_4x4": ((1000, 4, 4), (1000, 4, 4)),
    "dense_form": ((3, 200, 70), (70, 30)),
    "heads": ((2, 4, 10, 8), (2, 4, 8, 10)),
    "one_batch_each_side": ((1, 6, 7), (5, 7, 3)),
    "stack_by_broadcast_matrix": ((5, 6, 7), (1, 7, 3)),
    "tile_edge_64": ((1, 64, 16), (1, 16, 64)),
    "tile_over_64": ((2, 65, 17), (2, 17, 70)),
    "small_32": ((3, 32, 32), (3, 32, 32)),
    "vector_by_matrix": ((5,), (5, 3)),
}


def case_input(name):
    """(a, b, g): small-integer float32 operands and an upstream gradient of the product's shape, seeded by the case's
    position in the table."""
    sa, sb = CASES[name]
    rs = np.random.RandomState(2000 + list(CASES).index(name))
    a = rs.randint(-3, 4, size=sa).astype(np.float32)
    b = rs.randint(-3, 4, size=sb).astype(np.float32)
    g = rs.randint(-3, 4, size=np.matmul(a, b).shape).astype(np.float32)
    return a, b, g


def import_reference():
    if not os.path.isdir(os.path.join(REF, "core")):
        raise RuntimeError("reference not found at %s" % REF)
    saved = {k: v for k, v in sys.modules.items() if k == "core" or k.startswith("core.")}
    for k in saved:
        del sys.modules[k]
    sys.path.insert(0, REF)
    old_flag = sys.dont_write_bytecode
    sys.dont_write_bytecode = True                       # never write into the reference tree
    try:
        import core.tensor as rt
        import core.ops as rops
        return rt, rops
    finally:
        sys.dont_write_bytecode = old_flag
        sys.path.remove(REF)
        for k in [k for k in sys.modules if k == "core" or k.startswith("core.")]:
            del sys.modules[k]
        sys.modules.update(saved)


def generate():
    """{array name: array} of every case, from the reference."""
    rt, rops = import_reference()
    arrays = {}
    for name in CASES:
        a, b, g = case_input(name)
        ta, tb = rt.Tensor(a, requires_grad=True), rt.Tensor(b, requires_grad=True)
        out = rops.dot_(ta, tb)
        try:
            out.backward(g)
            raised = False
        except Exception:
            raised = True
        fwd = np.asarray(out.values)
        assert fwd.dtype == np.float32 and np.array_equal(fwd, fwd.astype(np.int16)), name
        arrays[name + "/fwd"] = fwd.astype(np.int16)             # integers, exactly: a third of the float32 file
        arrays[name + "/bwd_raised"] = np.array(raised)
    return arrays


def load():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def closed_form_grads(a, b, g):
    """The mathematical vjps of a @ b in float64 (einsum over the promoted, broadcast operands), un-broadcast to the
    operands' shapes.  Exact on the fixture's integer data."""
    a64, b64, g64 = (np.asarray(v, dtype=np.float64) for v in (a, b, g))
    a2 = a64[None, :] if a64.ndim == 1 else a64
    b2 = b64[:, None] if b64.ndim == 1 else b64
    batch = np.broadcast_shapes(a2.shape[:-2], b2.shape[:-2])
    g2 = g64.reshape(batch + (a2.shape[-2], b2.shape[-1]))
    ab = np.broadcast_to(a2, batch + a2.shape[-2:])
    bb = np.broadcast_to(b2, batch + b2.shape[-2:])
    ga = np.einsum("...mn,...kn->...mk", g2, bb)
    gb = np.einsum("...mk,...mn->...kn", ab, g2)

    def unbroadcast(x, shape):
        x = x.sum(axis=tuple(range(x.ndim - len(shape)))) if x.ndim > len(shape) else x
        for i, d in enumerate(shape):
            if d == 1 and x.shape[i] != 1:
                x = x.sum(axis=i, keepdims=True)
        return x

    return unbroadcast(ga, a2.shape).reshape(a64.shape), unbroadcast(gb, b2.shape).reshape(b64.shape)


if __name__ == "__main__":
    arrays = generate()
    np.savez_compressed(GOLDEN, **arrays)
    print("wrote %s (%d cases, %d bytes)" % (GOLDEN, len(CASES), os.path.getsize(GOLDEN)))
