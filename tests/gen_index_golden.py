"""TEST INFRASTRUCTURE — the advanced-indexing fixture tests/golden/index_cases.npz, recorded from the REAL reference.

    python tests/gen_index_golden.py          (needs the reference checkout: TNN_REFERENCE_DIR, default /root/reference)

Every case of CASES runs through the reference's own core.ops.getitem_ / pad_ (imported, never copied): the forward values
and the gradient that `backward(g)` leaves on the input.  The keys are rebuilt from this table by whoever reads the fixture
(tests/test_index_golden.py, tests/test_gpu_indexing.py); the fixture holds arrays only: x, g, fwd and grad of each case.
Values are float32-representable, so the float32 mode of this package must reproduce them bit for bit (pure moves).
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("TNN_REFERENCE_DIR", "/root/reference")
GOLDEN = os.path.join(HERE, "golden", "index_cases.npz")


def _i(*v):
    return np.array(v, dtype=np.int64)


# name -> (input shape, key(x) or ("pad", pad_width, mode)); key(x) builds the key from the input's values — a numpy array
# for the reference, a device array for this package (so `x > 0` is a device mask there)
CASES = {
    "nll_labels": ((8, 5), lambda x: (np.arange(8), _i(0, 4, 2, 2, 1, 3, 0, 4))),
    "mask_cmp": ((6, 7), lambda x: x > 0),
    "mask_rows": ((6, 7), lambda x: np.array([True, False, True, True, False, True])),
    "idx_2d": ((10, 4), lambda x: _i(0, 9, 3, 3, 1, 2, 8, 7, 5, 5, 0, 6).reshape(3, 4)),
    "separated_adv": ((2, 3, 4, 5), lambda x: (slice(None), [0, 1], slice(None), [1, 2])),
    "adjacent_adv": ((3, 4, 5), lambda x: (slice(None), _i(0, 2, 1), _i(1, 1, 4))),
    "dup_rows": ((5, 3), lambda x: _i(0, 0, 1, 4, 4, 4)),
    "dup_pairs": ((4, 4), lambda x: (_i(0, 0, 1, 0), _i(2, 2, 3, 2))),
    "negative_rows": ((6, 3), lambda x: (_i(-1, -6, 2), slice(None))),
    "columns": ((4, 6), lambda x: (slice(None), _i(5, 0, 2))),
    "rows_then_slice": ((7, 8), lambda x: (_i(1, 3, 6), slice(2, None))),
    "ellipsis_newaxis": ((3, 4, 5), lambda x: (Ellipsis, None, _i(0, 4))),
    "int_with_array": ((3, 4, 5), lambda x: (1, slice(None), _i(0, 1, 3))),
    "mask_3d": ((2, 3, 4), lambda x: x < 0.25),
    "mask_trailing": ((3, 4, 5), lambda x: (slice(None), np.arange(20).reshape(4, 5) % 3 == 1)),
    "broadcast_idx": ((5, 6), lambda x: (_i(4, 0, 2).reshape(3, 1), _i(5, 1, 1, 0).reshape(1, 4))),
    "empty_idx": ((4, 3), lambda x: np.zeros(0, dtype=np.int64)),
    "reversed_slice_adv": ((6, 5), lambda x: (slice(None, None, -2), _i(4, 0))),
    "rows_with_mask": ((4, 5), lambda x: (_i(1, 1, 2), np.array([False, True, False, True, True]))),
    "idx_2d_dup_cols": ((3, 6), lambda x: (slice(None), _i(1, 1, 5, 1).reshape(2, 2))),
    "pad_constant": ((3, 4), ("pad", ((1, 2), (0, 3)), "constant")),
    "pad_edge": ((3, 4), ("pad", ((2, 1), (1, 1)), "edge")),
    "pad_reflect": ((3, 4), ("pad", ((1, 2), (2, 2)), "reflect")),
    "pad_reflect_wide": ((3, 4), ("pad", ((5, 4), (7, 1)), "reflect")),
    "pad_symmetric": ((3, 4), ("pad", ((2, 3), (1, 4)), "symmetric")),
    "pad_wrap": ((3, 4), ("pad", ((3, 1), (2, 5)), "wrap")),
    "pad_edge_3d": ((2, 3, 4), ("pad", ((1, 0), (0, 2), (1, 1)), "edge")),
    "pad_reflect_1d": ((5,), ("pad", ((3, 2),), "reflect")),
    "pad_wrap_wide": ((2, 3), ("pad", ((4, 4), (5, 5)), "wrap")),
    "pad_symmetric_wide": ((3, 2), ("pad", ((4, 1), (3, 3)), "symmetric")),
}


def case_input(name):
    """(x, g) of a case: float32-representable float64 values, seeded by the case's position in the table."""
    shape, spec = CASES[name]
    rs = np.random.RandomState(1000 + list(CASES).index(name))
    x = rs.randn(*shape).astype(np.float32).astype(np.float64)
    if isinstance(spec, tuple):
        _, pw, mode = spec
        out_shape = tuple(s + b + a for s, (b, a) in zip(shape, pw))
    else:
        out_shape = x[spec(x)].shape
    g = rs.randn(*out_shape).astype(np.float32).astype(np.float64)
    return x, g


def run_case(name, Tensor, ops, to_values=lambda v: v):
    """(fwd, grad) of one case through a Tensor / ops pair (the reference's or this package's)."""
    _, spec = CASES[name]
    x, g = case_input(name)
    t = Tensor(x, requires_grad=True)
    if isinstance(spec, tuple):
        _, pw, mode = spec
        out = ops.pad_(t, pw, mode)
    else:
        out = ops.getitem_(t, spec(t.values))
    out.backward(g)
    return np.asarray(to_values(out.values), dtype=np.float64), np.asarray(to_values(t.grad), dtype=np.float64)


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
        x, g = case_input(name)
        fwd, grad = run_case(name, rt.Tensor, rops)
        arrays[name + "/x"], arrays[name + "/g"] = x, g
        arrays[name + "/fwd"], arrays[name + "/grad"] = fwd, grad
    return arrays


def load():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


if __name__ == "__main__":
    arrays = generate()
    np.savez_compressed(GOLDEN, **arrays)
    print("wrote %s (%d cases, %d bytes)" % (GOLDEN, len(CASES), os.path.getsize(GOLDEN)))
