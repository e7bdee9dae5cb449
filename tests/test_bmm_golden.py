"""tests/golden/bmm_cases.npz is what the reference computes: regenerated from the reference's own core.ops.dot_ and compared
bit for bit.  The regeneration is skipped where the reference is absent (it never travels to the GPU machine)."""

import os

import numpy as np
import pytest

import gen_bmm_golden as G

needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(G.REF, "core")),
                                     reason="reference checkout not present (it never travels to the GPU box)")


@needs_reference
def test_fixture_is_the_reference_bit_for_bit():
    stored = G.load()
    fresh = G.generate()
    assert sorted(stored) == sorted(fresh)
    for k in fresh:
        assert stored[k].dtype == fresh[k].dtype and stored[k].shape == fresh[k].shape, k
        np.testing.assert_array_equal(stored[k], fresh[k], err_msg=k)


def test_fixture_holds_the_named_forms():
    stored = G.load()
    assert len(G.CASES) >= 20 and os.path.getsize(G.GOLDEN) <= 100 * 1024
    shapes = set(G.CASES.values())
    for pair in (((4, 3, 5), (4, 5, 2)), ((4, 3, 5), (5, 2)), ((3, 5), (4, 5, 2)), ((2, 1, 3, 5), (1, 4, 5, 2)),
                 ((5,), (4, 5, 2)), ((4, 3, 5), (5,)), ((3, 3, 3), (3, 3, 3)),
                 ((1000, 4, 4), (1000, 4, 4)), ((3, 200, 70), (70, 30))):
        assert pair in shapes
    assert any(len(a) == 5 or len(b) == 5 for a, b in shapes)                  # a 5-D broadcast
    assert any(len(a) > 2 and a[-1] == 1 for a, b in shapes)                    # K = 1
    assert any(len(a) > 2 and a[-2] % 16 and a[-1] % 16 and b[-1] % 16 for a, b in shapes)
    for name, (sa, sb) in G.CASES.items():
        a, b, g = G.case_input(name)
        fwd = stored[name + "/fwd"]
        assert a.dtype == np.float32 and b.dtype == np.float32
        assert fwd.shape == np.matmul(a, b).shape == g.shape, name
        np.testing.assert_array_equal(fwd.astype(np.float64), np.matmul(a.astype(np.float64), b.astype(np.float64)))


def test_recorded_reference_backward_results():
    """The issue's finding, as recorded data: the reference's backward raises for the six N-d / 1-D shape pairs, runs for
    2-D @ 2-D, and runs (with a wrong gradient) for cubes."""
    stored = G.load()
    raised = {name: bool(stored[name + "/bwd_raised"]) for name in G.CASES}
    for name in ("stack", "stack_by_matrix", "matrix_by_stack", "broadcast_4d", "vector_by_stack", "stack_by_vector"):
        assert raised[name], name
    assert not raised["plain_2d"] and not raised["cubes"]
