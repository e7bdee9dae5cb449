"""tests/golden/index_cases.npz is what the reference computes: regenerated from the reference's own core.ops and compared
bit for bit.  Skipped where the reference is absent (it never travels to the GPU machine)."""

import os

import numpy as np
import pytest

import gen_index_golden as G

pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(G.REF, "core")),
                                reason="reference checkout not present (it never travels to the GPU box)")


def test_fixture_is_the_reference_bit_for_bit():
    stored = G.load()
    fresh = G.generate()
    assert sorted(stored) == sorted(fresh)
    assert len(G.CASES) >= 30 and os.path.getsize(G.GOLDEN) <= 100 * 1024
    for k in fresh:
        assert stored[k].dtype == fresh[k].dtype and stored[k].shape == fresh[k].shape, k
        np.testing.assert_array_equal(stored[k], fresh[k], err_msg=k)


def test_fixture_holds_the_named_forms():
    names = set(G.CASES)
    for must in ("nll_labels", "mask_cmp", "idx_2d", "separated_adv", "dup_rows", "pad_edge", "pad_reflect",
                 "pad_reflect_wide", "pad_symmetric", "pad_wrap"):
        assert must in names
