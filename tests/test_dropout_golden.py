"""tests/golden/dropout_cases.npz (written by tests/gen_dropout_golden.py from the planner's own generator) against the
planner as it is now: an edit of the generator, of the index mapping or of the rounding rules cannot silently change every
seeded run."""

import os

import numpy as np
import pytest

import gen_dropout_golden as gd
from tinynn_autograd_amd import dropout as dp

FIELDS = ("x", "residual", "words", "keep", "uniform", "y", "y_residual")


@pytest.fixture(scope="module")
def golden():
    with np.load(gd.OUT) as data:
        return dict(data)


def test_fixture_is_complete_and_small(golden):
    assert set(golden) == {"%s.%s" % (name, field) for name in gd.CASES for field in FIELDS}
    assert os.path.getsize(gd.OUT) < 16 * 1024


def test_known_words_of_the_fixture(golden):
    assert golden["across_the_block_carry.words"][:4].tolist() == [2624505957, 2176703114, 2516343209, 1286663913]
    assert golden["zero_state.words"][:4].tolist() == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]      # the all-zero vector


@pytest.mark.parametrize("name", sorted(gd.CASES))
def test_planner_reproduces_the_fixture(golden, name):
    seed, calls, first, n, p, dtype = gd.CASES[name]
    x, res = gd.case_input(name)
    np.testing.assert_array_equal(x, golden[name + ".x"].astype(dtype))
    np.testing.assert_array_equal(res, golden[name + ".residual"].astype(dtype))
    words = dp.stream_words(seed, calls, first, n)
    assert words.dtype == golden[name + ".words"].dtype == np.uint32
    np.testing.assert_array_equal(words, golden[name + ".words"])
    keep = dp.keep_mask(seed, calls, first, n, dp.threshold_of(p))
    np.testing.assert_array_equal(keep, golden[name + ".keep"])
    assert 0 < keep.sum() < n
    for field, got in (("uniform", dp.uniform(seed, calls, first, n, dtype)), ("y", dp.reference(x, seed, calls, p, first=first)),
                       ("y_residual", dp.reference(x, seed, calls, p, residual=res, first=first))):
        want = golden[name + "." + field]
        assert got.dtype == want.dtype == dtype
        np.testing.assert_array_equal(got.view(np.uint8), want.view(np.uint8), err_msg=field)


def test_the_generator_script_rebuilds_the_fixture(golden):
    rebuilt = gd.build(gd.planner())
    assert set(rebuilt) == set(golden)
    for key, want in golden.items():
        assert rebuilt[key].dtype == want.dtype, key
        np.testing.assert_array_equal(rebuilt[key], want, err_msg=key)
