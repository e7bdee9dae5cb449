"""The numpy-only planner of dropout (tinynn-autograd_amd/dropout.py): the reference Philox4x32-10 generator against the
published known-answer vectors, the mapping from a stream index to a block and a word, the threshold / scale rounding, every
ValueError, and two deterministic statistical checks of the keep masks."""

import math

import numpy as np
import pytest

from tinynn_autograd_amd import dropout as dp

KAT = [  # (counter, key, words): the known-answer vectors of the Random123 distribution for philox4x32-10
    ([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ([0xffffffff] * 4, [0xffffffff] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


def words_of(text):
    return [int(w, 16) for w in text.split()]


def test_known_answer_vectors():
    for counter, key, want in KAT:
        got = dp.philox4x32_10(counter, key)
        assert got.dtype == np.uint32 and got.tolist() == words_of(want)
    together = dp.philox4x32_10([c for c, _, _ in KAT], [k for _, k, _ in KAT])          # vectorised over blocks
    assert together.tolist() == [words_of(w) for _, _, w in KAT]
    with pytest.raises(ValueError, match="counter"):
        dp.philox4x32_10([0, 0, 0], [0, 0])


def test_constants():
    assert (dp.MUL0, dp.MUL1, dp.KEY0, dp.KEY1) == (0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85)
    assert dp.ROUNDS == 10 and dp.DRAW_BITS == 24 and dp.STATE_BYTES == 16 and dp.THREADS == 256 and dp.VEC == 16


def block(seed, calls, index):
    return dp.philox4x32_10([index & 0xffffffff, index >> 32, calls & 0xffffffff, calls >> 32],
                            [seed & 0xffffffff, seed >> 32])


def test_index_mapping():
    """Element i is word i & 3 of block i >> 2; `calls` fills the upper counter words and the seed the key."""
    seed, calls = 2 ** 40 + 7, 2 ** 33 + 5
    words = dp.stream_words(seed, calls, 0, 24)
    for i in range(24):
        assert words[i] == block(seed, calls, i >> 2)[i & 3]
    for first in (1, 2, 3, 4, 7):
        for n in (0, 1, 4, 9):
            np.testing.assert_array_equal(dp.stream_words(seed, calls, first, n), words[first:first + n])
    assert block(seed, calls, 0).tolist() != block(seed, calls + 1, 0).tolist()
    assert block(seed, calls, 0).tolist() != block(seed, calls + 2 ** 32, 0).tolist()     # the high word of calls counts
    assert block(seed, calls, 0).tolist() != block(seed + 2 ** 32, calls, 0).tolist()     # the high word of the seed counts
    # across the 32-bit carry of the block index: blocks 2^32 - 2 .. 2^32 + 1
    first = 2 ** 34 - 8
    words = dp.stream_words(7, 3, first, 16)
    assert words[:4].tolist() == [2624505957, 2176703114, 2516343209, 1286663913]
    for j in range(16):
        assert words[j] == block(7, 3, (first + j) >> 2)[(first + j) & 3]
    assert words[8:12].tolist() == dp.philox4x32_10([0, 1, 3, 0], [7, 0]).tolist()
    assert dp.stream_words(7, 3, 5, 0).shape == (0,)


def test_draws_masks_and_uniform_numbers():
    words = dp.stream_words(1, 2, 3, 1000)
    r = dp.draws(1, 2, 3, 1000)
    np.testing.assert_array_equal(r, words >> 8)
    for t in (0, 1, 2 ** 23, 2 ** 24 - 1):
        np.testing.assert_array_equal(dp.keep_mask(1, 2, 3, 1000, t), r >= t)
    assert dp.keep_mask(1, 2, 3, 1000, 0).all()
    for dtype in (np.float32, np.float64):
        u = dp.uniform(1, 2, 3, 1000, dtype)
        assert u.dtype == dtype and (u >= 0).all() and (u < 1).all()
        np.testing.assert_array_equal(u.astype(np.float64) * 2.0 ** 24, r.astype(np.float64))       # exact
    with pytest.raises(ValueError, match="float32 or float64"):
        dp.uniform(1, 2, 3, 4, np.float16)
    with pytest.raises(ValueError, match="threshold"):
        dp.keep_mask(1, 2, 3, 4, 2 ** 24)


def test_threshold_and_scale():
    assert dp.threshold_of(0.0) == 0 and dp.threshold_of(0.5) == 2 ** 23 and dp.threshold_of(0.25) == 2 ** 22
    assert dp.threshold_of(0.1) == round(0.1 * 2 ** 24) == 1677722
    assert dp.threshold_of(2.0 ** -26) == 0                      # rounds to "keep everything"; the scale stays 1 / (1 - p)
    assert dp.threshold_of(1 - 2.0 ** -24) == 2 ** 24 - 1
    plan = dp.plan_dropout((3, 5), 0.1, np.float32, first=6)
    assert (plan.shape, plan.n, plan.first, plan.threshold, plan.route) == ((3, 5), 15, 6, 1677722, "native")
    assert plan.scale == 1.0 / (1.0 - 0.1) and isinstance(plan.scale, float)
    assert dp.plan_dropout((), 0.5).n == 1 and dp.plan_dropout((0, 4), 0.5).n == 0
    assert dp.plan_dropout((4,), 0.5, np.float64, native=False).route == "composed"
    assert dp.plan_dropout((4,), 0.5, np.float64, float_ok=False).route == "composed"
    assert dp.plan_dropout((4,), 0.5, np.int64).route == "composed"
    assert dp.plan_dropout((4,), 0.5, route="composed").route == "composed"
    # the grid of the native launch: one lane per Philox block that overlaps the slice, capped
    assert dp.plan_dropout((0,), 0.5).grid() == 0
    assert dp.plan_dropout((1024,), 0.5).grid() == 1 and dp.plan_dropout((1024,), 0.5, first=1).grid() == 2
    assert dp.plan_dropout((4 * 256 * dp.MAX_BLOCKS + 5,), 0.5).grid() == dp.MAX_BLOCKS == 2048


def test_every_value_error():
    for p in (-0.1, 1.0, 1.5, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match=r"p must be"):
            dp.plan_dropout((4,), p)
    with pytest.raises(ValueError, match="rounds to a threshold of 2\\^24"):
        dp.plan_dropout((4,), 1 - 2.0 ** -26)
    with pytest.raises(ValueError, match="route must be one of"):
        dp.plan_dropout((4,), 0.5, route="fast")
    with pytest.raises(ValueError, match="native dropout route needs"):
        dp.plan_dropout((4,), 0.5, np.int64, route="native")
    with pytest.raises(ValueError, match="native dropout route needs"):
        dp.plan_dropout((4,), 0.5, np.float32, native=False, route="native")
    for first, n in ((-1, 4), (2 ** 63 - 4, 5)):
        with pytest.raises(ValueError, match="stream slice"):
            dp.plan_dropout((n,), 0.5, first=first)
        with pytest.raises(ValueError, match="stream slice"):
            dp.stream_words(0, 0, first, n)
    assert dp.plan_dropout((4,), 0.5, first=2 ** 63 - 5).first == 2 ** 63 - 5


def test_kept_fraction_within_four_standard_deviations():
    n = 2 ** 20
    worst = 0.0
    for seed, calls in ((0, 0), (1234, 0), (1234, 1), (2 ** 40 + 7, 5)):
        for p in (0.1, 0.5, 0.9):
            kept = dp.keep_mask(seed, calls, 0, n, dp.threshold_of(p)).mean()
            z = abs(kept - (1 - p)) / math.sqrt(p * (1 - p) / n)
            worst = max(worst, z)
            assert z <= 4.0, (seed, calls, p, z)
    print("worst deviation: %.2f standard deviations" % worst)


def test_masks_of_consecutive_calls_are_independent():
    n = 2 ** 20
    t = dp.threshold_of(0.5)
    agree = (dp.keep_mask(1234, 0, 0, n, t) == dp.keep_mask(1234, 1, 0, n, t)).mean()
    print("agreement of consecutive masks: %.4f" % agree)
    assert abs(agree - 0.5) <= 4 * math.sqrt(0.25 / n)


def test_reference_formula():
    x = np.array([1.5, -2.0, np.inf, np.nan, 3.0, -0.5, 7.0, 1.0], dtype=np.float32)
    keep = dp.keep_mask(9, 4, 2, 8, dp.threshold_of(0.5))
    assert 0 < keep.sum() < 8
    y = dp.reference(x, 9, 4, 0.5, first=2)
    assert y.dtype == np.float32 and not np.signbit(y[~keep]).any() and (y[~keep] == 0).all()
    np.testing.assert_array_equal(y[keep], (x * np.float32(2.0))[keep])
    res = np.arange(8, dtype=np.float32) + 1
    np.testing.assert_array_equal(dp.reference(x, 9, 4, 0.5, residual=res, first=2)[~keep], res[~keep])
    # the scale is rounded ONCE to the operand dtype, the product and the sum separately
    x64 = np.array([0.1, 0.2, 0.3, 0.7], dtype=np.float64)
    keep = dp.keep_mask(9, 4, 0, 4, dp.threshold_of(0.3))
    want = np.where(keep, x64 * np.float64(1.0 / (1.0 - 0.3)), 0.0) + x64
    np.testing.assert_array_equal(dp.reference(x64, 9, 4, 0.3, residual=x64), want)
    x32 = x64.astype(np.float32)
    want = np.where(keep, x32 * np.float32(1.0 / (1.0 - 0.3)), np.float32(0)) + x32
    np.testing.assert_array_equal(dp.reference(x32, 9, 4, 0.3, residual=x32), want)
