"""tests/golden/decode_cases.npz against tests/decode_oracle.py: the oracle reproduces the fixture, every u of the sampling
cases has the margin of 4 CDF bounds, every greedy step of the language model has a top-2 logit margin above 4 logit bounds,
and the bounds are tight enough to test something.  numpy only."""

import os

import numpy as np
import pytest

import attn_oracle as ao
import decode_oracle as do
import decode_support as ds


@pytest.fixture(scope="module")
def golden():
    return ds.load_golden()


def test_the_fixture_is_small_and_complete(golden):
    assert os.path.getsize(ds.GOLDEN) < 64 * 1024
    want = {"decode." + n for n in do.DECODE_CASES} | {"lm.head_scale", "lm.logit_bound", "lm.ids"}
    want |= {"sample.%s.%s" % (n, f) for n in do.SAMPLE_CASES for f in ("u", "ids")}
    assert set(golden) == want


@pytest.mark.parametrize("name", sorted(do.DECODE_CASES))
def test_decode_oracle_reproduces_the_fixture(golden, name):
    case = do.decode_case(name, np.float32)
    for dtype in (np.float32, np.float64):
        res = ds.reference(case, dtype, case["splits"])
        np.testing.assert_allclose(res.values["o"], golden["decode." + name], rtol=1e-12, atol=1e-300)
        # the bound means something: the oracle's own value passes the tightness gate of attn_oracle.assert_within
        ao.assert_within(res.values["o"], res.values["o"], res.bounds["o"], "%s %s" % (name, np.dtype(dtype).name))
    k_after = res.values["k_cache"]
    if case["k_new"] is not None:                              # the appended row, and nothing else
        row = k_after[:, case["length"]] if case["layout"] == "bthd" else k_after[:, :, case["length"]]
        assert np.array_equal(row, case["k_new"])
        assert np.array_equal(do.put_row(k_after, case["layout"], case["length"], 0 * case["k_new"]),
                              do.put_row(case["k_cache"], case["layout"], case["length"], 0 * case["k_new"]))


def test_the_rescale_count():
    assert do.rescales(1, 1) == 4 + 8 and do.rescales(64, 1) == 4 + 8 and do.rescales(65, 1) == 8 + 8
    assert do.rescales(301, 5) == 4 + 8 and do.rescales(301, 2) == 12 + 8          # runs of at most 1 and 3 chunks


@pytest.mark.parametrize("name", sorted(do.SAMPLE_CASES))
def test_sampling_oracle_reproduces_the_fixture_with_the_margin(golden, name):
    x, temperature, top_k = do.sample_case(name, np.float32)
    u, ids = golden["sample.%s.u" % name], golden["sample.%s.ids" % name]
    assert u.dtype == np.float32 and ((u >= 0) & (u < 1)).all()
    for dtype in (np.float32, np.float64):
        res = do.sample_reference(x, temperature, top_k, dtype)
        assert np.array_equal(res.tokens(u), ids)
        margins = res.margins(u)
        assert (margins > do.MARGIN).all(), "%s %s: least margin %.2f bounds" % (name, np.dtype(dtype).name, margins.min())
        for r in range(x.shape[0]):
            kept = res.kept[r]
            assert kept[ids[r]] and kept.sum() == (top_k if top_k and top_k < x.shape[1] else x.shape[1])
            assert res.lo[r][ids[r]] <= u[r] < res.hi[r][ids[r]]
            assert 0 < res.cdf_bound[r] < 1e-3


def test_the_rule_on_hand_made_rows():
    """Ties at the threshold go to the lowest indices; -inf owns an empty interval; the ends 0 and 1 are exempt."""
    x = np.array([[1.0, 3.0, 3.0, 3.0, -np.inf, 0.0]], dtype=np.float32)
    res = do.sample_reference(x, 1.0, 2, np.float32)
    assert res.kept[0].tolist() == [False, True, True, False, False, False]
    assert res.lo[0][1] == 0.0 and res.hi[0][1] == 0.5 == res.lo[0][2] and res.hi[0][2] == 1.0
    assert res.tokens([0.0]).tolist() == [1] and res.tokens([0.75]).tolist() == [2]
    assert res.margins([0.0])[0] > 1e4 and res.margins([np.nextafter(1.0, 0.0)])[0] > 1e4
    assert res.margins([0.5])[0] == 0.0
    full = do.sample_reference(x, 2.0, None, np.float64)
    assert full.kept[0].all() and full.lo[0][4] == full.hi[0][4]          # -inf: never chosen
    assert full.tokens([np.nextafter(1.0, 0.0)]).tolist() == [5]
    assert do.sample_reference(x, 0.0, None).argmax.tolist() == [1]
    neg_zero = do.tempered(np.array([[-0.0, 0.0]], dtype=np.float32), 1.0, np.float32)
    assert not np.signbit(neg_zero).any()


def test_language_model_margin(golden):
    scale, bound = float(golden["lm.head_scale"]), float(golden["lm.logit_bound"])
    params = do.lm_params(scale)
    ids, steps = do.lm_generate(params, do.lm_prompt(), do.LM_NEW)
    assert np.array_equal(ids, golden["lm.ids"]) and ids.shape == (3, do.LM_PROMPT + do.LM_NEW)
    assert bound > 0 and do.top2_margin(steps) > do.MARGIN * bound
    assert do.LM_PROMPT + do.LM_NEW <= do.to.LM_CASE["max_len"]
