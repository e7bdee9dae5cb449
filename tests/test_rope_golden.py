"""The rotary oracle (tests/rope_oracle.py, long double) reproduces tests/golden/rope_cases.npz, which
tests/gen_rope_golden.py wrote from it: the yardstick the kernel is judged against has not moved."""

import numpy as np
import pytest

import rope_oracle as ro
import rope_support as rsup
from tinynn_autograd_amd import rope as rp


@pytest.fixture(scope="module")
def golden():
    return rsup.load_golden()


def test_the_fixture_holds_every_case(golden):
    names = {"%s.%s.%s" % (pairing, name, which) for pairing in ro.PAIRINGS for name, c in ro.CASES.items()
             for which in ("a", "b") if which == "a" or c[3]}
    assert names <= set(golden) and not [k for k in golden if k.split(".")[0] in ro.PAIRINGS and k not in names]
    assert {"table.spots", "table.cos", "table.sin", "lm.seed", "lm.head_scale", "lm.logit_bound", "lm.ids"} <= set(golden)
    assert list(ro.CASES.values()) == [(1, 1, 1, 0, 2, 2), (2, 5, 3, 1, 3, 2), (1, 5, 2, 2, 8, 8), (3, 1, 4, 2, 16, 8),
                                       (1, 65, 4, 1, 24, 12), (2, 3, 8, 1, 64, 64), (1, 2, 2, 2, 128, 128), (1, 2, 1, 1, 130, 128)]


@pytest.mark.parametrize("pairing", ro.PAIRINGS)
@pytest.mark.parametrize("name", sorted(ro.CASES))
def test_the_oracle_reproduces_the_fixture(golden, name, pairing):
    """To 2^-50 of the magnitudes behind every element: the fixture stores the long-double values rounded to float64."""
    R = ro.CASES[name][5]
    cos_t, sin_t = rp.tables(ro.P, R, ro.BASE, np.float32)
    for which, x in zip("ab", ro.case_input(name, np.float32)):
        if x is None:
            continue
        res = ro.reference(x, cos_t, sin_t, ro.GOLDEN_OFFSET, None, "bthd", pairing, False, np.float32)
        want = golden["%s.%s.%s" % (pairing, name, which)]
        assert want.shape == x.shape and want.dtype == np.float64
        scale = res.bounds / (ro.gamma2(np.float32) + ro.ORACLE_REL)              # |x_lo c| + |x_hi s| per element
        assert (np.abs(res.values.astype(np.float64) - want) <= 2.0 ** -50 * scale).all()
        assert np.array_equal(want[..., R:], x[..., R:].astype(np.float64))          # the tail is a copy
        # the layouts are views of one result, and the inverse undoes the rotation to twice the bound
        xt = np.ascontiguousarray(x.transpose(0, 2, 1, 3))
        rt = ro.reference(xt, cos_t, sin_t, ro.GOLDEN_OFFSET, None, "bhtd", pairing, False, np.float32)
        assert np.array_equal(rt.values.transpose(0, 2, 1, 3), res.values)
        back = ro.reference(res.values.astype(np.float64), cos_t.astype(np.float64), sin_t.astype(np.float64), ro.GOLDEN_OFFSET,
                            None, "bthd", pairing, True, np.float64)
        c2s2 = 1.0 + 2.0 ** -22                                                    # cos^2 + sin^2 of float32-rounded entries
        assert (np.abs(back.values.astype(np.float64) - x) <= (c2s2 - 1.0) * np.abs(x).max() + 1e-12).all()


def test_the_language_model_fixture(golden):
    c = ro.LM
    seed, scale, bound = int(golden["lm.seed"]), float(golden["lm.head_scale"]), float(golden["lm.logit_bound"])
    params, prompt = ro.lm_params(seed, scale), ro.lm_prompt(seed)
    assert "emb.pos" not in params
    ids, steps = ro.lm_generate(params, prompt, c["new"])
    srt = np.sort(steps, axis=-1)
    assert np.array_equal(ids, golden["lm.ids"]) and float((srt[..., -1] - srt[..., -2]).min()) > 2 * ro.LM_MARGIN * bound
