"""tests/golden/varlen_cases.npz (tests/gen_varlen_golden.py: float64, cross-checked against torch per sequence there) against
the composed route, under the per-sequence oracle's bounds; the fixture itself against the oracle as it is computed today."""

import numpy as np
import pytest

import varlen_support as vs
import tinynn_autograd_amd as tn


@pytest.fixture(scope="module")
def golden():
    return vs.load_golden()


def test_the_fixture_holds_every_case(golden):
    assert sorted(golden) == sorted("varlen.%s.%s" % (c, f) for c in vs.VARLEN_CASES for f in ("o", "lse", "dq", "dk", "dv"))


@pytest.mark.parametrize("name", sorted(vs.VARLEN_CASES))
def test_the_composed_route_against_the_fixture(golden, name):
    for dtype in (np.float32, np.float64):
        tn.set_default_float(dtype)
        q, k, v, do_, lens, causal, scale, layout = vs.case_input(name, dtype)
        res = vs.reference(q, k, v, do_, lens, causal, scale, layout, dtype)
        for field in ("o", "lse", "dq", "dk", "dv"):
            stored = golden["varlen.%s.%s" % (name, field)]
            if dtype == np.float32:                        # (the float64 inputs are other numbers: the fixture is float32's)
                assert np.abs(stored - res.values[field]).max() <= 1e-12 * max(np.abs(stored).max(), 1.0), field
                res.values[field] = stored
        if dtype == np.float32:
            got = vs.run("composed", q, k, v, do_, lens, causal, scale, layout, dtype)
            vs.check(got, res, name)
            vs.assert_dead_are_plus_zero(got, lens, layout, name)
    tn.set_default_float(np.float32)
