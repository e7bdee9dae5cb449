"""The committed fixture tests/golden/extend_cases.npz against its generator's oracle and against the composed route (the
one the CPU test twin takes): regenerating the inputs from their seeds reproduces the stored float64 results, and the
composed attention_extend lies within the derived bounds of them in both dtypes."""

import numpy as np
import pytest

import attn_oracle as ao
import extend_oracle as eo
import extend_support as es
import tinynn_autograd_amd as tn


@pytest.fixture(scope="module")
def golden():
    return es.load_golden()


def test_the_fixture_holds_every_case_and_the_oracle_reproduces_it(golden):
    assert sorted(golden) == sorted("extend." + name for name in eo.EXTEND_CASES)
    for name in eo.EXTEND_CASES:
        res = es.reference(eo.extend_case(name, np.float32), np.float32)
        assert golden["extend." + name].dtype == np.float64
        np.testing.assert_allclose(res.values["o"], golden["extend." + name], rtol=1e-13, atol=0)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", sorted(eo.EXTEND_CASES))
def test_the_composed_route_within_the_bounds(golden, name, dtype):
    tn.set_default_float(dtype)
    case = eo.extend_case(name, np.float32)
    res = es.reference(case, dtype)
    o, kc, vc = es.run_extend("composed", case, dtype)
    assert o.dtype == dtype and o.shape == golden["extend." + name].shape and np.isfinite(o).all()
    ao.assert_within(o, golden["extend." + name], res.bounds["o"], "%s composed" % name)
    want_k, want_v = es.expected_caches(case, dtype)
    assert np.array_equal(es.bits(kc), es.bits(want_k)) and np.array_equal(es.bits(vc), es.bits(want_v))
