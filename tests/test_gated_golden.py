"""The gated oracle (tests/gated_oracle.py) reproduces tests/golden/gated_cases.npz, which tests/gen_gated_golden.py wrote
from it — the yardstick has not moved — and the composed route of device_array.gated / gated_bwd meets the derived bounds on
every case that has a composed form."""

import numpy as np
import pytest

import gated_oracle as go
import gated_support as gs


@pytest.fixture(scope="module")
def golden():
    return gs.load_golden()


def test_the_fixture_holds_every_case(golden):
    names = {"%s.%s" % (name, field) for name, c in go.GOLDEN_CASES.items() for field in ("y", "dgate", "dup")
             if field != "dup" or c[3]}
    assert names == set(golden)
    assert list(go.GOLDEN_CASES.values()) == [("silu", 3, 5, True), ("silu", 2, 8, True), ("silu", 4, 3, False),
                                              ("gelu_tanh", 3, 5, True), ("gelu_tanh", 2, 4, False), ("gelu", 3, 5, True)]


@pytest.mark.parametrize("name", sorted(go.GOLDEN_CASES))
def test_the_oracle_reproduces_the_fixture(golden, name):
    """To 2^-50 relative: the fixture stores the oracle's values rounded to float64."""
    act, M, F, with_up = go.GOLDEN_CASES[name]
    gate, up, dy = go.make_inputs(M, F, go.case_seed(name), np.float32)
    assert np.array_equal(gate.reshape(-1)[:8], go.SPECIALS.astype(np.float32)) and np.signbit(gate.reshape(-1)[1])
    res = go.reference(gate, up if with_up else None, dy, act, np.float32)
    for field in ("y", "dgate", "dup"):
        if res.values[field] is None:
            assert field == "dup" and not with_up
            continue
        want = golden["%s.%s" % (name, field)]
        assert want.shape == (M, F) and want.dtype == np.float64
        assert (np.abs(res.values[field] - want) <= 2.0 ** -50 * np.abs(want)).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", sorted(go.GOLDEN_CASES))
def test_the_composed_route_meets_the_fixture(golden, name, dtype):
    act, M, F, with_up = go.GOLDEN_CASES[name]
    gate, up, dy = go.make_inputs(M, F, go.case_seed(name), dtype)
    up = up if with_up else None
    if act == "gelu":                                    # no erf among the generic operations: the composed route says so
        with pytest.raises(ValueError, match="exact \\(erf\\) GELU gate needs the native route"):
            gs.composed(act, dtype, gate, up, dy)
        return
    res = go.reference(gate, up, dy, act, dtype)
    for field in ("y", "dgate", "dup"):                  # the oracle is the fixture's (float32 numbers in either dtype)
        if res.values[field] is not None:
            assert (np.abs(res.values[field] - golden["%s.%s" % (name, field)]) <= 2.0 ** -50 * np.abs(res.values[field])).all()
    got = gs.composed(act, dtype, gate, up, dy)
    assert all(got[f] is None or got[f].dtype == dtype for f in got)
    # the composed route rounds every operation once but evaluates sig = 1 / (1 + exp(-g)) without the branch and the slope
    # without the fma: one more rounding than the fixed expression, which the factor 2 covers
    go.check(got, res, "%s %s composed" % (name, np.dtype(dtype).name), factor=2.0)
    assert np.isfinite(got["y"]).all() and np.isfinite(got["dgate"]).all()
