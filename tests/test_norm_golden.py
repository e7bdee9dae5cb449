"""tests/golden/norm_cases.npz (written by tests/gen_norm_golden.py, where every value is cross-checked against torch in
float64) against the numpy oracle of tests/norm_oracle.py: the oracle the other tests trust reproduces the fixture, its
GELU slope agrees with a central difference, and its bounds meet their own tightness gate on every case."""

import os

import numpy as np
import pytest

import norm_oracle as no

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "norm_cases.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as data:
        return dict(data)


def test_fixture_is_complete_and_small(golden):
    wanted = set(no.NORM_CASES) | set(no.GELU_CASES) | {"block.params", "block.grads", "block.loss", "block.adam_losses",
                                                          "block.f32_gate", "block.grad_scale"}
    assert set(golden) == wanted
    attn = os.path.join(os.path.dirname(GOLDEN), "attn_cases.npz")
    assert os.path.getsize(GOLDEN) < os.path.getsize(attn)


@pytest.mark.parametrize("name", sorted(no.NORM_CASES))
def test_oracle_reproduces_the_norm_cases(golden, name):
    x, gamma, beta, dy, kind, eps = no.case_input(name)
    res = no.reference(x, gamma, beta, dy, kind, eps)
    stored = no.unpack(golden[name], no.case_fields(name))
    assert [f for f, _ in no.case_fields(name)] == [f for f in no.FIELDS if res.values[f] is not None]
    for field, want in stored.items():
        np.testing.assert_allclose(res.values[field].reshape(want.shape), want, rtol=1e-12, atol=1e-12 * np.abs(want).max(),
                                   err_msg="%s %s" % (name, field))


@pytest.mark.parametrize("name", sorted(no.NORM_CASES))
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_bounds_meet_the_tightness_gate(golden, name, dtype):
    """The stored values lie within their own bounds (trivially) AND the bounds pass the median gate: every fixture case is
    a case the bounds can judge."""
    x, gamma, beta, dy, kind, eps = no.case_input(name, dtype)
    res = no.reference(x, gamma, beta, dy, kind, eps, dtype)
    no.check({f: res.values[f] for f in no.FIELDS}, res, "%s %s" % (name, np.dtype(dtype).name))


@pytest.mark.parametrize("name", sorted(no.GELU_CASES))
def test_oracle_reproduces_the_gelu_cases(golden, name):
    form = no.GELU_CASES[name]
    x, dy = no.gelu_input(40, no.case_seed(name))
    res = no.gelu_reference(x, dy, form)
    np.testing.assert_allclose(np.stack([res.values["y"], res.values["dx"]]), golden[name], rtol=1e-12, atol=1e-300)
    # the analytic slope against a float64 central difference: truncation h^2 / 6 max|f'''| (|f'''| < 2), rounding u64 |f| / h
    h = 1e-5
    x64 = x.astype(np.float64)
    cd = (no.gelu64(x64 + h, form) - no.gelu64(x64 - h, form)) / (2 * h)
    tol = h * h / 3 + 4 * no.U64 * (np.abs(x64) + 1) / h
    assert (np.abs(cd * dy - res.values["dx"]) <= np.abs(dy) * tol).all()
    for dtype in (np.float32, np.float64):
        r = no.gelu_reference(x, dy, form, dtype)
        no.check(r.values, r, "%s %s" % (name, np.dtype(dtype).name), fields=("y", "dx"))


def test_oracle_reproduces_the_block_case(golden):
    c = no.BLOCK_CASE
    params = no.block_initial()
    np.testing.assert_array_equal(no.pack(params, no.block_layout()), golden["block.params"].astype(np.float64))
    assert golden["block.params"].dtype == np.float16
    x, y = no.block_data()
    loss, grads, bk_terms = no.block_loss_and_grads(params, x, y, c["H"], c["causal"], c["eps"], with_bk_terms=True)
    np.testing.assert_allclose(loss, float(golden["block.loss"]), rtol=1e-12)
    stored = no.unpack(golden["block.grads"], no.block_layout())
    assert list(stored) == list(no.BLOCK_NAMES)
    for name, scale in zip(no.BLOCK_NAMES, golden["block.grad_scale"]):
        assert np.abs(grads[name] - stored[name]).max() <= 1e-11 * scale, name
        if name != "attn.bk":
            assert scale == np.abs(stored[name]).max()
    np.testing.assert_allclose(golden["block.grad_scale"][no.BLOCK_NAMES.index("attn.bk")], bk_terms.max(), rtol=1e-12)
    assert np.abs(stored["attn.bk"]).max() < 1e-12 * golden["block.grad_scale"][no.BLOCK_NAMES.index("attn.bk")]
    losses = no.block_adam_losses(params, x, y, c["H"], c["causal"], c["eps"], c["lr"], c["steps"])
    np.testing.assert_allclose(losses, golden["block.adam_losses"], rtol=1e-9)
    assert losses[0] == loss and (np.diff(golden["block.adam_losses"]) < 0).all()
    gates = golden["block.f32_gate"]
    assert gates.shape == (len(no.BLOCK_NAMES),) and (gates > 0).all() and (gates < 1e-5).all()
