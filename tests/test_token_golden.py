"""tests/token_oracle.py against the fixture tests/golden/token_cases.npz (written by tests/gen_token_golden.py, where every
case was cross-checked against torch in float64), the analytic gradients against central differences, and the tightness
condition of the derived bounds on the inputs the other tests use."""

import numpy as np
import pytest

import token_oracle as to
import token_support as ts


@pytest.fixture(scope="module")
def golden():
    return ts.load_golden()


@pytest.mark.parametrize("name", sorted(to.EMBED_CASES))
def test_embedding_cases(golden, name):
    inputs = to.embed_case(name)
    res = to.embedding_reference(*inputs)
    want = to.unpack(golden[name], to.embed_fields(name))
    for field, _ in to.embed_fields(name):
        np.testing.assert_allclose(res.values[field], want[field], rtol=1e-13, atol=1e-13)
    table, ids, pos, dy, padding_idx = inputs
    if pos is None:
        assert not res.bounds["out"].any()                       # bit-exact without positions
    if padding_idx is not None:
        assert (ids == padding_idx).any() and not res.values["dtable"][padding_idx].any()


def test_repeated_ids_accumulate():
    table, ids, pos, dy, _ = to.embed_case("embed_repeat")
    assert ids.tolist() == [3, 1, 3, 3]
    d = to.embedding_reference(table, ids, None, dy).values["dtable"]
    np.testing.assert_allclose(d[3], dy[0].astype(np.float64) + dy[2] + dy[3], rtol=1e-15)
    np.testing.assert_array_equal(d[1], dy[1])
    assert not d[[0, 2, 4]].any()


@pytest.mark.parametrize("name", sorted(to.XENT_CASES))
def test_cross_entropy_cases(golden, name):
    x, t, ignore_index, reduction, g = to.xent_case(name)
    res = to.cross_entropy_reference(x, t, ignore_index, reduction, g)
    want = to.unpack(golden[name], to.xent_fields(name))
    for field, _ in to.xent_fields(name):
        np.testing.assert_allclose(res.values[field], want[field], rtol=1e-13, atol=1e-13)
    m, _, _, _, _, _, ignored = to.XENT_CASES[name]
    assert res.values["count"] == m - len(ignored)
    assert not res.values["dlogits"][list(ignored)].any() and not res.values["losses"][list(ignored)].any()
    if len(ignored) == m:
        assert res.values["loss"] == 0.0


@pytest.mark.parametrize("name", ["xent_small", "xent_sum_g", "xent_ignore", "xent_neg_inf"])
def test_analytic_gradient_against_central_differences(name):
    x, t, ignore_index, reduction, g = to.xent_case(name, np.float64)
    dl = to.cross_entropy_reference(x, t, ignore_index, reduction, g, np.float64).values["dlogits"]
    h = 1e-5
    for r, c in [(0, 0), (1, 2), (x.shape[0] - 1, x.shape[1] - 1)]:
        if not np.isfinite(x[r, c]):
            assert dl[r, c] == 0.0
            continue
        hi, lo = x.copy(), x.copy()
        hi[r, c] += h
        lo[r, c] -= h
        cd = g * (to.loss64(hi, t, ignore_index, reduction) - to.loss64(lo, t, ignore_index, reduction)) / (2 * h)
        assert abs(cd - dl[r, c]) <= 1e-8 * max(1.0, abs(g))


def test_language_model_case(golden):
    params = to.unpack(golden["lm.params"].astype(np.float64), to.lm_layout())
    assert all(np.array_equal(params[n], to.lm_initial()[n].astype(np.float64)) for n in to.LM_NAMES)
    ids, targets = to.lm_data()
    np.testing.assert_array_equal(ids, golden["lm.ids"])
    np.testing.assert_array_equal(to.lm_targets(targets), golden["lm.targets"])
    assert (np.bincount(ids.reshape(-1)) > 1).any()              # ids repeat: the table's gradient must accumulate
    loss, grads = to.lm_loss_and_grads(params, ids, golden["lm.targets"])
    np.testing.assert_allclose(loss, float(golden["lm.loss"]), rtol=1e-12)
    ref = to.unpack(golden["lm.grads"], to.lm_layout())
    for name, scale in zip(to.LM_NAMES, golden["lm.grad_scale"]):
        assert np.abs(grads[name] - ref[name]).max() <= 1e-11 * scale, name
    assert (golden["lm.f32_gate"] < 1e-5).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_bounds_are_tight_on_the_inputs_the_tests_use(dtype):
    """The MEDIAN_GATE condition, checked against the oracle's own values (error 0): the widest row, the offset rows, and the
    largest sums of the embedding tests."""
    rs = np.random.RandomState(0)
    for m, v, offset, rescales in ((3, 1025, 0.0, 3), (5, 2 * 4096 + 37, 0.0, 7), (5, 65, 1000.0, 0), (4, 2, 0.0, 0)):
        x, t = to.xent_inputs(rs, m, v, offset, dtype=dtype)
        res = to.cross_entropy_reference(x, t, None, "mean", 1.0, dtype, rescales=rescales)
        to.check(res.values, res, "M%d V%d" % (m, v), fields=("lse", "losses", "loss", "dlogits"))
    table, pos, dy = to.embed_inputs(rs, 7, 5, (3, 300), 300, dtype)
    ids = rs.randint(0, 7, (3, 300))
    res = to.embedding_reference(table, ids, pos, dy, None, dtype)
    to.check(res.values, res, "embedding", fields=("out", "dtable", "dpos"))
