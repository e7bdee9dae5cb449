"""The host planner of the normalisations (tinynn-autograd_amd/norm.py): folding of the leading axes, validation, the form
and route at the limits of the two kernel geometries, the empty plan and the backward workspace."""

import pytest

from tinynn_autograd_amd import norm as nm


def test_shapes_and_folding():
    p = nm.plan_norm((8,))
    assert (p.M, p.N, p.stats_shape, p.form, p.route) == (1, 8, (), "wave", "native")
    p = nm.plan_norm((5, 8), (8,), (1, 8))
    assert (p.M, p.N, p.stats_shape) == (5, 8, (5,)) and p.has_gamma and p.has_beta
    p = nm.plan_norm((2, 3, 4, 16), (1, 16), None, kind="rms", eps=1e-6)
    assert (p.M, p.N, p.stats_shape, p.kind, p.eps) == (24, 16, (2, 3, 4), "rms", 1e-6)
    assert p.has_gamma and not p.has_beta and p.x_shape == (2, 3, 4, 16)
    assert nm.KIND_CODE == {"layer": 0, "rms": 1} and nm.GELU_CODE == {"none": 0, "tanh": 1}


def test_validation_errors():
    with pytest.raises(ValueError, match="at least one axis"):
        nm.plan_norm(())
    with pytest.raises(ValueError, match="normalised axis is empty"):
        nm.plan_norm((4, 0))
    for bad in ((7,), (8, 1), (2, 8), (1, 1, 8)):
        with pytest.raises(ValueError, match="gamma must hold"):
            nm.plan_norm((4, 8), bad)
        with pytest.raises(ValueError, match="beta must hold"):
            nm.plan_norm((4, 8), (8,), bad)
    for eps in (-1e-9, float("inf"), float("nan"), "small"):
        with pytest.raises(ValueError, match="eps must be"):
            nm.plan_norm((4, 8), eps=eps)
    assert nm.plan_norm((4, 8), eps=0).eps == 0.0
    with pytest.raises(ValueError, match="kind must be"):
        nm.plan_norm((4, 8), kind="batch")
    with pytest.raises(ValueError, match="RMS norm takes no beta"):
        nm.plan_norm((4, 8), (8,), (8,), kind="rms")
    with pytest.raises(ValueError, match="route must be"):
        nm.plan_norm((4, 8), route="quick")


def test_form_and_route_at_the_limits():
    assert nm.WAVE_MAX_N < nm.BLOCK_MAX_N
    for n, form, route in ((nm.WAVE_MAX_N - 1, "wave", "native"), (nm.WAVE_MAX_N, "wave", "native"),
                           (nm.WAVE_MAX_N + 1, "block", "native"), (nm.BLOCK_MAX_N - 1, "block", "native"),
                           (nm.BLOCK_MAX_N, "block", "native"), (nm.BLOCK_MAX_N + 1, "block", "composed")):
        p = nm.plan_norm((3, n))
        assert (p.form, p.route) == (form, route), n
        assert p.rows_per_block() == (nm.ROWS_PER_BLOCK if form == "wave" else 1)
    assert nm.plan_norm((3, 8), route="composed").route == "composed"
    assert nm.plan_norm((3, 8), native=False).route == "composed"
    assert nm.plan_norm((3, 8), float_ok=False).route == "composed"
    for kwargs in (dict(native=False), dict(float_ok=False)):
        with pytest.raises(ValueError, match="native normalisation route"):
            nm.plan_norm((3, 8), route="native", **kwargs)
    with pytest.raises(ValueError, match="native normalisation route"):
        nm.plan_norm((3, nm.BLOCK_MAX_N + 1), route="native")


def test_empty_plan():
    for shape in ((0, 8), (3, 0, 8)):
        p = nm.plan_norm(shape)
        assert p.empty() and p.M == 0 and p.stats_shape == shape[:-1]
        assert p.workspace_bytes(4, True, True) == 0
    assert not nm.plan_norm((1, 8)).empty()


def test_backward_partials_and_workspace():
    r = nm.ROWS_PER_BLOCK
    assert nm.plan_norm((1, 8)).partials() == 1
    assert nm.plan_norm((r, 8)).partials() == 1
    assert nm.plan_norm((r + 1, 8)).partials() == 2
    assert nm.plan_norm((r * nm.MAX_PARTIALS + 1, 8)).partials() == nm.MAX_PARTIALS
    assert nm.plan_norm((5, nm.WAVE_MAX_N + 1)).partials() == 5
    assert nm.plan_norm((nm.MAX_PARTIALS + 7, nm.WAVE_MAX_N + 1)).partials() == nm.MAX_PARTIALS
    p = nm.plan_norm((9, 12))
    assert p.workspace_bytes(4, True, True) == 2 * 3 * 12 * 4
    assert p.workspace_bytes(8, True, False) == 3 * 12 * 8
    assert p.workspace_bytes(4, False, False) == 0


def test_gelu_forms_and_routes():
    assert nm.gelu_route("none") == "native" and nm.gelu_route("tanh") == "native"
    assert nm.gelu_route("tanh", native=False) == "composed" and nm.gelu_route("tanh", route="composed") == "composed"
    for kwargs in (dict(native=False), dict(route="composed"), dict(float_ok=False)):
        with pytest.raises(ValueError, match="exact .erf. GELU needs the native route"):
            nm.gelu_route("none", **kwargs)
    with pytest.raises(ValueError, match="native GELU route"):
        nm.gelu_route("tanh", native=False, route="native")
    with pytest.raises(ValueError, match="approximate must be"):
        nm.gelu_route("sigmoid")
    with pytest.raises(ValueError, match="route must be"):
        nm.gelu_route("tanh", route="quick")
