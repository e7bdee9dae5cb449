"""The optimizer step against torch: tests/golden/ostep_cases.npz holds what torch.nn.utils.clip_grad_norm_ followed by
torch.optim.AdamW computes on the CPU in float64 (tests/gen_ostep_golden.py; torch is imported only there).  The independent
oracle (tests/ostep_oracle.py) and the planner's reference (tinynn-autograd_amd/ostep.py) must each reproduce it.

Tolerances.  All three evaluate the same formulas in float64 and differ only in the ORDER of a handful of roundings per step
(torch folds the bias corrections into a step size and a scaled root, the planner multiplies by reciprocals): a few 2^-53
relative per step.  1e-12 of each tensor's max-norm covers 5 steps with room; the norms, one sum and one root, agree within
1e-14 relative."""

import os

import numpy as np
import pytest

import ostep_oracle as oo
from tinynn_autograd_amd import ostep

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ostep_cases.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as data:
        return {k: data[k] for k in data.files}


def split(flat, sizes):
    out, off = [], 0
    for s in sizes:
        out.append(flat[off:off + int(s)])
        off += int(s)
    return out


def check(got, want, sizes, what):
    for i, (a, b) in enumerate(zip(split(got, sizes), split(want, sizes))):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-12 * np.abs(b).max(), err_msg="%s, parameter %d" % (what, i))


def test_the_fixture_is_small_and_complete(golden):
    assert os.path.getsize(GOLDEN) < 100 * 1024
    assert list(golden["sizes"]) == [5, 1, 7] and list(golden["decay"]) == [True, False, True]
    assert sorted(golden["case_names"]) == ["clip_nowd", "clip_wd", "noclip_nowd", "noclip_wd"]
    for name in golden["case_names"]:
        norms, max_norm = golden[name + ".norms"], float(golden[name + ".max_norm"])
        assert golden[name + ".params"].shape == (5, 13) and norms.shape == (5,)
        assert (norms > max_norm).all() if name.startswith("clip") else (norms < max_norm).all()
    assert {float(golden[n + ".wd"]) for n in golden["case_names"]} == {0.0, 0.1}


def test_the_oracle_reproduces_torch(golden):
    sizes, decay = golden["sizes"], list(golden["decay"])
    lr, b1, b2, eps = golden["hyper"]
    for name in golden["case_names"]:
        params, state = split(golden["p0"], sizes), None
        state = oo.new_state(params)
        for s in range(5):
            params = oo.adamw_step(params, split(golden["grads"][s], sizes), state, decay, lr=lr, b1=b1, b2=b2, eps=eps,
                                   wd=float(golden[name + ".wd"]), max_norm=float(golden[name + ".max_norm"]))
            check(np.concatenate(params), golden[name + ".params"][s], sizes, "%s step %d" % (name, s + 1))
            np.testing.assert_allclose(state["gnorm"], golden[name + ".norms"][s], rtol=1e-14, atol=0)
        assert state["t"] == 5 and state["skipped"] == 0


def test_the_planner_reference_reproduces_torch(golden):
    sizes, decay = golden["sizes"], list(golden["decay"])
    lr, b1, b2, eps = golden["hyper"]
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    runs = ostep.decay_runs(list(zip(offsets, sizes)), decay)
    assert list(runs[0]) == [0, 5, 6] and list(runs[1]) == [1, 0, 1]
    for name in golden["case_names"]:
        hyper = ostep.Hyper(lr=lr, b1=b1, b2=b2, eps=eps, wd=float(golden[name + ".wd"]),
                            max_norm=float(golden[name + ".max_norm"]))
        p = golden["p0"].copy()
        m, v, state = np.zeros_like(p), np.zeros_like(p), ostep.initial_state(lr)
        for s in range(5):
            p, m, v, state = ostep.reference(p, golden["grads"][s], m, v, state, hyper, runs)
            check(p, golden[name + ".params"][s], sizes, "%s step %d" % (name, s + 1))
            np.testing.assert_allclose(state[ostep.GNORM], golden[name + ".norms"][s], rtol=1e-14, atol=0)
            clipped = name.startswith("clip")
            assert (state[ostep.COEF] < 1.0) == clipped
        assert state[ostep.T] == 5 and state[ostep.SKIPPED] == 0 and state[ostep.SKIP] == 0
        assert state[ostep.B1_POW] == pytest.approx(b1 ** 5, rel=1e-15) and state[ostep.B2_POW] == pytest.approx(b2 ** 5, rel=1e-15)
