"""The host planner of the optimizer step (tinynn-autograd_amd/ostep.py): run merging, grid and workspace sizes, the
schedules against closed forms, the clip factor, the plan's route and launch list.  No device is touched."""

import math

import numpy as np
import pytest

from tinynn_autograd_amd import ostep


def test_adjacent_equal_flags_merge_and_empty_segments_drop():
    starts, flags = ostep.decay_runs([(0, 5), (5, 1), (6, 7)], [True, False, True])
    assert list(starts) == [0, 5, 6] and list(flags) == [1, 0, 1] and starts.dtype == flags.dtype == np.int64
    starts, flags = ostep.decay_runs([(0, 4), (4, 2), (6, 3), (9, 1)], [True, True, False, False])
    assert list(starts) == [0, 6] and list(flags) == [1, 0]
    # an empty segment between two equal neighbours does not split them, whatever its own flag
    starts, flags = ostep.decay_runs([(0, 4), (4, 0), (4, 2)], [True, False, True])
    assert list(starts) == [0] and list(flags) == [1]
    starts, flags = ostep.decay_runs([(0, 0), (0, 3)], [True, False])
    assert list(starts) == [0] and list(flags) == [0]


def test_a_single_run_and_no_element_at_all():
    starts, flags = ostep.decay_runs([(0, 9)], [False])
    assert list(starts) == [0] and list(flags) == [0]
    starts, flags = ostep.decay_runs([], [])
    assert list(starts) == [0] and list(flags) == [0]
    assert list(ostep.run_table([0, 5], [1, 0])) == [0, 5, 1, 0]
    np.testing.assert_array_equal(ostep.decay_vector(7, (np.array([0, 2, 5]), np.array([1, 0, 1])), 0.5),
                                  [0.5, 0.5, 0, 0, 0, 0.5, 0.5])


def test_segments_must_continue():
    with pytest.raises(ValueError, match="does not continue"):
        ostep.decay_runs([(0, 4), (5, 2)], [True, False])
    with pytest.raises(ValueError, match="segments"):
        ostep.decay_runs([(0, 4)], [True, False])


@pytest.mark.parametrize("n, groups", [(0, 0), (1, 1), (255, 1), (256, 1), (257, 1), (1024, 1), (1025, 2),
                                       (4 * 256 * 2048 + 5, 2048), (4 * 256 * 2048, 2048), (4 * 256 * 2047 + 1, 2048),
                                       (4 * 256 * 2047, 2047)])
def test_grid_and_workspace(n, groups):
    """A lane takes 4 elements, a workgroup 256 lanes, at most 2048 workgroups; one double of workspace per workgroup."""
    assert ostep.grid(n) == groups
    assert ostep.workspace_bytes(n) == 8 * groups
    plan = ostep.plan_ostep(n, np.float32, max_norm=1.0)
    assert plan.grid == groups and plan.workspace_bytes == 8 * groups
    assert ostep.plan_ostep(n, np.float64, max_norm=1.0).grid == groups          # a function of n alone


def test_schedules_against_closed_forms():
    base, warmup, total, min_lr = 3e-3, 4, 20, 1e-4
    cos, lin, const = ostep.Cosine(warmup, total, min_lr), ostep.Linear(warmup, total, min_lr), ostep.Constant()
    for sched in (cos, lin):
        assert sched.value(1, base) == base * 1 / 4
        assert sched.value(warmup, base) == base                                  # the warm-up ends exactly at base
        assert sched.value(total, base) == min_lr                                 # exactly: cos(pi) = -1, 1 - 1 = 0
        assert sched.value(total + 10, base) == sched.value(total, base)          # constant afterwards
    frac = 1.0 / 16.0
    assert cos.value(warmup + 1, base) == pytest.approx(min_lr + 0.5 * (base - min_lr) * (1 + math.cos(math.pi * frac)), rel=1e-15)
    assert lin.value(warmup + 1, base) == pytest.approx(base - (base - min_lr) * frac, rel=1e-15)
    assert cos.value(12, base) == pytest.approx(0.5 * (base + min_lr), rel=1e-15)  # half way: cos(pi / 2) = 0
    assert lin.value(12, base) == pytest.approx(0.5 * (base + min_lr), rel=1e-15)
    for t in (1, warmup, warmup + 1, total, total + 10):
        assert const.value(t, base) == base
    assert (cos.kind, lin.kind, const.kind) == (ostep.SCHED_COSINE, ostep.SCHED_LINEAR, ostep.SCHED_CONST)
    assert ostep.Cosine(0, 10).value(1, base) == pytest.approx(0.5 * base * (1 + math.cos(math.pi * 0.1)), rel=1e-15)
    with pytest.raises(ValueError):
        ostep.Cosine(-1, 10)


def test_clip_factor_is_exactly_one_when_nothing_is_clipped():
    assert ostep.clip_coef(0.0, 1.0) == 1.0
    assert ostep.clip_coef(0.0, 1e-9) < 1.0                 # torch's rule: the 1e-6 in the denominator counts
    assert ostep.clip_coef(3.0, 3.0 + 1e-6 + 1e-9) == 1.0   # max_norm > gnorm + 1e-6
    assert ostep.clip_coef(3.0, 3.0) < 1.0
    assert ostep.clip_coef(4.0, 1.0) == 1.0 / (4.0 + 1e-6)
    assert ostep.clip_coef(123.0, None) == 1.0
    assert ostep.clip_coef(float("inf"), 1.0) == 0.0
    hyper = ostep.Hyper(max_norm=10.0)
    st = ostep.begin(ostep.initial_state(1e-3), np.zeros(5, np.float32), hyper)
    assert st[ostep.GNORM] == 0.0 and st[ostep.COEF] == 1.0 and st[ostep.T] == 1 and st[ostep.SKIP] == 0


def test_the_record_and_the_skip_rule():
    st0 = ostep.initial_state(2e-3)
    assert list(st0) == [1, 1, 0, 2e-3, 0, 1, 0, 0] and st0.dtype == np.float64 and st0.size == ostep.STATE_DOUBLES
    assert ostep.STATE_NAMES == ("b1_pow", "b2_pow", "t", "lr", "gnorm", "coef", "skipped", "skip")
    hyper = ostep.Hyper(lr=2e-3, max_norm=1.0)
    bad = ostep.begin(st0, np.array([1.0, np.inf]), hyper)
    assert bad[ostep.SKIP] == 1 and bad[ostep.SKIPPED] == 1 and bad[ostep.T] == 0 and bad[ostep.B1_POW] == 1
    nan = ostep.begin(st0, np.array([1.0, np.nan]), hyper)
    assert nan[ostep.SKIP] == 1 and nan[ostep.T] == 0
    good = ostep.begin(bad, np.array([3.0, 4.0]), hyper)
    assert good[ostep.SKIP] == 0 and good[ostep.SKIPPED] == 1 and good[ostep.T] == 1 and good[ostep.GNORM] == 5.0
    assert good[ostep.B1_POW] == 0.9 and good[ostep.B2_POW] == 0.999
    p = np.arange(4, dtype=np.float32)
    out = ostep.reference(p, np.array([1, np.inf, 0, 0], np.float32), p * 0, p * 0, st0, hyper, ostep.decay_runs([(0, 4)], [True]))
    assert out[0].tobytes() == p.tobytes() and not out[1].any() and not out[2].any()
    unguarded = ostep.begin(st0, np.array([np.inf]), ostep.Hyper(max_norm=None, guard=False))
    assert unguarded[ostep.GNORM] == 0.0 and unguarded[ostep.SKIP] == 0            # no norm is taken at all


def test_plan_routes_and_launches():
    plan = ostep.plan_ostep(1000, np.float32, max_norm=1.0)
    assert plan.route == "native" and plan.launches == ("sumsq", "begin", "adamw") and plan.need_norm
    plan = ostep.plan_ostep(1000, np.float32, max_norm=None, skip_nonfinite=False)
    assert plan.launches == ("begin", "adamw") and not plan.need_norm and plan.workspace_bytes == 0
    assert ostep.plan_ostep(1000, np.float32, native=False).route == "composed"
    assert ostep.plan_ostep(1000, np.float16).route == "composed"
    assert ostep.plan_ostep(1000, np.float64, route="composed").route == "composed"
    assert ostep.plan_ostep(0, np.float32, max_norm=1.0).launches == ("begin",)
    with pytest.raises(ValueError, match="native optimizer-step route"):
        ostep.plan_ostep(1000, np.float32, native=False, route="native")
    with pytest.raises(ValueError, match="route must be"):
        ostep.plan_ostep(1000, route="fast")
    with pytest.raises(ValueError, match="max_norm"):
        ostep.plan_ostep(1000, max_norm=-1.0)
