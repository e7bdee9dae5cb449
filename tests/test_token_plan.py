"""tokens.py, the numpy-only planner of the embedding and the per-row cross-entropy: extents, the forms at their limits,
workspace sizes, routes and errors."""

import numpy as np
import pytest

from tinynn_autograd_amd import tokens as tk


def test_embedding_extents_fold_the_leading_axes():
    p = tk.plan_embedding((11, 6), (2, 3, 5))
    assert (p.M, p.V, p.E, p.T, p.has_pos, p.padding_idx) == (30, 11, 6, 1, False, -1)
    assert p.out_shape == (2, 3, 5, 6) and p.route == "native" and not p.empty()
    p = tk.plan_embedding((11, 6), (4, 5), pos_shape=(8, 6), padding_idx=np.int64(3))
    assert (p.M, p.T, p.has_pos, p.padding_idx) == (20, 5, True, 3)            # T is the LAST extent of ids
    assert tk.plan_embedding((11, 6), ()).M == 1 and tk.plan_embedding((11, 6), (0, 4)).empty()
    assert tk.plan_embedding((11, 6), (0, 4)).workspace_bytes(4) == 0


def test_embedding_workspace_and_partial_counts():
    k, r = tk.EMBED_SEGMENT, tk.EMBED_VOCAB_PER_BLOCK
    for m, segments in ((1, 1), (k, 1), (k + 1, 2), (4 * k + 1, 5)):
        assert tk.plan_embedding((3, 5), (m,)).segments() == segments
    for v, blocks in ((1, 1), (r, 1), (r + 1, 2)):
        assert tk.plan_embedding((v, 2), (3,)).placement_blocks() == blocks
    p = tk.plan_embedding((7, 5), (k + 1,))
    assert p.workspace_bytes(4) == 32 + 32 + 272 + 2 * 2 * 5 * 4         # counts, offsets, sorted, 4 partial rows of 20 bytes
    assert p.workspace_bytes(8) == 32 + 32 + 272 + 160
    assert all(tk.plan_embedding((v, e), (m,)).workspace_bytes(s) % 16 == 0
               for v in (1, 2, 7) for e in (1, 3) for m in (1, 3, 257) for s in (4, 8))


def test_embedding_errors():
    for bad in ((5,), (0, 4), (4, 0), (2, 3, 4)):
        with pytest.raises(ValueError, match="table must be"):
            tk.plan_embedding(bad, (3,))
    with pytest.raises(ValueError, match="pos must be"):
        tk.plan_embedding((5, 4), (2, 3), pos_shape=(3, 5))
    with pytest.raises(ValueError, match="pos holds 2 rows"):
        tk.plan_embedding((5, 4), (2, 3), pos_shape=(2, 4))
    with pytest.raises(ValueError, match="at least one axis"):
        tk.plan_embedding((5, 4), (), pos_shape=(2, 4))
    for bad in (5, -1):
        with pytest.raises(ValueError, match="padding_idx"):
            tk.plan_embedding((5, 4), (3,), padding_idx=bad)
    with pytest.raises(ValueError, match="padding_idx must be an integer"):
        tk.plan_embedding((5, 4), (3,), padding_idx=1.5)
    with pytest.raises(ValueError, match="below 2\\^31"):
        tk.plan_embedding((5, 4), (1 << 31,))


def test_cross_entropy_forms_at_the_limit():
    w = tk.XENT_WAVE_MAX_V
    for v, form in ((1, "wave"), (w - 1, "wave"), (w, "wave"), (w + 1, "block"), (1 << 20, "block")):
        p = tk.plan_cross_entropy((3, v), (3,))
        assert p.form == form and p.rows_per_block() == (tk.XENT_ROWS_PER_BLOCK if form == "wave" else 1)
    step = tk.XENT_BLOCK_STEP
    assert tk.plan_cross_entropy((3, w), (3,)).steps(4) == 1
    assert [tk.plan_cross_entropy((1, v), (1,)).steps(4) for v in (w + 1, step, step + 1, 2 * step + 37)] == [1, 1, 2, 3]
    assert tk.plan_cross_entropy((1, 2 * step + 37), (1,)).steps(8) == 5          # float64: half the columns per step
    p = tk.plan_cross_entropy((2, 3, 4, 9), (2, 3, 4), ignore_index=7, reduction="sum")
    assert (p.M, p.V, p.ignore_index, p.reduction, p.rows_shape) == (24, 9, 7, "sum", (2, 3, 4))
    assert tk.plan_cross_entropy((9,), ()).M == 1 and tk.plan_cross_entropy((0, 9), (0,)).empty()
    assert tk.plan_cross_entropy((2, 9), (2,)).ignore_index == -1                  # None: no class is ignored


def test_cross_entropy_errors():
    with pytest.raises(ValueError, match="at least one class"):
        tk.plan_cross_entropy((), ())
    with pytest.raises(ValueError, match="at least one class"):
        tk.plan_cross_entropy((3, 0), (3,))
    with pytest.raises(ValueError, match="targets must have shape"):
        tk.plan_cross_entropy((3, 4), (3, 1))
    with pytest.raises(ValueError, match="reduction must be"):
        tk.plan_cross_entropy((3, 4), (3,), reduction="none")
    with pytest.raises(ValueError, match="ignore_index must be an integer"):
        tk.plan_cross_entropy((3, 4), (3,), ignore_index=0.5)


@pytest.mark.parametrize("plan", [lambda **kw: tk.plan_embedding((5, 4), (3,), **kw),
                                  lambda **kw: tk.plan_cross_entropy((3, 4), (3,), **kw)])
def test_routes(plan):
    assert tk.ROUTES == ("native", "composed")
    assert plan().route == "native" and plan(native=False).route == "composed" and plan(float_ok=False).route == "composed"
    assert plan(route="composed").route == "composed" and plan(native=False, route="composed").route == "composed"
    with pytest.raises(ValueError, match="route must be"):
        plan(route="quick")
    for kw in (dict(native=False), dict(float_ok=False)):
        with pytest.raises(ValueError, match="needs libtnn_hip.so and float32 / float64"):
            plan(route="native", **kw)
