"""varlen.py, the host planner of attention with per-sequence lengths: its constants are the headers', the refusals (Tq != Tk,
a wrong lens shape, "bhtd" with four axes), what it carries (the group, the wrapped plan's strides and shapes) and the routes."""

import os
import re

import numpy as np
import pytest

from conftest import ROOT
from tinynn_autograd_amd import attention as at, gqa as gq, varlen as vl


def define(name, header):
    text = open(os.path.join(ROOT, "include", header)).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))


def test_the_constants_are_the_headers():
    assert vl.MAX_GROUP == define("TNN_VARLEN_MAX_GROUP", "tnn_varlen.h") == define("TNN_GQA_MAX_GROUP", "tnn_gqa.h") == gq.MAX_GROUP
    assert vl.MAX_HEAD_DIM == define("TNN_ATTN_MAX_HEAD_DIM", "tnn_attn.h")
    assert vl.BLOCK == define("TNN_ATTN_BLOCK_Q", "tnn_attn.h") == define("TNN_ATTN_BLOCK_K", "tnn_attn.h")
    assert vl.ROUTES == at.ROUTES


def test_refusals():
    q, k, v = (2, 9, 4, 8), (2, 9, 4, 8), (2, 9, 4, 6)
    with pytest.raises(ValueError, match="Tq == Tk"):
        vl.plan_varlen(q, (2, 10, 4, 8), (2, 10, 4, 6), (2,))
    with pytest.raises(ValueError, match="Tq == Tk"):
        vl.plan_varlen(q, (2, 10, 2, 8), (2, 10, 2, 6), (2,), grouped=True)
    for bad in ((3,), (2, 1), (), (1, 2)):
        with pytest.raises(ValueError, match=r"lens must have shape \(B,\)"):
            vl.plan_varlen(q, k, v, bad)
    with pytest.raises(ValueError, match="exactly three axes"):
        vl.plan_varlen((2, 4, 9, 8), (2, 4, 9, 8), (2, 4, 9, 6), (2,), layout="bhtd")
    with pytest.raises(ValueError, match="exactly three axes"):
        vl.plan_varlen((9, 8), (9, 8), (9, 6), (1,), layout="bhtd")
    with pytest.raises(ValueError, match="exactly three axes"):
        vl.plan_varlen((2, 9, 8), (2, 9, 8), (2, 9, 6), (2,), layout="bhtd", grouped=True)
    with pytest.raises(ValueError, match="layout must be one of"):
        vl.plan_varlen(q, k, v, (2,), layout="tbhd")
    with pytest.raises(ValueError, match="route must be one of"):
        vl.plan_varlen(q, k, v, (2,), route="fast")
    with pytest.raises(ValueError, match="no multiple"):
        vl.plan_varlen(q, (2, 9, 3, 8), (2, 9, 3, 6), (2,), grouped=True)


def test_what_the_plan_carries():
    p = vl.plan_varlen((3, 70, 4, 16), (3, 70, 2, 16), (3, 70, 2, 24), (3,), causal=True, grouped=True)
    assert (p.T, p.group, p.grouped, p.Hkv, p.route) == (70, 2, True, 2, "native")
    assert p.geometry() == (3, 4, 70, 70, 16, 24)                   # H counts the QUERY heads; the group goes separately
    assert p.out_shape == (3, 70, 4, 24) and p.lse_shape == (3, 4, 70) and p.causal and not p.empty()
    assert p.strides("k") == list(at._strides("bthd", 2, 70, 16))   # the head stride of k steps over key / value heads
    plain = vl.plan_varlen((3, 70, 4, 16), (3, 70, 4, 16), (3, 70, 4, 24), (3,))
    assert (plain.group, plain.grouped, plain.route) == (1, False, "native")
    three = vl.plan_varlen((5, 13, 8), (5, 13, 8), (5, 13, 6), (5,), layout="bhtd")
    assert (three.B, three.H, three.T, three.lse_shape) == (5, 1, 13, (5, 13))
    assert three.strides("q", "o") == [13 * 8, 13 * 8, 8, 13 * 6, 13 * 6, 6]


def test_routing():
    q, k, v = (2, 9, 16, 8), (2, 9, 1, 8), (2, 9, 1, 6)
    assert vl.plan_varlen(q, k, v, (2,), grouped=True).route == "composed"                # group 16 > MAX_GROUP
    with pytest.raises(ValueError, match="native gqa_attention route with lens="):
        vl.plan_varlen(q, k, v, (2,), grouped=True, route="native")
    sq = (2, 9, 4, 8)
    assert vl.plan_varlen(sq, sq, sq, (2,), native=False).route == "composed"
    assert vl.plan_varlen(sq, sq, sq, (2,), float_ok=False).route == "composed"
    assert vl.plan_varlen(sq, sq, sq, (2,), route="composed").route == "composed"
    wide = (2, 9, 4, 129)
    assert vl.plan_varlen(wide, wide, wide, (2,)).route == "composed"
    with pytest.raises(ValueError, match="native attention route with lens="):
        vl.plan_varlen(sq, sq, sq, (2,), native=False, route="native")


def test_host_helpers():
    with pytest.raises(ValueError, match=r"outside \[0, T = 9\]"):
        vl.check_lens([3, 10], 9)
    with pytest.raises(ValueError, match=r"outside \[0, T = 9\]"):
        vl.check_lens([-1, 2], 9)
    assert vl.check_lens([0, 9], 9).tolist() == [0, 9]
    keys, rows = vl.key_mask([2, 0], 3, 2, np.float32), vl.row_mask([2, 0], 3, 2, np.float32)
    assert keys.shape == (4, 3, 3) and rows.shape == (4, 3, 1)
    assert keys[0].tolist() == [[0, 0, -np.inf], [0, 0, -np.inf], [0, 0, 0]] and np.array_equal(keys[0], keys[1])
    assert not keys[2:].any() and rows[:, :, 0].tolist() == [[1, 1, 0]] * 2 + [[0, 0, 0]] * 2       # a dead row stays unmasked
    assert vl.live_blocks([130, 64, 65, 0], 130, True) == (6 + 1 + 3 + 0, 4 * 6)
    assert vl.live_blocks([130, 64, 65, 0], 130, False) == (9 + 1 + 4 + 0, 4 * 9)
