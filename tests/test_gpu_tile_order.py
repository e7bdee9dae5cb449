"""`pytest -m gpu`: the launches whose workgroups find their tile through csrc/tnn_tile_order.h, through the ABI, at every branch
of the order: tile grids cut 1 x 8, 2 x 4 (with a power-of-two and with an odd rectangle height), not cut at all, ragged, and
the MNIST step's own grids.  tests/test_tile_order.py proves the map equal to the division formulas on the host; here the kernels
run with the host-filled argument blocks (GemmArgs::ord / GemmArgs::f, HeadBwdArgs::ord_dw / ord_dx).  The checks, float64 bounds
and sentinel guards are those of tests/test_gpu_step_prologues.py, whose case functions this file calls: a workgroup sent to the
wrong tile leaves sentinels where its tile should be (C, head_z) or errors of the size of the result itself (dW1, dx)."""

import os
import subprocess
import sys

import numpy as np
import pytest

import tinynn_autograd_amd as tn
import test_gpu_step_prologues as sp
from conftest import ROOT

# (M, N): the 16 x 16 tile grid and the cut pick_xcd_cut gives it
FWD_GRIDS = [(16, 128),     # 1 x 8 tiles: cut 1 x 8
             (32, 64),      # 2 x 4: cut 2 x 4
             (96, 64),      # 6 x 4: cut 2 x 4 with rectangles of 3 tile rows — no power of two
             (48, 80),      # 3 x 5: no cut
             (128, 256),    # 8 x 16: the MNIST first layer's grid
             (17, 40)]      # ragged 2 x 3: no cut


def _fwd(M, N, K):
    rs = np.random.RandomState(7 * M + 3 * N + K)
    a = rs.randn(M, K).astype(np.float32)
    w = (rs.randn(K, N) * 0.2).astype(np.float32)
    sp._fwd_case(rs, M, N, K, a, w, 10, True, True)


@pytest.mark.gpu
@pytest.mark.parametrize("M,N", FWD_GRIDS)
def test_dense_fwd_head_partials_every_tile_order(M, N):
    assert tn.backend_name() == "hip-gfx950"
    _fwd(M, N, 16)


@pytest.mark.gpu
def test_dense_fwd_head_partials_16_wave_form():
    assert tn.backend_name() == "hip-gfx950"
    _fwd(32, 64, 784)


@pytest.mark.gpu
def test_generic_small_tile_plain_order_in_a_child_process():
    env = dict(os.environ, TNN_GEMM_SMALL="1", PYTHONDONTWRITEBYTECODE="1")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tile_order_small_worker.py")], env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert run.returncode == 0, run.stdout[-3000:]
    assert "tile_order_small_worker ok" in run.stdout, run.stdout[-3000:]


# (rows, n_in): dW1 is tiles_in x 8 tiles, dx is ceil(rows / 16) x (tiles_in or, wide, tiles_in / 2) tiles
HEAD_CASES = [(96, 96),     # tiles_in 6: dW1 cut with rectangles of 3; 6 row tiles x 3 wide dx columns: plain order
              (128, 160),   # tiles_in 10: rectangles of 5; wide dx tiles, 8 x 5: plain order
              (128, 784)]   # tiles_in 49, odd: both roles in plain order, 16-wide dx tiles (the MNIST first layer's width)


@pytest.mark.gpu
@pytest.mark.parametrize("m,n_in", HEAD_CASES)
def test_mlp_head_bwd_tick_every_tile_order(m, n_in):
    sp.test_mlp_head_bwd_tick_vs_float64(m, n_in)
