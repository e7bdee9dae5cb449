"""`pytest -m gpu`: the latency tiles whose K walk runs one straight-line body per number of live chunks (csrc/tnn_gemm_small.h:
small_tile_fast's first batch, tn_batches), through the ABI, at every body and on both sides of every branch that is left.

tnn_dense_fwd_head_partials (small_tile_fast).  A wave's first batch is specialised on its number of live chunks (0 .. 4) and on
what it requests for the epilogue (nothing, the bias, the bias and wave 0's head_w fragment).  With 4 waves K = 4 leaves three
waves without a chunk, 16 .. 64 give one chunk to one .. four waves, 80 / 144 / 208 make wave 0 the only one with two / three /
four chunks and 256 fills every wave; 272 / 400 / 512 run the 8-wave form with three / four chunks on its first waves and 528
sends wave 0 into the second batch's loop; 784 / 1024 are the 16-wave form (waves past the fourth request no epilogue operand)
and 1040 its second batch.  M 16 / 17 and N 16 / 40 add a ragged tile row and column.  One more case runs the same kernel
without bias and without a head (tnn_gemm_bias_act): every epilogue request is then out of range and must read 0.
The checks, float64 bounds and sentinel guards are those of tests/test_gpu_step_prologues.py (_fwd_case).

tnn_dense_bwd_first_adam (tn_batches), driven as tests/test_gpu_bwd0_roundtrips.py drives it.  (40, 48) and (32, 64) take the
16 x 16 tiles (small_tile<.., ADAM>): the 16 x 32 tile needs n_out a multiple of 32 AND at least 256 wide tiles (dw0_wide_ok), and
(32, 64) has four.  (2048, 64) has 128 x 2 = 256 of them and takes the 16 x 32 tile (dw_tile_wide, the kernel of the MNIST step).
Rows 1 .. 256 on four waves leave waves with 0, 1, 2, 3 and 4 live chunks on both tile widths (1 / 16: one wave with one chunk;
17: two; 48 / 64: three / four waves with one; 80: wave 0 with two; 128: two each; 192: three; 256: four).  dW, db and the
parameters, m and v of two Adam steps against its float64 recurrences, with its bounds."""

import numpy as np
import pytest

import tinynn_autograd_amd as tn
from tinynn_autograd_amd import _lib
import test_gpu_bwd0_roundtrips as b0
import test_gpu_step_prologues as sp

FWD_K = [4, 16, 20, 64, 80, 144, 208, 256,     # 4 waves
         272, 400, 512, 528,                   # 8 waves; 528: second batch
         784, 1024, 1040]                      # 16 waves; 1040: second batch
FWD_MN = [(16, 16), (17, 16), (16, 40), (17, 40)]


@pytest.mark.gpu
@pytest.mark.parametrize("K", FWD_K)
def test_dense_fwd_head_partials_every_chunk_count(K):
    assert tn.backend_name() == "hip-gfx950"
    for M, N in FWD_MN:
        rs = np.random.RandomState(11 * M + 5 * N + K)
        a = rs.randn(M, K).astype(np.float32)
        w = (rs.randn(K, N) * 0.2).astype(np.float32)
        sp._fwd_case(rs, M, N, K, a, w, 10, True, True)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [4, 80, 784])
def test_small_fast_tile_without_bias_and_head(K):
    """bias = NULL and no head: the epilogue operand's resource is empty and no wave takes the head role"""
    assert tn.backend_name() == "hip-gfx950"
    M, N = 17, 40
    rs = np.random.RandomState(K)
    a = rs.randn(M, K).astype(np.float32)
    w = (rs.randn(K, N) * 0.2).astype(np.float32)
    ldc = N + 3
    c0 = np.full((M + 1, ldc), sp.SENT, np.float32)
    A, W, C = tn.asarray(a), tn.asarray(w), tn.asarray(c0)
    _lib.get().gemm_bias_act(0, 0, M, N, K, A._ptr, K, W._ptr, N, None, _lib.ACT_NONE, 0, C._ptr, ldc, _lib.F32)
    c = np.asarray(C)
    assert np.array_equal(c[M], c0[M]) and np.array_equal(c[:, N:], c0[:, N:]), "C written outside [M][N]"
    a64, w64 = a.astype(np.float64), w.astype(np.float64)
    err = np.abs(c[:M, :N].astype(np.float64) - a64 @ w64)
    assert (err <= 2e-6 * (np.abs(a64) @ np.abs(w64)) + 1e-30).all(), "K %d: C max err %g" % (K, err.max())


BWD_SHAPES = [(40, 48), (32, 64),      # 16 x 16 tiles
              (2048, 64)]             # 256 tiles of 16 x 32: dw_tile_wide
BWD_ROWS = [1, 16, 17, 48, 64, 80, 128, 192, 256]


@pytest.mark.gpu
@pytest.mark.parametrize("n_in,n_out", BWD_SHAPES)
def test_dense_bwd_first_adam_every_chunk_count(n_in, n_out):
    assert tn.backend_name() == "hip-gfx950"
    rs = np.random.RandomState(43)
    w = (rs.randn(n_in, n_out) * 0.05).astype(np.float32)
    b = rs.randn(n_out).astype(np.float32)
    for rows in BWD_ROWS:
        x = rs.rand(rows, n_in).astype(np.float32)
        dz = (rs.randn(rows, n_out) * 0.1).astype(np.float32)
        outs = b0._run(rs, rows, n_in, n_out, x, dz, w, b, 3, 0)
        b0._check_tiles(outs, x, dz, w, b)
