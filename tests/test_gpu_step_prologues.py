"""`pytest -m gpu`: the two launches of the MNIST step whose prologues request every operand in one round —
tnn_dense_fwd_head_partials (hidden layer forward + the classifier's partial logits) and tnn_mlp_head_bwd_tick (classifier head +
the hidden layer's backward) — through the ABI against float64 numpy, at every branch their operand requests take.

tnn_dense_fwd_head_partials.  The epilogue's operand (the bias) and wave 0's head_w fragment are buffer loads whose offset is
0xffffffff for a thread, row, class or hidden unit that does not exist and whose resource is empty for a NULL bias.  M 1 .. 17
leave tile rows ragged, N = 40 is a ragged tile column (units 40 .. 47 of the last tile do not exist), head_c 1 / 10 / 16 moves the
class guard, K 4 leaves three of the four waves without a chunk (they still request the bias), K 16 .. 256 fill one to four
chunks per wave, K 272 takes the 8-wave form, K 528 gives a wave of that form five chunks (two loop trips), K 784 takes the 16-wave
form and K 1040 two trips of it (gemm_small: 4 waves up to 16 chunks of 16, 8 up to 48, 16 beyond).
Bounds: those of gemm_shapes_and_transposes, 2e-6 |A| |B| — the bias is one more term of every sum (a column of ones in A, the
bias as the row of B under it), so where there is one it enters |A| |B| as |bias|.  The partial logits are checked as a product of
the activations the device wrote: sum over tiles of head_z = relu(C) head_w within 2e-6 |C| |head_w| (a sign-encoded zero counts
as 0), and every tile's own share within the same bound over its 16 units.  Where ReLU zeroed an element whose float64
pre-activation is further from 0 than the bound, the sign bit must be set, and clear where it kept one.  C is written into a
wider, longer sentinel-filled array and head_z into a longer one: nothing outside [M][N] / [tiles][M][head_c] may change.

tnn_mlp_head_bwd_tick.  The bias of the logits is requested with the staged partial logits, and a tile workgroup requests the
loads of its role (dW1: the x fragment; dx: W1 fragment(s) and mask source(s)) in one sequence with the shared ones.  Rows 2 / 16 /
126 / 128 take the 16-byte staging path, 127 (odd) the element-wise one; 2 and 126 / 127 leave clamped rows; n_in 16 and 48 have an
odd number of input tiles (16-wide dx tiles), 32 and 256 take the 32-wide ones.  Loss, dW2, db2, dW1, db1, dx (and logits, dz,
statistics) against the float64 chain on the activations the forward launch wrote, with the tolerances
head_and_hidden_backward_one_launch_vs_numpy applies to the same quantities."""

import numpy as np
import pytest

import tinynn_autograd_amd as tn
from tinynn_autograd_amd import _lib

PAD = 8
SENT = np.float32(-777.25)

FWD_M = [1, 15, 16, 17, 128]
FWD_N = [16, 40, 128]
FWD_K = [4, 16, 64, 256, 272, 528, 784, 1040]
FWD_HC = [1, 10, 16]


def _fwd_case(rs, M, N, K, a, w, hc, with_bias, relu):
    tiles = (N + 15) // 16
    ldc = N + 3
    bias = rs.randn(N).astype(np.float32)
    hw = (rs.randn(N, hc) * 0.3).astype(np.float32)
    c0 = np.full((M + 1, ldc), SENT, np.float32)
    z0 = np.full(tiles * M * hc + PAD, SENT, np.float32)
    A, W, Bv, HW, C, Z = (tn.asarray(v) for v in (a, w, bias, hw, c0, z0))
    _lib.get().dense_fwd_head_partials(M, N, K, A._ptr, K, W._ptr, N, Bv._ptr if with_bias else None,
                                       _lib.ACT_RELU if relu else _lib.ACT_NONE, 1, C._ptr, ldc, HW._ptr, hc, Z._ptr, _lib.F32)
    tag = "M %d N %d K %d head_c %d bias %s relu %s" % (M, N, K, hc, with_bias, relu)
    c, z = np.asarray(C), np.asarray(Z)
    assert np.array_equal(c[M], c0[M]) and np.array_equal(c[:, N:], c0[:, N:]), tag + ": C written outside [M][N]"
    assert np.array_equal(z[tiles * M * hc:], z0[tiles * M * hc:]), tag + ": head_z written behind its last tile"
    c, z = c[:M, :N], z[:tiles * M * hc].reshape(tiles, M, hc)

    a64, w64 = a.astype(np.float64), w.astype(np.float64)
    pre = a64 @ w64
    bound = 2e-6 * (np.abs(a64) @ np.abs(w64)) + 1e-30
    if with_bias:
        pre = pre + bias
        bound = bound + 2e-6 * np.abs(bias.astype(np.float64))
    ref = np.maximum(pre, 0) if relu else pre
    err = np.abs(np.abs(c.astype(np.float64)) - ref) if relu else np.abs(c.astype(np.float64) - ref)
    assert (err <= bound).all(), "%s: C max err %g" % (tag, err.max())
    if relu:
        assert np.signbit(c[pre < -bound]).all(), tag + ": a zeroed element without the sign bit"
        assert not np.signbit(c[pre > bound]).any(), tag + ": a kept element with the sign bit"

    act = np.where(np.signbit(c), 0.0, c.astype(np.float64)) if relu else c.astype(np.float64)
    hw64 = hw.astype(np.float64)
    total = np.zeros((M, hc))
    for t in range(tiles):
        sl = slice(16 * t, min(16 * t + 16, N))
        part = act[:, sl] @ hw64[sl]
        pb = 2e-6 * (np.abs(act[:, sl]) @ np.abs(hw64[sl])) + 1e-30
        err = np.abs(z[t].astype(np.float64) - part)
        assert (err <= pb).all(), "%s: head_z tile %d max err %g" % (tag, t, err.max())
        total += z[t].astype(np.float64)
    err = np.abs(total - act @ hw64)
    assert (err <= 2e-6 * (np.abs(act) @ np.abs(hw64)) + 1e-30).all(), "%s: sum of the tiles' head_z, max err %g" % (tag, err.max())


@pytest.mark.gpu
@pytest.mark.parametrize("K", FWD_K)
@pytest.mark.parametrize("N", FWD_N)
def test_dense_fwd_head_partials_vs_float64(N, K):
    assert tn.backend_name() == "hip-gfx950"
    rs = np.random.RandomState(1000 * N + K)
    w = (rs.randn(K, N) * 0.2).astype(np.float32)
    for M in FWD_M:
        a = rs.randn(M, K).astype(np.float32)
        for hc in FWD_HC:
            for with_bias in (True, False):
                for relu in (False, True):
                    _fwd_case(rs, M, N, K, a, w, hc, with_bias, relu)


HEAD_ROWS = [2, 16, 126, 127, 128]
HEAD_N_IN = [16, 32, 48, 256]


@pytest.mark.gpu
@pytest.mark.parametrize("n_in", HEAD_N_IN)
@pytest.mark.parametrize("m", HEAD_ROWS)
def test_mlp_head_bwd_tick_vs_float64(m, n_in):
    assert tn.backend_name() == "hip-gfx950"
    lib = _lib.get()
    rs = np.random.RandomState(100 * m + n_in)
    Hn, C = 128, 10
    pre0 = rs.randn(m, n_in).astype(np.float32)
    x = np.where(pre0 < 0, np.float32(-0.0), np.abs(pre0)).astype(np.float32)        # the hidden layer's input (a ReLU output)
    x[0, 3] = 0.0                                                                    # exactly-zero pre-activation: mask = 1
    w1 = (rs.randn(n_in, Hn) * 0.2).astype(np.float32)
    b1 = rs.randn(Hn).astype(np.float32)
    w = (rs.randn(Hn, C) * 0.3).astype(np.float32)
    b = rs.randn(C).astype(np.float32)
    y = rs.rand(m, C).astype(np.float32) if n_in % 32 else np.eye(C, dtype=np.float32)[rs.randint(0, C, m)]
    X, W1, B1, W, B, Y = (tn.asarray(v) for v in (x, w1, b1, w, b, y))
    A, zpart = tn.empty((m, Hn)), tn.zeros((Hn // 16, m, C))
    lib.dense_fwd_head_partials(m, Hn, n_in, X._ptr, n_in, W1._ptr, Hn, B1._ptr, _lib.ACT_RELU, 1, A._ptr, Hn, W._ptr, C,
                                zpart._ptr, _lib.F32)
    a = np.asarray(A).copy()
    logits, dz = tn.empty((m, C)), tn.empty((m, C))
    stats, loss = tn.empty((2,)), tn.empty(())
    dw, db = tn.zeros((Hn, C)), tn.zeros((C,))
    dx0 = np.full((m + 1, n_in), SENT, np.float32)
    dw1, db1, dx = tn.zeros((n_in, Hn)), tn.zeros((Hn,)), tn.asarray(dx0)
    pows = tn.asarray(np.array([0.9, 0.999, 0, 0]), dtype=np.float64)
    lib.mlp_head_bwd_tick(m, n_in, Hn, C, X._ptr, W1._ptr, A._ptr, W._ptr, B._ptr, Y._ptr, zpart._ptr, logits._ptr, dz._ptr,
                          stats._ptr, loss._ptr, dw._ptr, db._ptr, dw1._ptr, db1._ptr, dx._ptr, _lib.F32, pows._ptr, 0.9, 0.999)
    tag = "rows=%d n_in=%d" % (m, n_in)
    a64, w64, y64, x64, w164 = (v.astype(np.float64) for v in (a, w, y, x, w1))
    z = a64 @ w64 + b
    e = np.exp(z - z.max()); S = e.sum(); q = (e * y64).sum(1, keepdims=True)
    ref_loss = (np.log(S) - np.log(q)).sum() / m
    ref_dz = e / S - (e * y64 / q) / m
    ref_da = (ref_dz @ w64.T) * ~np.signbit(a)                                        # the hidden layer's dz
    np.testing.assert_allclose(np.asarray(logits), z, rtol=0, atol=2e-5 * np.abs(z).max(), err_msg=tag)
    np.testing.assert_allclose(float(loss), ref_loss, rtol=1e-5, err_msg=tag)
    np.testing.assert_allclose(np.asarray(stats), [z.max(), S], rtol=1e-5, err_msg=tag)
    np.testing.assert_allclose(np.asarray(dz), ref_dz, rtol=0, atol=1e-5 * np.abs(ref_dz).max(), err_msg=tag)
    ref_dw = a64.T @ ref_dz
    np.testing.assert_allclose(np.asarray(dw), ref_dw, rtol=0, atol=1e-5 * np.abs(ref_dw).max(), err_msg="dw " + tag)
    np.testing.assert_allclose(np.asarray(db), ref_dz.sum(0), rtol=0, atol=1e-5 * np.abs(ref_dz.sum(0)).max() + 1e-9,
                               err_msg="db " + tag)
    got_dx = np.asarray(dx)
    assert np.array_equal(got_dx[m], dx0[m]), tag + ": dx written behind its last row"
    for name, got, ref in (("dw1", np.asarray(dw1), x64.T @ ref_da), ("db1", np.asarray(db1), ref_da.sum(0)),
                           ("dx", got_dx[:m], (ref_da @ w164.T) * ~np.signbit(x))):
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-5 * np.abs(ref).max() + 1e-12, err_msg="%s %s" % (name, tag))
    assert got_dx[0, 3] != 0.0                                                        # mask = 1 at an exactly-zero input
    np.testing.assert_allclose(np.asarray(pows)[:2], [0.9 ** 2, 0.999 ** 2], rtol=1e-14)
