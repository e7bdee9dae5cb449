"""`pytest -m gpu`: the step kernels with their first-request arguments as leading scalar parameters (preloaded into user SGPRs
at wave launch: gemm_small_pre_f32_kernel, dense_bwd0_adam_pre_kernel, mlp_head_bwd_pre_kernel) against the same launches on the
argument-block kernels, forced per call with TNN_STEP_ARGS=struct — through the ABI, in one process, BIT FOR BIT.  The forward
kernels run one tile body (small_tile_fast); what differs
is where the operands' resources, the extents and the tile order come from, so a wrong dword, a wrong bit field of the packed
order or a wrong flag shows as a different tile, a different chunk count or a missing head_w fragment.

tnn_dense_fwd_head_partials: M 1 / 17 / 128 (one ragged tile row, two, eight), N 16 / 40 (one tile column; three with a ragged
last one), K 4 (three of four waves without a chunk), 272 (the 8-wave form), 784 (the 16-wave form), 1040 (two trips of it),
head_c 1 / 10, with and without bias.  C sits inside a wider, longer sentinel-filled array and head_z in front of sentinels:
both forms must leave them alone.  tnn_step_args_form(0) tells which kernel the last launch took.

tnn_dense_bwd_first_adam (dW0 = X^T dZ0 + Adam on 16 x 32 tiles, the flat range behind them; tnn_step_args_form(1)): rows 1 / 16 /
128 (one chunk with 15 rows missing, one whole chunk, two chunks on each of four waves), n_in 32 with 4096 units (two tile rows:
the smallest gradient that takes the 16 x 32 tiles, 256 of them) and 784 with 256 (the MNIST layer, 49 tile rows, the 2 x 4 cut),
two consecutive steps, so the state a step reads up front is the state the step before wrote.  dW, db, the weight and bias
blocks with their moments, and the flat range: byte-equal between the forms after each step.  n_in 32 with 256 units has too few
tiles for the 16 x 32 form and keeps the 16 x 16 argument-block kernel: the case whose sizes choose the fallback.

tnn_mlp_head_bwd_tick: see test_mlp_head_bwd_tick_sgprs_equal_struct (tnn_step_args_form_head()).

The host keeps a launch of tnn_dense_fwd_head_partials on the argument-block kernel when its operands are not the FAST form's (K = 6 is no
multiple of 4) or when it has more workgroups than the CUs place at once (M = 2064, N = 40: 387 tiles): the two fallback cases
here.  An order that does not pack cannot be reached by size (grids above 8192 tiles go to the tiled kernel, the three dwords
hold rectangles up to 65,535): tests/tile_order_packed_check.cpp covers the packer's refusals on the host."""

import ctypes
import os

import numpy as np
import pytest

import tinynn_autograd_amd as tn
from tinynn_autograd_amd import _lib

PAD = 8
SENT = np.float32(-777.25)
SWITCH = "TNN_STEP_ARGS"


def _form(which=0):
    fn = ctypes.CDLL(_lib.LIB_PATH).tnn_step_args_form
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int]
    return fn(which)


def _launch(struct_form, call, which=0):
    """`call()` with the switch set for exactly this call; returns the form the launch reports."""
    old = os.environ.pop(SWITCH, None)
    try:
        if struct_form:
            os.environ[SWITCH] = "struct"
        call()
        return _form(which)
    finally:
        os.environ.pop(SWITCH, None)
        if old is not None:
            os.environ[SWITCH] = old


def _fwd(M, N, K, a, w, bias, hw, hc, with_bias, struct_form):
    tiles = (N + 15) // 16
    ldc = N + 3
    c0 = np.full((M + 1, ldc), SENT, np.float32)
    z0 = np.full(tiles * M * hc + PAD, SENT, np.float32)
    A, W, Bv, HW, C, Z = (tn.asarray(v) for v in (a, w, bias, hw, c0, z0))
    form = _launch(struct_form, lambda: _lib.get().dense_fwd_head_partials(
        M, N, K, A._ptr, K, W._ptr, N, Bv._ptr if with_bias else None, _lib.ACT_RELU, 1, C._ptr, ldc, HW._ptr, hc, Z._ptr, _lib.F32))
    return form, np.asarray(C).copy(), np.asarray(Z).copy(), c0, z0


@pytest.mark.gpu
@pytest.mark.parametrize("K", [4, 272, 784, 1040])
@pytest.mark.parametrize("N", [16, 40])
def test_dense_fwd_head_partials_sgprs_equal_struct(N, K):
    assert tn.backend_name() == "hip-gfx950"
    rs = np.random.RandomState(7000 * N + K)
    w = (rs.randn(K, N) * 0.2).astype(np.float32)
    bias = rs.randn(N).astype(np.float32)
    for M in (1, 17, 128):
        a = rs.randn(M, K).astype(np.float32)
        for hc in (1, 10):
            hw = (rs.randn(N, hc) * 0.3).astype(np.float32)
            for with_bias in (True, False):
                tag = "M %d N %d K %d head_c %d bias %s" % (M, N, K, hc, with_bias)
                f1, c1, z1, c0, z0 = _fwd(M, N, K, a, w, bias, hw, hc, with_bias, False)
                f0, cs, zs, _, _ = _fwd(M, N, K, a, w, bias, hw, hc, with_bias, True)
                assert f1 == 1, tag + ": the launch did not take the preloaded kernel (form %d)" % f1
                assert f0 == 0, tag + ": TNN_STEP_ARGS=struct was not honoured (form %d)" % f0
                tiles = (N + 15) // 16
                assert np.array_equal(c1[M], c0[M]) and np.array_equal(c1[:, N:], c0[:, N:]), tag + ": C written outside [M][N]"
                assert np.array_equal(z1[tiles * M * hc:], z0[tiles * M * hc:]), tag + ": head_z written behind its last tile"
                assert not (c1[:M, :N] == SENT).any() and not (z1[:tiles * M * hc] == SENT).any(), tag + ": an output left unwritten"
                assert c1.tobytes() == cs.tobytes(), tag + ": C differs between the two forms"
                assert z1.tobytes() == zs.tobytes(), tag + ": head_z differs between the two forms"


@pytest.mark.gpu
@pytest.mark.parametrize("M,K", [(17, 6), (2064, 8)])
def test_dense_fwd_head_partials_fallback_by_sizes(M, K):
    """K = 6: not the FAST form's operands.  M = 2064 with N = 40: 129 x 3 tiles, more workgroups than the 256 CUs place at
    once.  Both keep the argument-block kernel without the switch, and compute the same product."""
    assert tn.backend_name() == "hip-gfx950"
    rs = np.random.RandomState(6)
    N, hc = 40, 10
    bias = rs.randn(N).astype(np.float32)
    hw = (rs.randn(N, hc) * 0.3).astype(np.float32)
    a8, w8 = rs.randn(17, 8).astype(np.float32), (rs.randn(8, N) * 0.2).astype(np.float32)
    assert _fwd(17, N, 8, a8, w8, bias, hw, hc, True, False)[0] == 1          # (the getter moves: a preloaded launch first)
    a, w = rs.randn(M, K).astype(np.float32), (rs.randn(K, N) * 0.2).astype(np.float32)
    form, c, z, c0, z0 = _fwd(M, N, K, a, w, bias, hw, hc, True, False)
    assert form == 0
    pre = a.astype(np.float64) @ w.astype(np.float64) + bias
    bound = 2e-6 * (np.abs(a.astype(np.float64)) @ np.abs(w.astype(np.float64)) + np.abs(bias.astype(np.float64))) + 1e-30
    assert (np.abs(np.abs(c[:M, :N].astype(np.float64)) - np.maximum(pre, 0)) <= bound).all()
    assert np.array_equal(c[M], c0[M]) and np.array_equal(c[:, N:], c0[:, N:])


def _bwd0_two_steps(rows, n_in, n_out, x, dz, w, b, flat, struct_form):
    """steps 1 and 2 on fresh state; returns the forms taken and every array the launch writes, after each step"""
    nf = flat[0].size
    X, DZ = tn.asarray(x), tn.asarray(dz)
    dw, db = tn.asarray(np.full((n_in, n_out), SENT, np.float32)), tn.asarray(np.full((n_out,), SENT, np.float32))
    pw, pb = tn.asarray(w), tn.asarray(b)
    mw, vw, mb, vb = tn.zeros((n_in, n_out)), tn.zeros((n_in, n_out)), tn.zeros((n_out,)), tn.zeros((n_out,))
    fp, fg, fm, fv = tn.asarray(flat[0]), tn.asarray(flat[1]), tn.zeros((nf,)), tn.zeros((nf,))
    forms, outs = [], []
    for t in (1, 2):
        pows = tn.asarray(np.array([0.9 ** t, 0.999 ** t, 0, 0]), dtype=np.float64)
        forms.append(_launch(struct_form, lambda: _lib.get().dense_bwd_first_adam(
            rows, n_in, n_out, X._ptr, DZ._ptr, dw._ptr, db._ptr, pw._ptr, mw._ptr, vw._ptr, pb._ptr, mb._ptr, vb._ptr, fp._ptr,
            fg._ptr, fm._ptr, fv._ptr, nf, 1e-3, 0.9, 0.999, 1e-8, pows._ptr, _lib.F32), which=1))
        outs.append([np.asarray(v).copy() for v in (dw, db, pw, mw, vw, pb, mb, vb, fp, fm, fv)])
    return forms, outs


BWD0_NAMES = ("dw", "db", "p_w", "m_w", "v_w", "p_b", "m_b", "v_b", "flat_p", "flat_m", "flat_v")


@pytest.mark.gpu
@pytest.mark.parametrize("n_in,n_out,preloaded", [(32, 4096, True), (784, 256, True), (32, 256, False)])
@pytest.mark.parametrize("rows", [1, 16, 128])
def test_dense_bwd_first_adam_sgprs_equal_struct(rows, n_in, n_out, preloaded):
    assert tn.backend_name() == "hip-gfx950"
    rs = np.random.RandomState(10 * n_in + rows)
    x = (rs.rand(rows, n_in) * (rs.rand(rows, n_in) < 0.5)).astype(np.float32)
    dz = (rs.randn(rows, n_out) * 0.1).astype(np.float32)
    w, b = (rs.randn(n_in, n_out) * 0.1).astype(np.float32), rs.randn(n_out).astype(np.float32)
    flat = (rs.randn(1003).astype(np.float32), (rs.randn(1003) * 0.1).astype(np.float32))
    tag = "rows %d n_in %d n_out %d" % (rows, n_in, n_out)
    f1, o1 = _bwd0_two_steps(rows, n_in, n_out, x, dz, w, b, flat, False)
    f0, o0 = _bwd0_two_steps(rows, n_in, n_out, x, dz, w, b, flat, True)
    assert f1 == [int(preloaded)] * 2, tag + ": forms %s without the switch" % f1
    assert f0 == [0, 0], tag + ": TNN_STEP_ARGS=struct was not honoured (forms %s)" % f0
    for t in (0, 1):
        for name, got, ref in zip(BWD0_NAMES, o1[t], o0[t]):
            assert got.tobytes() == ref.tobytes(), "%s step %d: %s differs between the two forms" % (tag, t + 1, name)
        assert not (o1[t][0] == SENT).any() and not (o1[t][1] == SENT).any(), tag + ": a gradient entry left unwritten"
    # the gradient itself against float64 (the bound of gemm_shapes_and_transposes: 2e-6 |X|^T |dZ|), both steps the same
    x64, dz64 = x.astype(np.float64), dz.astype(np.float64)
    bound = 2e-6 * (np.abs(x64).T @ np.abs(dz64)) + 1e-30
    assert (np.abs(o1[0][0].astype(np.float64) - x64.T @ dz64) <= bound).all(), tag + ": dW"
    assert (np.abs(o1[0][1].astype(np.float64) - dz64.sum(0)) <= 2e-6 * np.abs(dz64).sum(0) + 1e-30).all(), tag + ": db"
    assert o1[0][0].tobytes() == o1[1][0].tobytes() and not np.array_equal(o1[0][2], o1[1][2]), tag + ": the second step"


def _form_head():
    fn = ctypes.CDLL(_lib.LIB_PATH).tnn_step_args_form_head
    fn.restype = ctypes.c_int
    return fn()


HEAD_NAMES = ("logits", "dz", "stats", "loss", "dw", "db", "dw1", "db1", "dx", "pows")


def _head_tick(m, n_in, x, w1, a, zp, w, b, y, struct_form):
    Hn, C = 128, 10
    lib = _lib.get()
    X, W1, A, ZP, W, B, Y = (tn.asarray(v) for v in (x, w1, a, zp, w, b, y))
    logits, dz, stats, loss = tn.empty((m, C)), tn.empty((m, C)), tn.empty((2,)), tn.empty(())
    dw, db, dw1, db1 = tn.zeros((Hn, C)), tn.zeros((C,)), tn.zeros((n_in, Hn)), tn.zeros((Hn,))
    dx = tn.asarray(np.full((m + 1, n_in), SENT, np.float32))
    pows = tn.asarray(np.array([0.9, 0.999, 0, 0]), dtype=np.float64)
    old = os.environ.pop(SWITCH, None)
    try:
        if struct_form:
            os.environ[SWITCH] = "struct"
        lib.mlp_head_bwd_tick(m, n_in, Hn, C, X._ptr, W1._ptr, A._ptr, W._ptr, B._ptr, Y._ptr, ZP._ptr, logits._ptr, dz._ptr,
                              stats._ptr, loss._ptr, dw._ptr, db._ptr, dw1._ptr, db1._ptr, dx._ptr, _lib.F32, pows._ptr, 0.9, 0.999)
        form = _form_head()
    finally:
        os.environ.pop(SWITCH, None)
        if old is not None:
            os.environ[SWITCH] = old
    return form, [np.asarray(v).copy() for v in (logits, dz, stats, loss, dw, db, dw1, db1, dx, pows)]


@pytest.mark.gpu
@pytest.mark.parametrize("n_in", [16, 48, 256])
@pytest.mark.parametrize("m", [2, 127, 128])
def test_mlp_head_bwd_tick_sgprs_equal_struct(m, n_in):
    """The merged head + hidden-backward launch with its first-request block (zpart, y, b, m, vec) in preloaded SGPRs against
    the argument-block kernel, bit for bit: rows 2 / 128 take the 16-byte staging, 127 (odd) the element-wise one; n_in 16 / 48
    the 16-wide dx tiles, 256 the 32-wide ones.  Every single-GPU launch of this form fits the block (five dwords' worth of
    scalars, three pointers), so this entry has no fallback chosen by size: the switch is the only way to the old kernel, and
    more than 128 rows take the row-blocked kernel, which has one form."""
    assert tn.backend_name() == "hip-gfx950"
    rs = np.random.RandomState(300 * m + n_in)
    Hn, C = 128, 10
    pre0 = rs.randn(m, n_in).astype(np.float32)
    x = np.where(pre0 < 0, np.float32(-0.0), np.abs(pre0)).astype(np.float32)
    w1 = (rs.randn(n_in, Hn) * 0.2).astype(np.float32)
    b1 = rs.randn(Hn).astype(np.float32)
    w, b = (rs.randn(Hn, C) * 0.3).astype(np.float32), rs.randn(C).astype(np.float32)
    y = np.eye(C, dtype=np.float32)[rs.randint(0, C, m)]
    X, W1, B1, W = (tn.asarray(v) for v in (x, w1, b1, w))
    A, ZP = tn.empty((m, Hn)), tn.zeros((Hn // 16, m, C))
    _lib.get().dense_fwd_head_partials(m, Hn, n_in, X._ptr, n_in, W1._ptr, Hn, B1._ptr, _lib.ACT_RELU, 1, A._ptr, Hn, W._ptr, C,
                                       ZP._ptr, _lib.F32)
    a, zp = np.asarray(A).copy(), np.asarray(ZP).copy()
    f1, o1 = _head_tick(m, n_in, x, w1, a, zp, w, b, y, False)
    f0, o0 = _head_tick(m, n_in, x, w1, a, zp, w, b, y, True)
    tag = "rows %d n_in %d" % (m, n_in)
    assert f1 == 1, tag + ": the launch did not take the preloaded kernel (form %d)" % f1
    assert f0 == 0, tag + ": TNN_STEP_ARGS=struct was not honoured (form %d)" % f0
    for name, got, ref in zip(HEAD_NAMES, o1, o0):
        assert got.tobytes() == ref.tobytes(), "%s: %s differs between the two forms" % (tag, name)
    assert (o1[8][m] == SENT).all() and not (o1[8][:m] == SENT).any(), tag + ": dx rows"
    z = a.astype(np.float64) * ~np.signbit(a) @ w.astype(np.float64) + b
    np.testing.assert_allclose(o1[0], z, rtol=0, atol=2e-5 * np.abs(z).max(), err_msg=tag)
