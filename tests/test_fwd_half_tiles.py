"""The half-height form of the first layer's forward (csrc/tnn_gemm_small.h: gemm_small_half_f32_kernel, 8-row x 16-column
tiles over the whole K on sixteen waves; csrc/tnn_gemm.hip: half_tiles_ok) against the 16-row form it replaces.

Host (no GPU): tests/half_tile_order_check.cpp, the grid and order of the 8-row tiles against the division formulas.

`pytest -m gpu`, through tnn_gemm_bias_act (the entry point of the step's fwd0) with TNN_FWD0_TILE unset and = 16:
  * rows 1 / 8 / 9 / 17 / 128 (less than a tile, one tile, a ragged second tile, a ragged third, the headline), K 1 / 16 / 49 /
    65 / 784, N 16 / 24 / 250 (250: a ragged sixteenth column tile), each plain and with bias + sign-encoded ReLU.  Both
    settings must give the same bytes, leave everything outside [M][N] alone, and meet the float64 product at the bound of
    tests/gemm_edges.py for this kernel family: |got - ref| <= gamma_n (|A| |B| + |bias|) with n = K + 3, u = 2^-24, the ReLU
    compared only where |z| exceeds that gate (elsewhere a zero of either sign or a value below the gate).  K = 784 is the
    depth at which the host takes the sixteen-wave kernel and, at these grids, its half-height form (tnn_small_tile_rows: 8,
    and 16 under the switch); the other depths run the 4-wave or the plain kernel under both settings.
  * the column sums of the same shapes (tnn_gemm_tn_colsum, the entry point that has them: a TN product, which keeps its
    kernel): equal bytes under both settings and the float64 sums within gamma_K sum |B|.
  * 20 steps of the whole-step trainer at 128 rows under both settings: loss and every parameter byte-equal."""

import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH = "TNN_FWD0_TILE"
SENT = np.float32(-777.25)
U = 2.0 ** -24


def test_half_tile_order_matches_the_division_formulas(tmp_path):
    exe = os.path.join(str(tmp_path), "half_tile_order_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tinynn-autograd_amd", "csrc"),
                           os.path.join(ROOT, "tests", "half_tile_order_check.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert run.returncode == 0, run.stdout
    assert run.stdout.strip().startswith("half tile order ok"), run.stdout


class _Switch:
    """TNN_FWD0_TILE=16 (or unset) for the calls inside the block; the host reads it per launch."""

    def __init__(self, keep16):
        self.keep16 = keep16

    def __enter__(self):
        self.old = os.environ.pop(SWITCH, None)
        if self.keep16:
            os.environ[SWITCH] = "16"

    def __exit__(self, *exc):
        os.environ.pop(SWITCH, None)
        if self.old is not None:
            os.environ[SWITCH] = self.old


def _tile_rows():
    from tinynn_autograd_amd import _lib
    fn = ctypes.CDLL(_lib.LIB_PATH).tnn_small_tile_rows
    fn.restype, fn.argtypes = ctypes.c_int, []
    return fn()


def _gamma(n):
    return n * U / (1.0 - n * U)


ROWS = [1, 8, 9, 17, 128]
COLS = [16, 24, 250]


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 16, 49, 65, 784])
def test_half_height_equals_16_row_form_and_float64(K):
    import tinynn_autograd_amd as tn
    from tinynn_autograd_amd import _lib
    assert tn.backend_name() == "hip-gfx950"
    lib = _lib.get()
    rs = np.random.RandomState(100 + K)
    for N in COLS:
        w = (rs.randn(K, N) * 0.2).astype(np.float32)
        bias = rs.randn(N).astype(np.float32)
        W, Bv = tn.asarray(w), tn.asarray(bias)
        for M in ROWS:
            a = rs.randn(M, K).astype(np.float32)
            A = tn.asarray(a)
            a64, w64 = a.astype(np.float64), w.astype(np.float64)
            prod, absp = a64 @ w64, np.abs(a64) @ np.abs(w64)        # one reference for the four launches below
            ldc = N + 3
            c0 = np.full((M + 1, ldc), SENT, np.float32)
            for epi in (False, True):
                tag = "M %d N %d K %d %s" % (M, N, K, "bias + ReLU" if epi else "plain")
                out = []
                for keep16 in (False, True):
                    C = tn.asarray(c0)
                    with _Switch(keep16):
                        lib.gemm_bias_act(0, 0, M, N, K, A._ptr, K, W._ptr, N, Bv._ptr if epi else None,
                                          _lib.ACT_RELU if epi else _lib.ACT_NONE, 1 if epi else 0, C._ptr, ldc, _lib.F32)
                        out.append(np.asarray(C).copy())
                    if K == 784:
                        assert _tile_rows() == (16 if keep16 else 8), tag + ": tile rows %d (switch %s)" % (_tile_rows(), keep16)
                c8, c16 = out
                assert np.array_equal(c8[M], c0[M]) and np.array_equal(c8[:, N:], c0[:, N:]), tag + ": C written outside [M][N]"
                assert not (c8[:M, :N] == SENT).any(), tag + ": an output left unwritten"
                assert c8.tobytes() == c16.tobytes(), tag + ": the two tile forms differ"
                got = c8[:M, :N].astype(np.float64)
                z = prod + bias.astype(np.float64) if epi else prod
                gate = _gamma(K + 3) * (absp + (np.abs(bias.astype(np.float64)) if epi else 0.0)) + 1e-300
                if epi:
                    pos, neg = z > gate, z < -gate
                    assert (np.abs(got - z)[pos] <= gate[pos]).all(), tag + ": positive side outside the bound"
                    assert (got[neg] == 0).all() and np.signbit(got[neg]).all(), tag + ": a negative pre-activation not -0.0"
                    assert (np.abs(got)[~pos & ~neg] <= gate[~pos & ~neg]).all(), tag + ": inside the gate"
                else:
                    err = np.abs(got - z)
                    assert (err <= gate).all(), tag + ": max err / gate %g" % (err / gate).max()


@pytest.mark.gpu
def test_colsum_entry_is_left_alone_by_the_switch():
    import tinynn_autograd_amd as tn
    from tinynn_autograd_amd import _lib
    assert tn.backend_name() == "hip-gfx950"
    lib = _lib.get()
    rs = np.random.RandomState(5)
    for K in (1, 16, 49, 65, 784):                         # the contraction of dW = X^T G runs over the K rows of both operands
        for M, N in ((17, 16), (128, 24), (9, 250)):
            x = rs.randn(K, M).astype(np.float32)
            g = rs.randn(K, N).astype(np.float32)
            X, G = tn.asarray(x), tn.asarray(g)
            out = []
            for keep16 in (False, True):
                C, D = tn.asarray(np.zeros((M, N), np.float32)), tn.asarray(np.full(N + 1, SENT, np.float32))
                with _Switch(keep16):
                    lib.gemm_tn_colsum(M, N, K, X._ptr, M, G._ptr, N, C._ptr, N, D._ptr, _lib.F32)
                    out.append((np.asarray(C).copy(), np.asarray(D).copy()))
            tag = "M %d N %d K %d" % (M, N, K)
            assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes(), tag + ": the switch changed a TN product"
            db = out[0][1]
            assert db[N] == SENT, tag + ": db written behind its end"
            g64 = g.astype(np.float64)
            assert (np.abs(db[:N] - g64.sum(axis=0)) <= _gamma(K + 3) * np.abs(g64).sum(axis=0) + 1e-300).all(), tag + ": column sums"
            x64 = x.astype(np.float64)
            assert (np.abs(out[0][0] - x64.T @ g64) <= _gamma(K + 3) * (np.abs(x64).T @ np.abs(g64)) + 1e-300).all(), tag + ": dW"


@pytest.mark.gpu
def test_trainer_steps_equal_under_both_tile_forms():
    import tinynn_autograd_amd as tn
    from tinynn_autograd_amd.fused import MLPTrainer
    assert tn.backend_name() == "hip-gfx950"
    widths, rows = [784, 256, 128, 10], 128
    rs = np.random.RandomState(3)
    xs = [(rs.rand(rows, 784) * (rs.rand(rows, 784) < 0.19)).astype(np.float32) for _ in range(4)]
    ys = [np.eye(10, dtype=np.float32)[rs.randint(0, 10, rows)] for _ in range(4)]
    results = []
    for keep16 in (False, True):
        with _Switch(keep16):
            np.random.seed(11)                             # the same initial parameters for both trainers
            t = MLPTrainer(widths, rows, loss="softmax_nll", optimizer="adam", lr=1e-3)
            losses = [float(t.step(tn.asarray(xs[i % 4]), tn.asarray(ys[i % 4]))) for i in range(20)]
            assert _tile_rows() == (16 if keep16 else 8), "fwd0 ran on %d-row tiles (switch %s)" % (_tile_rows(), keep16)
            params = [np.asarray(t.param_view(l, k)).copy() for l in range(3) for k in ("w", "b")]
            results.append((np.asarray(losses, np.float64), params))
    (l8, p8), (l16, p16) = results
    assert l8.tobytes() == l16.tobytes(), "losses differ between the tile forms"
    assert np.isfinite(l8).all() and l8[-1] < l8[0], "the trainer did not train"
    for i, (u, v) in enumerate(zip(p8, p16)):
        assert u.tobytes() == v.tobytes(), "parameter %d differs between the tile forms" % i
