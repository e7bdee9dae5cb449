"""`pytest -m gpu`: tnn_dense_bwd_first_adam through the ABI against float64 numpy, at every branch of its K walk and of its
flat-range Adam tail.

The first layer's backward requests all of a wave's 16-deep K chunks before its first MFMA (batches of four) and the trailing
workgroups update the flat range with 16-byte loads when all four arrays are 16-byte aligned.  Shapes: (784, 256) takes the
16 x 32 tiles, (790, 256) has a ragged last tile row, (784, 200) and (40, 48) take the 16 x 16 tiles; rows 1 .. 64 leave waves
with no chunk or a partial one, 128 / 130 give two and three chunks per wave, 256 a full batch of four, 272 / 300 the 8-wave
form, 530 more than four chunks per wave on the 16 x 16 tiles (two batches) and the 32 x 32-tile kernel, which shares the
flat tail, on the others.  Every flat length runs once with the pointers as allocated and once offset by one float (the
4-byte path); what lies behind the range must stay untouched.

Bounds: dW within 2e-6 (|x|^T |dz|), db within 2e-6 sum |dz| (those of gemm_shapes_and_transposes); parameters after a first
Adam step from zero moments within 2e-6 of the float64 step on the device's own gradient (as mid_size_gemm_epilogues_vs_numpy);
after a second call on the first call's moments within the Adam gate 0.01 lr of the float64 recurrence, m and v at rtol 1e-5.
The tile results cannot depend on the flat arguments, so they are checked against float64 for the first flat configuration of
a (shape, rows) pair and must be bit-equal to that run's for the others."""

import numpy as np
import pytest

import tinynn_autograd_amd as tn
from tinynn_autograd_amd import _lib

LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
SHAPES = [(784, 256), (790, 256), (784, 200), (40, 48)]
ROWS = [1, 15, 17, 64, 128, 130, 256, 272, 300, 530]
FLAT_N = [0, 1, 3, 4, 1023, 34186, 70001]
PAD = 8                                   # floats behind every flat array that must stay as they were


# The library holds b1 and b2 as float32 (AdamEpi, as adam_kernel does): 1 - float32(0.999) is 1.3e-5 (relative) away from 0.001,
# more than the rtol of the m / v check on its own.  The float64 recurrences therefore run on the coefficients the kernels are
# given — the float32 values, exactly — and every operation in float64; the bias corrections use the float64 powers passed in.
C1, C2 = 1.0 - float(np.float32(B1)), 1.0 - float(np.float32(B2))


def _adam64(p, g, m, v, t):
    m = m + C1 * (g - m)
    v = v + C2 * (g * g - v)
    return p - LR * (m / (1 - B1 ** t)) / (np.sqrt(v / (1 - B2 ** t)) + EPS), m, v


def _pows(t):
    return tn.asarray(np.array([B1 ** t, B2 ** t, 0, 0]), dtype=np.float64)


class _Flat:
    """The flat range: four device arrays of 1 + n + PAD floats; `off` = 1 starts the range one float in."""

    def __init__(self, rs, n, off):
        self.n, self.off = n, off
        size = 1 + n + PAD
        self.p0 = rs.randn(size).astype(np.float32)
        self.g0 = (rs.randn(size) * 0.1).astype(np.float32)
        self.m0 = rs.randn(size).astype(np.float32)          # outside [off, off + n): sentinels; inside: zeroed below
        self.v0 = rs.rand(size).astype(np.float32)
        self.m0[off:off + n] = 0
        self.v0[off:off + n] = 0
        self.dev = [tn.asarray(a) for a in (self.p0, self.g0, self.m0, self.v0)]
        assert all(d._ptr % 16 == 0 for d in self.dev)

    def ptrs(self):
        return [d._ptr + 4 * self.off for d in self.dev]

    def check(self, t, ref):
        """ref: (p, m, v) in float64 after t - 1 steps; returns the state after t steps"""
        sl = slice(self.off, self.off + self.n)
        p, g, m, v = (np.asarray(d) for d in self.dev)
        for got, was in ((p, self.p0), (g, self.g0), (m, self.m0), (v, self.v0)):
            out = np.ones(got.size, dtype=bool)
            out[sl] = False
            assert np.array_equal(got[out], was[out]), "flat n %d off %d: written outside the range" % (self.n, self.off)
        assert np.array_equal(g[sl], self.g0[sl])
        rp, rm, rv = _adam64(ref[0], self.g0[sl].astype(np.float64), ref[1], ref[2], t)
        np.testing.assert_allclose(p[sl], rp, rtol=0, atol=2e-6 if t == 1 else 0.01 * LR)
        np.testing.assert_allclose(m[sl], rm, rtol=1e-5, atol=1e-35)
        np.testing.assert_allclose(v[sl], rv, rtol=1e-5, atol=1e-35)
        return rp, rm, rv


def _call(rows, n_in, n_out, X, DZ, dw, db, st, flat, t):
    pw, mw, vw, pb, mb, vb = st
    fp, fg, fm, fv = flat.ptrs()
    _lib.get().dense_bwd_first_adam(rows, n_in, n_out, X._ptr, DZ._ptr, dw._ptr, db._ptr, pw._ptr, mw._ptr, vw._ptr, pb._ptr,
                                    mb._ptr, vb._ptr, fp, fg, fm, fv, flat.n, LR, B1, B2, EPS, _pows(t)._ptr, _lib.F32)


def _run(rs, rows, n_in, n_out, x, dz, w, b, n_flat, off):
    """two calls (steps 1 and 2); returns the tile-side outputs of both and checks the flat side on the way"""
    X, DZ = tn.asarray(x), tn.asarray(dz)
    st = [tn.asarray(w), tn.zeros((n_in, n_out)), tn.zeros((n_in, n_out)), tn.asarray(b), tn.zeros((n_out,)), tn.zeros((n_out,))]
    flat = _Flat(rs, n_flat, off)
    sl = slice(off, off + n_flat)
    ref = (flat.p0[sl].astype(np.float64), np.zeros(n_flat), np.zeros(n_flat))
    outs = []
    for t in (1, 2):
        dw, db = tn.empty((n_in, n_out)), tn.empty((n_out,))
        _call(rows, n_in, n_out, X, DZ, dw, db, st, flat, t)
        ref = flat.check(t, ref)
        outs.append([np.asarray(a).copy() for a in [dw, db] + st])
    return outs


def _check_tiles(outs, x, dz, w, b):
    x64, d64 = x.astype(np.float64), dz.astype(np.float64)
    ref_dw, ref_db = x64.T @ d64, d64.sum(0)
    bound_dw, bound_db = np.abs(x64).T @ np.abs(d64), np.abs(d64).sum(0)
    state = {"w": (w.astype(np.float64), 0.0, 0.0), "b": (b.astype(np.float64), 0.0, 0.0)}
    for t, (dw, db, pw, mw, vw, pb, mb, vb) in zip((1, 2), outs):
        err = np.abs(dw.astype(np.float64) - ref_dw)
        assert (err <= 2e-6 * bound_dw + 1e-30).all(), "dW: max err %g" % err.max()
        err = np.abs(db.astype(np.float64) - ref_db)
        assert (err <= 2e-6 * bound_db + 1e-30).all(), "db: max err %g" % err.max()
        for key, g, p, m, v in (("w", dw, pw, mw, vw), ("b", db, pb, mb, vb)):
            rp, rm, rv = _adam64(state[key][0], g.astype(np.float64), state[key][1], state[key][2], t)
            np.testing.assert_allclose(p, rp, rtol=0, atol=2e-6 if t == 1 else 0.01 * LR)
            np.testing.assert_allclose(m, rm, rtol=1e-5, atol=1e-35)
            np.testing.assert_allclose(v, rv, rtol=1e-5, atol=1e-35)
            state[key] = (rp, rm, rv)


@pytest.mark.gpu
@pytest.mark.parametrize("n_in,n_out", SHAPES)
def test_dense_bwd_first_adam_vs_float64(n_in, n_out):
    assert tn.backend_name() == "hip-gfx950"
    rs = np.random.RandomState(41)
    w = (rs.randn(n_in, n_out) * 0.05).astype(np.float32)
    b = rs.randn(n_out).astype(np.float32)
    for rows in ROWS:
        x = rs.rand(rows, n_in).astype(np.float32)
        dz = (rs.randn(rows, n_out) * 0.1).astype(np.float32)
        first = None
        for n_flat in FLAT_N:
            for off in (0, 1):
                outs = _run(rs, rows, n_in, n_out, x, dz, w, b, n_flat, off)
                if first is None:
                    first = outs
                    _check_tiles(outs, x, dz, w, b)
                else:
                    for got, ref in zip(outs, first):
                        assert all(np.array_equal(g, r) for g, r in zip(got, ref)), \
                            "rows %d flat %d off %d: the tiles depend on the flat range" % (rows, n_flat, off)
