"""Worker of tests/test_gpu_tile_order.py, started as a fresh process with TNN_GEMM_SMALL=1: a 48 x 48 x 20 product through the
public matmul lands on the 16 x 16 latency kernel — `a @ b` on whichever of its forms the operands allow, `at.T @ b` (TN) always on
the generic small_tile — with a 3 x 3 tile grid, which has no XCD cut: the plain column-major order.  Both against float64 within
2e-6 |A| |B| (the bound of the GEMM tests); a workgroup sent to the wrong tile leaves a tile of zeros and errors of order 1."""

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    assert os.environ.get("TNN_GEMM_SMALL") == "1"
    import tinynn_autograd_amd as tn
    from tinynn_autograd_amd import _lib
    _lib.get()                                   # raises loudly if the library or the device is missing
    assert tn.backend_name() == "hip-gfx950", tn.backend_name()
    M = N = 48
    K = 20
    rs = np.random.RandomState(4820)
    a = rs.randn(M, K).astype(np.float32)
    b = rs.randn(K, N).astype(np.float32)
    ref = a.astype(np.float64) @ b.astype(np.float64)
    bound = 2e-6 * (np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64))
    A, At, B = tn.asarray(a), tn.asarray(np.ascontiguousarray(a.T)), tn.asarray(b)
    for name, got in (("a @ b", np.asarray(A @ B)), ("at.T @ b", np.asarray(At.T @ B))):
        err = np.abs(got.astype(np.float64) - ref)
        print("%s: max err %.3g, max err / bound %.3g" % (name, err.max(), (err / bound).max()))
        assert got.shape == (M, N) and (err <= bound).all(), name
    tn.synchronize()
    print("tile_order_small_worker ok")


if __name__ == "__main__":
    main()
