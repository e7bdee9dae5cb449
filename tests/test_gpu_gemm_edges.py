"""`pytest -m gpu`: the sweep of the fp32 / f64 GEMM entry points (gemm_edges.py) through libtnn_hip.so on the MI355X.  The
tuning overrides that force the LDS-tiled kernel at small shapes are set through monkeypatch, which restores them."""

import pytest

import gemm_edges
import tinynn_autograd_amd as tn


@pytest.mark.gpu
@pytest.mark.parametrize("case", gemm_edges.CASES)
def test_gpu_gemm_edges(case, monkeypatch):
    assert tn.backend_name() == "hip-gfx950"
    gemm_edges.run_case(case, monkeypatch)
