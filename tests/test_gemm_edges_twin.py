"""The same sweep (gemm_edges.py) on the CPU twin of the C-ABI: exercises the harness, the exact references and the derived
bounds against one independent implementation in the container (the twin ignores the tuning overrides).  On a machine
with a GPU the suite's backend is the HIP library and test_gpu_gemm_edges.py covers these cases, so there is nothing to
run here."""

import pytest

import gemm_edges
import tinynn_autograd_amd as tn


@pytest.mark.parametrize("case", gemm_edges.CASES)
def test_gemm_edges_twin(case, monkeypatch):
    if tn.backend_name() == "hip-gfx950":
        pytest.skip("the suite runs on libtnn_hip.so here: covered by test_gpu_gemm_edges.py")
    gemm_edges.run_case(case, monkeypatch)
