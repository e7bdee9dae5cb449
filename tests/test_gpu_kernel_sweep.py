"""`pytest -m gpu`: the sweep of the generic op kernels (kernel_sweep.py) through libtnn_hip.so on the MI355X."""

import pytest

import kernel_sweep
import tinynn_autograd_amd as tn


@pytest.mark.gpu
@pytest.mark.parametrize("case", kernel_sweep.CASES)
def test_gpu_kernel_sweep(case):
    assert tn.backend_name() == "hip-gfx950"
    kernel_sweep.run_case(case)
