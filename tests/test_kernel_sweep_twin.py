"""The same sweep (kernel_sweep.py) on the CPU twin of the C-ABI: exercises the harness, the references and the twin's
own arithmetic in the container.  On a machine with a GPU the suite's backend is the HIP library and
test_gpu_kernel_sweep.py covers these cases, so there is nothing to run here."""

import pytest

import kernel_sweep
import tinynn_autograd_amd as tn


@pytest.mark.parametrize("case", kernel_sweep.CASES)
def test_kernel_sweep_twin(case):
    if tn.backend_name() == "hip-gfx950":
        pytest.skip("the suite runs on libtnn_hip.so here: covered by test_gpu_kernel_sweep.py")
    kernel_sweep.run_case(case)
