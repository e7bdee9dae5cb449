"""`pytest -m gpu`: the sweep of the loss and optimizer kernels (loss_optim_sweep.py) through libtnn_hip.so on the MI355X."""

import pytest

import loss_optim_sweep
import tinynn_autograd_amd as tn


@pytest.mark.gpu
@pytest.mark.parametrize("case", loss_optim_sweep.CASES)
def test_gpu_loss_optim_sweep(case):
    assert tn.backend_name() == "hip-gfx950"
    loss_optim_sweep.run_case(case)
