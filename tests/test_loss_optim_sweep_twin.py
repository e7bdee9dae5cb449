"""The same sweep (loss_optim_sweep.py) on the CPU twin of the C-ABI: exercises the harness, the oracles and the twin's own
arithmetic in the container, and checks the softmax error model against the reference alone (the literal same-precision
numpy chain must stay within half of every bound).  On a machine with a GPU the suite's backend is the HIP library and
test_gpu_loss_optim_sweep.py covers these cases, so there is nothing to run here."""

import pytest

import loss_optim_sweep
import tinynn_autograd_amd as tn


@pytest.mark.parametrize("case", loss_optim_sweep.CASES)
def test_loss_optim_sweep_twin(case):
    if tn.backend_name() == "hip-gfx950":
        pytest.skip("the suite runs on libtnn_hip.so here: covered by test_gpu_loss_optim_sweep.py")
    loss_optim_sweep.run_case(case)
