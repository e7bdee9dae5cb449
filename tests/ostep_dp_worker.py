"""Worker of tests/test_ostep_dist.py: one rank of a world_size-N data-parallel run on the CPU twin with the gloo communicator.
Every rank writes its OWN gradients; Model.step all-reduces the arena before AdamW runs, so the norm every rank clips by is the
norm of the SUMMED gradient, and the parameters stay identical across the ranks and equal to the single-process oracle."""

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import conftest
    from tinynn_autograd_amd import _lib
    _lib.install_test_twin(conftest.build_twin())
    import tinynn_autograd_amd as tn
    import ostep_oracle as oo
    import ostep_support as su
    from tinynn_autograd_amd.core.model import Model
    from tinynn_autograd_amd.core.losses import SoftmaxCrossEntropyLoss
    from tinynn_autograd_amd.core.optimizer import AdamW
    comm = tn.dist.init_from_env(backend="gloo")
    rank, world = comm.rank, comm.world
    dtype = np.float64
    tn.set_default_float(dtype)
    opt_kw, orc_kw = su.hyper_kwargs()
    opt = AdamW(**opt_kw)
    net, xshape = su.dense_net()
    model = Model(net=net, loss=SoftmaxCrossEntropyLoss(), optimizer=opt, comm=comm)
    for p in model._live_params():
        p.values = tn.asarray(np.asarray(p.values).astype(dtype), dtype=dtype)
    decay = [d for _n, d in su.names_and_decay(model)]
    want = su.host_params(model)
    state = oo.new_state(want)
    for s in range(3):
        per_rank = [su.draw_grads(model, np.random.RandomState(100 * s + r), dtype) for r in range(world)]
        su.backward_then_inject(model, xshape, per_rank[rank], dtype, None, real_backward=False)
        model.step()
        summed = [sum(g[i] for g in per_rank) for i in range(len(want))]
        want = oo.adamw_step(want, summed, state, decay, **orc_kw)
        su.assert_params(model, want, dtype, "rank %d step %d" % (rank, s + 1))
        st = opt.state()
        np.testing.assert_allclose(st["gnorm"], state["gnorm"], rtol=1e-12)       # the GLOBAL norm, on every rank
        own = oo.global_norm(per_rank[rank])
        assert abs(st["gnorm"] - own) > 1e-3 * own                               # ... not the rank's own
        assert st["t"] == s + 1 and st["coef"] < 1.0
    flat = np.concatenate([np.asarray(p.values).ravel() for p in model._live_params()])
    both = np.asarray(comm.allgather(tn.asarray(flat, dtype=dtype)))
    assert np.array_equal(both[0], both[-1]), "parameters diverged across ranks"
    comm.barrier()
    print("ostep_dp_worker rank %d/%d ok" % (rank, world))


if __name__ == "__main__":
    main()
