"""Writes tests/golden/ostep_cases.npz: the inputs of the optimizer-step cases and what torch computes for them on the CPU in
float64 — torch.nn.utils.clip_grad_norm_ followed by torch.optim.AdamW with one decayed and one undecayed parameter group.
ONLY this generator imports torch; the tests read the fixture (tests/test_ostep_golden.py).

    python tests/gen_ostep_golden.py

Cases: 5 steps over 3 parameters of sizes 5 / 1 / 7 with flags decay / no / decay; max_norm below and above the gradient norm;
weight decay 0 and 0.1."""

import os

import numpy as np

SIZES = (5, 1, 7)
DECAY = (True, False, True)
STEPS = 5
LR, B1, B2, EPS = 1e-2, 0.9, 0.999, 1e-8
CASES = [("clip_wd", 1.0, 0.1), ("clip_nowd", 1.0, 0.0), ("noclip_wd", 100.0, 0.1), ("noclip_nowd", 100.0, 0.0)]
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ostep_cases.npz")


def inputs():
    rs = np.random.RandomState(20260)
    n = sum(SIZES)
    p0 = rs.standard_normal(n)
    grads = rs.uniform(0.1, 1.0, size=(STEPS, n)) * np.where(rs.rand(STEPS, n) < 0.5, -1.0, 1.0)
    grads[2] *= 40.0          # one step whose norm is far above the others (still below the "noclip" max_norm of 100)
    return p0, grads


def split(flat):
    out, off = [], 0
    for s in SIZES:
        out.append(flat[off:off + s])
        off += s
    return out


def torch_run(p0, grads, max_norm, wd):
    import torch
    params = [torch.tensor(a.copy(), dtype=torch.float64, requires_grad=True) for a in split(p0)]
    opt = torch.optim.AdamW([{"params": [p for p, d in zip(params, DECAY) if d], "weight_decay": wd},
                             {"params": [p for p, d in zip(params, DECAY) if not d], "weight_decay": 0.0}],
                            lr=LR, betas=(B1, B2), eps=EPS)
    traj, norms = [], []
    for s in range(STEPS):
        for p, g in zip(params, split(grads[s])):
            p.grad = torch.tensor(g.copy(), dtype=torch.float64)
        norms.append(float(torch.nn.utils.clip_grad_norm_(params, max_norm)))
        opt.step()
        traj.append(np.concatenate([p.detach().numpy().copy() for p in params]))
    return np.stack(traj), np.array(norms)


def main():
    p0, grads = inputs()
    arrays = {"sizes": np.array(SIZES, dtype=np.int64), "decay": np.array(DECAY, dtype=np.bool_), "p0": p0, "grads": grads,
              "hyper": np.array([LR, B1, B2, EPS]), "case_names": np.array([c[0] for c in CASES])}
    for name, max_norm, wd in CASES:
        traj, norms = torch_run(p0, grads, max_norm, wd)
        arrays[name + ".max_norm"] = np.float64(max_norm)
        arrays[name + ".wd"] = np.float64(wd)
        arrays[name + ".params"] = traj
        arrays[name + ".norms"] = norms
    np.savez(OUT, **arrays)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
