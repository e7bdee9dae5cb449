"""Writes tests/golden/norm_cases.npz: the float64 outputs and gradients of norm_oracle's named cases (inputs are regenerated
from seeds, not stored), each cross-checked here against torch.nn.functional.layer_norm / rms_norm / gelu and torch autograd
in float64 (one flat array per case: norm_oracle.pack), and the TransformerBlock case of norm_oracle.BLOCK_CASE from torch
in float64: the initial parameters (float16, exact), the loss, every parameter gradient, the losses of three Adam steps, and per gradient tensor

    scale    = max|torch float64|
    f32_gate = 4 * max|torch float32 - torch float64| / scale

— the reference's own float32 discrepancy; the factor 4 because the summation orders differ.  One tensor is different:
the gradient of attn.bk is mathematically zero (norm_oracle.block_loss_and_grads), torch's float64 value is 1e-17 of
rounding, and a scale taken from it would mean nothing; its scale is the largest sum of |terms| behind an element.  The
tests never import torch.

    python tests/gen_norm_golden.py
"""

import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import norm_oracle as no                                                    # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "norm_cases.npz")


def t64(a, grad=False):
    return None if a is None else torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=grad)


def torch_norm(x, gamma, beta, dy, kind, eps):
    xt, gt, bt = t64(x, True), t64(gamma, True), t64(beta, True)
    n = x.shape[-1]
    if kind == "layer":
        y = F.layer_norm(xt, (n,), gt, bt, eps)
    else:
        y = F.rms_norm(xt, (n,), gt, eps)
    y.backward(t64(dy))
    grab = lambda t: None if t is None else t.grad.numpy()
    return y.detach().numpy(), grab(xt), grab(gt), grab(bt)


def torch_block(params, x, y, dtype, steps=0, lr=1e-3):
    """(loss, grads) of the first evaluation and the losses of `steps` Adam steps, in `dtype`."""
    c = no.BLOCK_CASE
    p = {k: torch.tensor(np.asarray(v, dtype=np.float64), dtype=dtype, requires_grad=True) for k, v in params.items()}
    xt, yt = torch.tensor(x, dtype=dtype), torch.tensor(y, dtype=dtype)
    b, t, e = xt.shape
    h_, hd = c["H"], e // c["H"]
    keep = torch.tril(torch.ones(t, t, dtype=torch.bool))

    def loss_fn():
        ln1 = F.layer_norm(xt, (e,), p["ln1.gamma"][0], p["ln1.beta"][0], c["eps"]).reshape(b * t, e)
        q, k, v = ((ln1 @ p["attn.w" + n] + p["attn.b" + n]).reshape(b, t, h_, hd).transpose(1, 2) for n in "qkv")
        s = q @ k.transpose(-1, -2) / hd ** 0.5
        if c["causal"]:
            s = s.masked_fill(~keep, float("-inf"))
        att = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(b * t, e)
        h = xt + (att @ p["attn.wo"] + p["attn.bo"]).reshape(b, t, e)
        ln2 = F.layer_norm(h, (e,), p["ln2.gamma"][0], p["ln2.beta"][0], c["eps"]).reshape(b * t, e)
        z = F.gelu(ln2 @ p["fc1.w"] + p["fc1.b"], approximate="tanh")
        out = h + (z @ p["fc2.w"] + p["fc2.b"]).reshape(b, t, e)
        return ((out - yt) ** 2).sum() / b

    loss = loss_fn()
    loss.backward()
    grads = {k: v.grad.detach().numpy().astype(np.float64) for k, v in p.items()}
    first = float(loss.detach())
    losses = []
    if steps:
        opt = torch.optim.Adam([p[k] for k in no.BLOCK_NAMES], lr=lr, betas=(0.9, 0.999), eps=1e-8)
        for _ in range(steps):
            opt.zero_grad()
            step_loss = loss_fn()
            step_loss.backward()
            losses.append(float(step_loss.detach()))
            opt.step()
    return first, grads, np.array(losses)


def main():
    out = {}
    for name in no.NORM_CASES:
        x, gamma, beta, dy, kind, eps = no.case_input(name)
        res = no.reference(x, gamma, beta, dy, kind, eps)
        ty, tdx, tdg, tdb = torch_norm(x, gamma, beta, dy, kind, eps)
        pairs = [("y", ty), ("dx", tdx)] + ([("dgamma", tdg)] if gamma is not None else []) \
            + ([("dbeta", tdb)] if beta is not None else [])
        for field, theirs in pairs:
            ours = res.values[field]
            scale = max(1.0, float(np.abs(ours).max()))
            # float64 evaluations of the same formulas: rows around 1000 lose log2(1000 / 1.5) ~ 10 bits to the subtraction
            tol = 1e-12 * scale * (1000.0 if "offset" in name else 1.0)
            assert np.abs(ours - theirs.reshape(ours.shape)).max() <= tol, (name, field, np.abs(ours - theirs.reshape(ours.shape)).max())
        out[name] = no.pack(res.values, no.case_fields(name))
    for name, form in no.GELU_CASES.items():
        x, dy = no.gelu_input(40, no.case_seed(name))
        res = no.gelu_reference(x, dy, form)
        xt = t64(x, True)
        ty = F.gelu(xt, approximate=form)
        ty.backward(t64(dy))
        assert np.abs(res.values["y"] - ty.detach().numpy()).max() <= 1e-13 * 40, name
        assert np.abs(res.values["dx"] - xt.grad.numpy()).max() <= 1e-13 * 40, name
        out[name] = np.stack([res.values["y"], res.values["dx"]])

    c = no.BLOCK_CASE
    params = no.block_initial()
    x, y = no.block_data()
    loss64, grads64, losses64 = torch_block(params, x, y, torch.float64, steps=c["steps"], lr=c["lr"])
    _, grads32, _ = torch_block(params, x, y, torch.float32)
    own_loss, own_grads, bk_terms = no.block_loss_and_grads(params, x, y, c["H"], c["causal"], c["eps"], with_bk_terms=True)
    own_losses = no.block_adam_losses(params, x, y, c["H"], c["causal"], c["eps"], c["lr"], c["steps"])
    assert abs(own_loss - loss64) <= 1e-12 * abs(loss64)
    assert losses64[0] == loss64 and np.abs(own_losses - losses64).max() <= 1e-9 * abs(loss64), (own_losses, losses64)
    gates, scales = [], []
    for name in no.BLOCK_NAMES:
        ref = grads64[name]
        scale = float(bk_terms.max()) if name == "attn.bk" else float(np.abs(ref).max())
        assert np.abs(own_grads[name] - ref).max() <= 1e-11 * scale, name
        gate = 4.0 * np.abs(grads32[name] - ref).max() / scale
        gates.append(gate)
        scales.append(scale)
        print("f32_gate %-10s %.3e" % (name, gate))
    out["block.params"] = no.pack(params, no.block_layout()).astype(np.float16)
    assert np.array_equal(out["block.params"].astype(np.float64), no.pack(params, no.block_layout()))
    out["block.grads"] = no.pack(grads64, no.block_layout())
    out["block.loss"] = np.float64(loss64)
    out["block.adam_losses"] = losses64
    out["block.f32_gate"] = np.array(gates)
    out["block.grad_scale"] = np.array(scales)
    print("block loss %.12g, Adam losses %s" % (loss64, losses64))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print("%s: %d arrays, %d bytes" % (OUT, len(out), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
