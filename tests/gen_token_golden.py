"""Writes tests/golden/token_cases.npz: the float64 outputs and gradients of token_oracle's named cases (inputs are regenerated
from seeds, not stored; one flat array per case: token_oracle.pack), each cross-checked here against torch.nn.functional
embedding / cross_entropy and torch autograd in float64, and the language-model case of token_oracle.LM_CASE from torch in
float64: the initial parameters (float16, exact), the loss, every parameter gradient of one step, and per gradient tensor

    scale    = max|torch float64|        (attn.bk, whose gradient is mathematically zero: the largest sum of |terms| behind
                                          an element, as in tests/gen_norm_golden.py)
    f32_gate = 4 * max|torch float32 - torch float64| / scale

— the reference's own float32 discrepancy; the factor 4 because the summation orders differ.  The tests never import torch.

    python tests/gen_token_golden.py
"""

import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import norm_oracle as no                                                    # noqa: E402
import token_oracle as to                                                   # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "token_cases.npz")


def close(ours, theirs, what, tol=1e-12):
    ours, theirs = np.asarray(ours, dtype=np.float64), np.asarray(theirs, dtype=np.float64).reshape(np.shape(ours))
    both_inf = np.isinf(ours) & (ours == theirs)
    worst = np.abs(np.where(both_inf, 0.0, ours - theirs)).max() if ours.size else 0.0
    assert worst <= tol * max(1.0, float(np.abs(ours[np.isfinite(ours)]).max()) if ours.size else 1.0), (what, worst)


def torch_lm(params, ids, targets, dtype):
    c = to.LM_CASE
    p = {k: torch.tensor(np.asarray(v, dtype=np.float64), dtype=dtype, requires_grad=True) for k, v in params.items()}
    b, t = ids.shape
    e, h_, hd = c["E"], c["H"], c["E"] // c["H"]
    keep = torch.tril(torch.ones(t, t, dtype=torch.bool))
    x = F.embedding(torch.tensor(ids), p["emb.tok"]) + p["emb.pos"][:t]
    blk = lambda n: p["block." + n]
    ln1 = F.layer_norm(x, (e,), blk("ln1.gamma")[0], blk("ln1.beta")[0], c["eps"]).reshape(b * t, e)
    q, k, v = ((ln1 @ blk("attn.w" + n) + blk("attn.b" + n)).reshape(b, t, h_, hd).transpose(1, 2) for n in "qkv")
    s = (q @ k.transpose(-1, -2) / hd ** 0.5).masked_fill(~keep, float("-inf"))
    att = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(b * t, e)
    h = x + (att @ blk("attn.wo") + blk("attn.bo")).reshape(b, t, e)
    ln2 = F.layer_norm(h, (e,), blk("ln2.gamma")[0], blk("ln2.beta")[0], c["eps"]).reshape(b * t, e)
    z = F.gelu(ln2 @ blk("fc1.w") + blk("fc1.b"), approximate="tanh")
    out = h + (z @ blk("fc2.w") + blk("fc2.b")).reshape(b, t, e)
    ln = F.layer_norm(out, (e,), p["ln.gamma"][0], p["ln.beta"][0], c["eps"]).reshape(b * t, e)
    logits = ln @ p["head.w"] + p["head.b"]
    loss = F.cross_entropy(logits, torch.tensor(targets.reshape(-1)), ignore_index=to.LM_IGNORE)
    loss.backward()
    return float(loss.detach()), {k: v.grad.detach().numpy().astype(np.float64) for k, v in p.items()}


def main():
    out = {}
    for name in to.EMBED_CASES:
        table, ids, pos, dy, padding_idx = to.embed_case(name)
        res = to.embedding_reference(table, ids, pos, dy, padding_idx)
        tt = torch.tensor(table.astype(np.float64), requires_grad=True)
        tp = None if pos is None else torch.tensor(pos.astype(np.float64), requires_grad=True)
        ty = F.embedding(torch.tensor(ids), tt, padding_idx=padding_idx)
        if tp is not None:
            ty = ty + tp[:ids.shape[-1]]
        ty.backward(torch.tensor(dy.astype(np.float64)))
        close(res.values["out"], ty.detach().numpy(), name + " out")
        close(res.values["dtable"], tt.grad.numpy(), name + " dtable")
        if tp is not None:
            close(res.values["dpos"], tp.grad.numpy(), name + " dpos")
        out[name] = to.pack(res.values, to.embed_fields(name))
    for name in to.XENT_CASES:
        x, t, ignore_index, reduction, g = to.xent_case(name)
        res = to.cross_entropy_reference(x, t, ignore_index, reduction, g)
        xt = torch.tensor(x.astype(np.float64), requires_grad=True)
        tl = F.cross_entropy(xt, torch.tensor(t), ignore_index=-100 if ignore_index is None else ignore_index, reduction=reduction)
        if res.values["count"] > 0:                           # (torch's mean over no row is NaN; ours is defined as 0)
            tl.backward(torch.tensor(float(g), dtype=torch.float64))
            close(res.values["loss"], tl.detach().numpy(), name + " loss")
            close(res.values["dlogits"], xt.grad.numpy(), name + " dlogits")
        else:
            assert res.values["loss"] == 0.0 and not res.values["dlogits"].any()
        close(res.values["lse"], torch.logsumexp(xt, dim=1).detach().numpy(), name + " lse")
        out[name] = to.pack(res.values, to.xent_fields(name))

    params = to.lm_initial()
    ids, raw_targets = to.lm_data()
    targets = to.lm_targets(raw_targets)
    loss64, grads64 = torch_lm(params, ids, targets, torch.float64)
    _, grads32 = torch_lm(params, ids, targets, torch.float32)
    own_loss, own_grads, bk_terms = to.lm_loss_and_grads(params, ids, targets, with_bk_terms=True)
    assert abs(own_loss - loss64) <= 1e-12 * abs(loss64), (own_loss, loss64)
    scales = {name: float(np.abs(grads64[name]).max()) for name in to.LM_NAMES}
    scales["block.attn.bk"] = float(bk_terms.max())
    gates = []
    for name in to.LM_NAMES:
        assert np.abs(own_grads[name] - grads64[name]).max() <= 1e-11 * scales[name], name
        gates.append(4.0 * np.abs(grads32[name] - grads64[name]).max() / scales[name])
        print("f32_gate %-16s %.3e" % (name, gates[-1]))
    out["lm.params"] = to.pack(params, to.lm_layout()).astype(np.float16)
    assert np.array_equal(out["lm.params"].astype(np.float64), to.pack(params, to.lm_layout()))
    out["lm.ids"], out["lm.targets"] = ids, targets
    out["lm.grads"] = to.pack(grads64, to.lm_layout())
    out["lm.loss"] = np.float64(loss64)
    out["lm.f32_gate"] = np.array(gates)
    out["lm.grad_scale"] = np.array([scales[name] for name in to.LM_NAMES])
    print("lm loss %.12g" % loss64)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print("%s: %d arrays, %d bytes" % (OUT, len(out), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
