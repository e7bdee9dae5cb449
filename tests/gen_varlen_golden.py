"""Writes tests/golden/varlen_cases.npz: the float64 results of varlen_support's named cases (inputs are regenerated from
seeds, not stored), each cross-checked here against torch in float64 — scaled_dot_product_attention and autograd per sequence
on the operands cut to lens[b] rows.

    varlen.<name>.<field>     o, lse, dq, dk, dv of varlen_support.VARLEN_CASES, in the case's layout, zeros at dead elements

The tests never import torch.

    python tests/gen_varlen_golden.py
"""

import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import varlen_support as vs                                                 # noqa: E402

OUT = vs.GOLDEN
STORED = ("o", "lse", "dq", "dk", "dv")


def torch_case(q, k, v, do_, lens, causal, scale, layout):
    out = {n: np.zeros(s) for n, s in (("o", do_.shape), ("dq", q.shape), ("dk", k.shape), ("dv", v.shape))}
    scale = float(1.0 / np.sqrt(q.shape[-1]) if scale is None else scale)
    for b, n in enumerate(int(x) for x in lens):
        if n == 0:
            continue
        tq, tk, tv, tg = (torch.tensor(np.asarray(a[b:b + 1, :n], dtype=np.float64), requires_grad=True) for a in (q, k, v, do_))
        if layout == "bthd":
            group = q.shape[2] // k.shape[2]
            hq, hk, hv = tq.transpose(1, 2), tk.repeat_interleave(group, dim=2).transpose(1, 2), tv.repeat_interleave(group, dim=2).transpose(1, 2)
        else:
            hq, hk, hv = tq, tk, tv
        o = F.scaled_dot_product_attention(hq, hk, hv, is_causal=bool(causal), scale=scale)
        o = o.transpose(1, 2) if layout == "bthd" else o
        o.backward(tg.detach())
        for name, t in (("o", o), ("dq", tq.grad), ("dk", tk.grad), ("dv", tv.grad)):
            out[name][b:b + 1, :n] = t.detach().numpy()
    return out


def main():
    out = {}
    for name in sorted(vs.VARLEN_CASES):
        q, k, v, do_, lens, causal, scale, layout = vs.case_input(name, np.float32)
        res = vs.reference(q, k, v, do_, lens, causal, scale, layout, np.float32)
        theirs = torch_case(q, k, v, do_, lens, causal, scale, layout)
        for field, want in theirs.items():
            assert np.abs(res.values[field] - want).max() <= 1e-11 * max(np.abs(want).max(), 1.0), (name, field)
        for field in STORED:
            out["varlen.%s.%s" % (name, field)] = res.values[field]
        print("varlen %-18s lens %s, o %s, max bound %.3e" % (name, lens.tolist(), res.values["o"].shape, res.bounds["o"].max()))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
