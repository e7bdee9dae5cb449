"""TEST INFRASTRUCTURE — the attention fixture tests/golden/attn_cases.npz.

    python tests/gen_attn_golden.py

The reference has no attention, so the fixture's numbers come from the float64 numpy oracle tests/attn_oracle.py; when torch
is importable every number is additionally asserted against a float64 CPU torch softmax chain and its
autograd, so the fixture has two independent parents.  Operands are rebuilt by attn_oracle.case_input from the case's seed
(numpy's legacy RandomState stream is frozen); the file holds results only: o, lse, dq, dk, dv per case."""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import attn_oracle as ao          # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "attn_cases.npz")


def torch_parent(torch, q, k, v, do, causal, scale, layout):
    t = [torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True) for a in (q, k, v)]
    tq, tk, tv = (a.permute(0, 2, 1, 3) for a in t) if layout == "bthd" else t
    scale = 1.0 / np.sqrt(q.shape[-1]) if scale is None else scale
    s = scale * (tq @ tk.transpose(-1, -2))
    if causal:
        keep = torch.tensor(ao.keep_mask(s.shape[-2], s.shape[-1], True))
        s = s.masked_fill(~keep, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    o = torch.softmax(s, dim=-1) @ tv
    if layout == "bthd":
        o = o.permute(0, 2, 1, 3)
    o.backward(torch.tensor(np.asarray(do, dtype=np.float64)))
    return dict(o=o.detach().numpy(), lse=lse.detach().numpy(), dq=t[0].grad.numpy(), dk=t[1].grad.numpy(), dv=t[2].grad.numpy())


def main():
    try:
        import torch
    except ImportError:
        torch = None
    out = {}
    for name in ao.ATTN_CASES:
        q, k, v, do, causal, scale, layout = ao.case_input(name)
        res = ao.reference(q, k, v, do, causal, scale, layout)
        if torch is not None:
            parent = torch_parent(torch, q, k, v, do, causal, scale, layout)
            for field in ao.FIELDS:
                np.testing.assert_allclose(res.values[field], parent[field].reshape(res.values[field].shape), rtol=1e-11,
                                           atol=1e-12, err_msg="%s %s" % (name, field))
        out.update({"%s.%s" % (name, field): res.values[field] for field in ao.FIELDS})
    np.savez_compressed(GOLDEN, **out)
    print("wrote %s: %d arrays, %d bytes%s" % (GOLDEN, len(out), os.path.getsize(GOLDEN),
                                               "" if torch is not None else " (torch absent: not cross-checked)"))


if __name__ == "__main__":
    main()
