"""Writes tests/golden/extend_cases.npz: the float64 results of extend_oracle's named cases (inputs are regenerated from seeds,
not stored), each cross-checked here against torch in float64 (scaled_dot_product_attention with the explicit mask
j <= length + i over the concatenated keys).

    extend.<name>     o of extend_oracle.EXTEND_CASES, in the case's layout

The tests never import torch.

    python tests/gen_extend_golden.py
"""

import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import extend_oracle as eo                                                  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "extend_cases.npz")


def torch_extend(case):
    layout, length = case["layout"], case["length"]
    t_axis, h_axis = eo.AXES[layout]
    t = case["q"].shape[t_axis]
    group = case["q"].shape[h_axis] // case["k_cache"].shape[h_axis]
    cat = lambda c, new: np.concatenate([eo.rows_of(c, layout, 0, length), new], axis=t_axis)
    q, k, v = (torch.tensor(np.asarray(a, dtype=np.float64)) for a in
               (case["q"], np.repeat(cat(case["k_cache"], case["k_new"]), group, axis=h_axis),
                np.repeat(cat(case["v_cache"], case["v_new"]), group, axis=h_axis)))
    if layout == "bthd":
        q, k, v = q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)
    keep = torch.arange(length + t)[None, :] <= (length + torch.arange(t))[:, None]
    scale = case["scale"] if case["scale"] is not None else 1.0 / np.sqrt(q.shape[-1])
    o = F.scaled_dot_product_attention(q, k, v, attn_mask=keep, scale=float(scale))
    return (o.transpose(1, 2) if layout == "bthd" else o).numpy()


def main():
    out = {}
    for name in sorted(eo.EXTEND_CASES):
        case = eo.extend_case(name, np.float32)
        res = eo.extend_reference(case["q"], case["k_cache"], case["v_cache"], case["length"], case["k_new"], case["v_new"],
                                  case["scale"], case["layout"], np.float32)
        theirs = torch_extend(case)
        assert np.abs(res.values["o"] - theirs).max() <= 1e-12 * np.abs(theirs).max(), name
        out["extend." + name] = res.values["o"]
        print("extend %-26s o %s, max bound %.3e" % (name, res.values["o"].shape, res.bounds["o"].max()))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
