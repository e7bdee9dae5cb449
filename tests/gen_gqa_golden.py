"""Writes tests/golden/gqa_cases.npz: the float64 results of gqa_oracle's named cases (inputs are regenerated from seeds, not
stored), produced by this project's oracle alone.

    attn.<name>.<field>    o, lse, dq, dk, dv of gqa_oracle.GQA_CASES
    decode.<name>          o [B, H, Dv] of gqa_oracle.GQA_DECODE_CASES
    lm.*                   the two-block grouped-query language model's fixture (lm_fixture below)

Checked here, on the CPU, for float32 AND float64 evaluation:
  * an independent float64 evaluation — a loop over the query heads that indexes k / v by h // group, no repeat — agrees with
    the oracle to 1e-12 (the repeat is only a way of writing the head mapping);
  * the oracle alone meets attn_oracle's median gate on every field of every case: the oracle's own values lie within the
    bounds (trivially) AND the bounds are tight enough to test something.

    python tests/gen_gqa_golden.py
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_oracle as ao                                                    # noqa: E402
import gqa_oracle as go                                                     # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gqa_cases.npz")


def by_heads(q, k, v, do_, causal, scale):
    """The same mathematics head by head: query head h against key / value head h // group; dk / dv added per head."""
    group = q.shape[2] // k.shape[2]
    out = {"o": np.zeros(q.shape[:3] + (v.shape[3],)), "lse": np.zeros((q.shape[0], q.shape[2], q.shape[1])),
           "dq": np.zeros(q.shape), "dk": np.zeros(k.shape), "dv": np.zeros(v.shape)}
    scale = 1.0 / np.sqrt(q.shape[3]) if scale is None else scale
    for h in range(q.shape[2]):
        hk = h // group
        one = ao.reference(q[:, :, h:h + 1], k[:, :, hk:hk + 1], v[:, :, hk:hk + 1], do_[:, :, h:h + 1], causal, scale, "bthd")
        out["o"][:, :, h:h + 1], out["lse"][:, h:h + 1], out["dq"][:, :, h:h + 1] = (one.values[n] for n in ("o", "lse", "dq"))
        out["dk"][:, :, hk:hk + 1] += one.values["dk"]
        out["dv"][:, :, hk:hk + 1] += one.values["dv"]
    return out


def lm_fixture():
    """The seed and the head scale of gqa_oracle's two-block grouped-query model: the first seed, and the smallest power of
    two, at which EVERY greedy step's float64 top-2 logit margin exceeds 2 x LM_MARGIN x lm.logit_bound.
        lm.logit_bound   max |float32 - float64| over the last-position logits of every step, the float32 evaluation being
                         this package's composed route on the CPU twin — the discrepancy of a float32 evaluation as such
        lm.ids           the greedy continuation [B, P + N] of the float64 oracle
    Two float32 evaluations of one step (cached or not, captured or not, native or composed) each lie within LM_MARGIN bounds of
    the oracle, so they pick the oracle's token at every step."""
    import conftest
    from tinynn_autograd_amd import _lib
    import gqa_support as gs
    _lib.install_test_twin(conftest.build_twin())
    c = go.LM
    for seed in range(20):
        scale = 1.0
        for _ in range(6):
            params, prompt = go.lm_params(seed, scale), go.lm_prompt(seed)
            ids, steps = go.lm_generate(params, prompt, c["new"])
            net = gs.lm_net(params, np.float32, fused=False)
            net.set_phase("TEST")
            bound = max(np.abs(gs.lm_last_logits(net, ids[:, :c["prompt"] + n]) - steps[n]).max() for n in range(c["new"]))
            srt = np.sort(steps, axis=-1)
            margin = float((srt[..., -1] - srt[..., -2]).min())
            if margin > 2 * go.LM_MARGIN * bound:
                print("lm: seed %d, head scale %g, top-2 margin %.3e, logit bound %.3e" % (seed, scale, margin, bound))
                return {"lm.seed": np.int64(seed), "lm.head_scale": np.float64(scale), "lm.logit_bound": np.float64(bound),
                        "lm.ids": ids}
            scale *= 2.0
    raise AssertionError("no seed gives the margin")


def main():
    data = {}
    for name in go.GQA_CASES:
        q, k, v, do_, causal, scale = go.case_input(name)
        loop = by_heads(*(np.asarray(a, dtype=np.float64) for a in (q, k, v, do_)), causal, scale)
        for dtype in (np.float32, np.float64):
            res = go.reference(q, k, v, do_, causal, scale, dtype)
            for field in go.FIELDS:
                np.testing.assert_allclose(res.values[field], loop[field], rtol=0, atol=1e-12 * max(1.0, np.abs(loop[field]).max()))
                go.assert_within(res.values[field], res.values[field], res.bounds[field], "%s %s (oracle alone)" % (name, field))
        for field in go.FIELDS:
            data["attn.%s.%s" % (name, field)] = res.values[field]
    for name in go.GQA_DECODE_CASES:
        case = go.decode_case(name)
        for dtype in (np.float32, np.float64):
            res = go.decode_reference(dtype=dtype, **case)
            go.assert_within(res.values["o"], res.values["o"], res.bounds["o"], "decode %s (oracle alone)" % name)
        data["decode." + name] = res.values["o"]
    data.update(lm_fixture())
    np.savez_compressed(OUT, **data)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(data), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
