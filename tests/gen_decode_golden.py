"""Writes tests/golden/decode_cases.npz: the float64 results of decode_oracle's named cases (inputs are regenerated from seeds,
not stored), each cross-checked here against torch in float64, and the greedy generation of the one-block language model.

    decode.<name>     o [B, H, Dv] of decode_oracle.DECODE_CASES (torch: scaled_dot_product_attention over the live prefix)
    sample.<name>.u   the uniform numbers of decode_oracle.SAMPLE_CASES, float32-exact, each more than MARGIN = 4 cdf_bounds
                      inside its token's interval for float32 AND float64 operands (redrawn until it is)
    sample.<name>.ids the rule's tokens (torch: softmax + cumsum over the kept columns, float64)
    lm.head_scale     the power of two the head's weights of token_oracle.lm_initial() are scaled by: doubled until EVERY
                      greedy step's top-2 logit margin exceeds 4 x lm.logit_bound
    lm.logit_bound    max |torch float32 - torch float64| over the last-position logits of every step — the reference's own
                      float32 discrepancy, as in tests/gen_token_golden.py
    lm.ids            the greedy continuation [B, P + N] (torch float64 agrees token for token)

Both conditions are ASSERTED here and again in tests/test_decode_golden.py; no case is skipped.  The tests never import torch.

    python tests/gen_decode_golden.py
"""

import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_oracle as do                                                  # noqa: E402
import token_oracle as to                                                   # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_cases.npz")


def torch_decode(case):
    layout, n = case["layout"], case["length"] + (case["k_new"] is not None)
    kc, vc = case["k_cache"], case["v_cache"]
    if case["k_new"] is not None:
        kc, vc = do.put_row(kc, layout, case["length"], case["k_new"]), do.put_row(vc, layout, case["length"], case["v_new"])
    k, v = (torch.tensor(np.asarray(do.live_rows(a, layout, n), dtype=np.float64)) for a in (kc, vc))
    if layout == "bthd":
        k, v = k.transpose(1, 2), v.transpose(1, 2)
    q = torch.tensor(np.asarray(case["q"], dtype=np.float64))[:, :, None, :]
    return F.scaled_dot_product_attention(q, k, v)[:, :, 0].numpy()


def torch_sample(x, temperature, top_k, u, dtype):
    z = torch.tensor(do.tempered(x, temperature, dtype))
    out = []
    for r in range(z.shape[0]):
        kept = torch.tensor(do.kept_set(z[r].numpy(), top_k))
        p = torch.where(kept, torch.softmax(torch.where(kept, z[r], torch.tensor(-np.inf, dtype=torch.float64)), 0), torch.tensor(0.0, dtype=torch.float64))
        hit = torch.nonzero(kept & (torch.cumsum(p, 0) > float(u[r])))
        out.append(int(hit[0]) if len(hit) else int(torch.nonzero(p > 0)[-1]))
    return np.array(out, dtype=np.int64)


def torch_lm_logits(params, ids, dtype):
    c = to.LM_CASE
    p = {k: torch.tensor(np.asarray(v, dtype=np.float64), dtype=dtype) for k, v in params.items()}
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
    return (ln @ p["head.w"] + p["head.b"]).reshape(b, t, c["V"]).numpy().astype(np.float64)


def lm_fixture():
    """Doubles the head scale until every greedy step's top-2 margin exceeds MARGIN x the float32 discrepancy of torch."""
    prompt = do.lm_prompt()
    scale = 1.0
    for _ in range(12):
        params = do.lm_params(scale)
        ids, steps = do.lm_generate(params, prompt, do.LM_NEW)
        bound = 0.0
        for n in range(do.LM_NEW):
            prefix = ids[:, :do.LM_PROMPT + n]
            l64, l32 = torch_lm_logits(params, prefix, torch.float64)[:, -1], torch_lm_logits(params, prefix, torch.float32)[:, -1]
            assert np.abs(l64 - steps[n]).max() <= 1e-11 * np.abs(l64).max(), n
            assert np.array_equal(np.argmax(l64, axis=1), ids[:, do.LM_PROMPT + n])
            bound = max(bound, float(np.abs(l32 - l64).max()))
        margin = do.top2_margin(steps)
        print("lm head_scale %g: top-2 margin %.3e, float32 logit bound %.3e" % (scale, margin, bound))
        if margin > do.MARGIN * bound:
            return scale, bound, margin, ids
        scale *= 2.0
    raise AssertionError("no head scale gives the margin")


def main():
    out = {}
    for name in sorted(do.DECODE_CASES):
        case = do.decode_case(name, np.float32)
        res = do.decode_reference(case["q"], case["k_cache"], case["v_cache"], case["length"], case["k_new"], case["v_new"], None,
                                  case["layout"], np.float32, case["splits"])
        theirs = torch_decode(case)
        assert np.abs(res.values["o"] - theirs).max() <= 1e-12 * np.abs(theirs).max(), name
        out["decode." + name] = res.values["o"]
        print("decode %-14s o %s, max bound %.3e" % (name, res.values["o"].shape, res.bounds["o"].max()))
    for name in sorted(do.SAMPLE_CASES):
        x, temperature, top_k = do.sample_case(name, np.float32)
        refs = [do.sample_reference(x, temperature, top_k, dt) for dt in (np.float32, np.float64)]
        rs = np.random.RandomState(do.case_seed(name + ".u"))
        for _ in range(1000):
            u = do.draw_u(refs[0], rs, np.float32)
            if all((r.margins(u) > do.MARGIN).all() for r in refs):
                break
        else:
            raise AssertionError(name)
        ids = refs[0].tokens(u)
        for r, dt in zip(refs, (np.float32, np.float64)):
            assert np.array_equal(r.tokens(u), ids) and (r.margins(u) > do.MARGIN).all(), name
            assert np.array_equal(torch_sample(x, temperature, top_k, u, dt), ids), name
        out["sample.%s.u" % name], out["sample.%s.ids" % name] = u.astype(np.float32), ids
        print("sample %-14s ids %s, least margin %.1f bounds" % (name, ids, min(r.margins(u).min() for r in refs)))
    scale, bound, margin, ids = lm_fixture()
    assert margin > do.MARGIN * bound
    out["lm.head_scale"], out["lm.logit_bound"], out["lm.ids"] = np.float64(scale), np.float64(bound), ids
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
