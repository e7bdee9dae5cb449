"""TEST INFRASTRUCTURE — the float64 yardstick of grouped-query attention: numpy only, built on attn_oracle and decode_oracle,
which it imports unchanged.  H query heads share Hkv key / value heads, group = H / Hkv, query head h reads key / value head
h // group; layout "bthd" for the training operands.

The float64 result IS multi-head attention on k and v repeated over the group (np.repeat along the head axis: head h of the
repeat is head h // group).  Bounds:

    o, lse, dq     the per-head bounds of attn_oracle as they stand (a query head does not see that its k / v are shared)
    dk, dv         dk[hk] = sum over the group's heads h of d_h (the per-head gradient against the repeated operand).  Each d_h
                   carries attn_oracle's per-head bound b_h; adding the `group` contributions in ANY order (in one
                   accumulator, as the native kernel does, or after the fact, as the composed route does) costs at most
                   (group - 1) u sum_h |d_h| to first order, stated here as group u sum_h |d_h64|:
                       |dk - dk64| <= sum_h b_h + group u sum_h |d_h64|
    decode o       decode_oracle's bound per query head; the per-query rescale count R is unchanged (every query keeps its
                   own (m, l, acc) and meets the same steps, tree levels, waves and splits)

assert_within keeps attn_oracle's median gate, a condition on the inputs: the amplitudes are attn_oracle's (q <= 4, k 1, v 3,
do 1).  tests/gen_gqa_golden.py checks on the CPU that the oracle alone meets the gate on every case."""

import numpy as np

import attn_oracle as ao
import decode_oracle as do

unit, case_seed, assert_within, check = ao.unit, ao.case_seed, ao.assert_within, ao.check
FIELDS = ao.FIELDS
MAX_GROUP = 8             # TNN_GQA_MAX_GROUP (tests/test_gqa_abi.py ties it to the header)


def expand(x, group, axis=2):
    """k or v (or a cache) with every head repeated `group` times along the head axis."""
    return np.repeat(np.asarray(x), group, axis=axis)


def fold(x, group):
    """[B, T, H, W] -> [B, T, Hkv, W]: the sum over every key / value head's group of query heads."""
    b, t, h, w = x.shape
    return x.reshape(b, t, h // group, group, w).sum(axis=3)


def reference(q, k, v, do_=None, causal=False, scale=None, dtype=np.float32):
    """Forward, gradients for `do_` (None: forward only) and the bounds for an evaluation in `dtype`; q [B, Tq, H, D],
    k [B, Tk, Hkv, D], v [B, Tk, Hkv, Dv].  values["dk"] / ["dv"] have the shapes of k / v."""
    group = q.shape[2] // k.shape[2]
    assert group * k.shape[2] == q.shape[2] and k.shape[2] == v.shape[2]
    res = ao.reference(q, expand(k, group), expand(v, group), do_, causal, scale, "bthd", dtype)
    if do_ is None:
        return res
    u = unit(dtype)
    for name in ("dk", "dv"):
        per_head, bound = res.values[name], res.bounds[name]
        res.values[name] = fold(per_head, group)
        res.bounds[name] = fold(bound, group) + group * u * fold(np.abs(per_head), group)
    return res


def head_axis(layout):
    return 2 if layout == "bthd" else 1


def decode_reference(q, k_cache, v_cache, length, k_new=None, v_new=None, scale=None, layout="bthd", dtype=np.float32, splits=1):
    """decode_oracle.decode_reference on the caches repeated over the group: values["o"] [B, H, Dv], bounds["o"], and the
    Hkv-head caches after the append (values["k_cache"], ["v_cache"])."""
    ax = head_axis(layout)
    group = q.shape[1] // k_cache.shape[ax]
    assert group * k_cache.shape[ax] == q.shape[1]
    res = do.decode_reference(q, expand(k_cache, group, ax), expand(v_cache, group, ax), length,
                              None if k_new is None else expand(k_new, group, 1),
                              None if v_new is None else expand(v_new, group, 1), scale, layout, dtype, splits)
    if k_new is not None:
        k_cache, v_cache = do.put_row(k_cache, layout, length, k_new), do.put_row(v_cache, layout, length, v_new)
    res.values["k_cache"], res.values["v_cache"] = np.asarray(k_cache), np.asarray(v_cache)
    return res


# ---------------------------------------------------------------------- inputs
def make_inputs(rs, b, h, hkv, tq, tk, d, dv, dtype=np.float32, q_amp=4.0):
    """(q, k, v, do) in layout "bthd" with attn_oracle's amplitudes: q <= 4, k 1, v 3, do 1."""
    return ((rs.randn(b, tq, h, d) * q_amp).astype(dtype), rs.randn(b, tk, hkv, d).astype(dtype),
            (rs.randn(b, tk, hkv, dv) * 3).astype(dtype), rs.randn(b, tq, h, dv).astype(dtype))


def decode_inputs(rs, layout, b, h, hkv, tmax, d, dv, dtype=np.float32, q_amp=4.0):
    """(q, k_cache, v_cache, k_new, v_new) with attn_oracle's amplitudes."""
    return ((rs.randn(b, h, d) * q_amp).astype(dtype), rs.randn(*do.cache_shape(layout, b, hkv, tmax, d)).astype(dtype),
            (rs.randn(*do.cache_shape(layout, b, hkv, tmax, dv)) * 3).astype(dtype), rs.randn(b, hkv, d).astype(dtype),
            (rs.randn(b, hkv, dv) * 3).astype(dtype))


# name -> (B, H, Hkv, Tq, Tk, D, Dv, causal, scale (None: 1 / sqrt(D)))          the fixture's cases (tests/gen_gqa_golden.py)
GQA_CASES = {
    "mqa_small": (2, 4, 1, 7, 7, 5, 3, False, None),
    "group2_causal": (1, 4, 2, 17, 17, 8, 8, True, None),
    "group3_more_keys": (2, 3, 1, 9, 20, 6, 4, True, 0.7),
    "group1": (1, 2, 2, 11, 13, 16, 16, False, None),
    "group9_composed": (1, 9, 1, 5, 6, 4, 4, True, None),
}

# name -> (layout, B, H, Hkv, Tmax, length, D, Dv, append, splits)
GQA_DECODE_CASES = {
    "append_bthd": ("bthd", 2, 4, 2, 96, 70, 16, 24, True, 2),
    "append_bhtd_mqa": ("bhtd", 1, 3, 1, 140, 129, 17, 5, True, 3),
    "first_token": ("bthd", 1, 8, 1, 8, 0, 4, 3, True, 1),
    "no_append": ("bhtd", 2, 4, 2, 64, 64, 64, 65, False, 1),
}


def case_input(name, dtype=np.float32):
    b, h, hkv, tq, tk, d, dv, causal, scale = GQA_CASES[name]
    rs = np.random.RandomState(case_seed("gqa." + name))
    return make_inputs(rs, b, h, hkv, tq, tk, d, dv, dtype, q_amp=2.0) + (causal, scale)


def decode_case(name, dtype=np.float32):
    layout, b, h, hkv, tmax, length, d, dv, append, splits = GQA_DECODE_CASES[name]
    q, kc, vc, kn, vn = decode_inputs(np.random.RandomState(case_seed("gqa.decode." + name)), layout, b, h, hkv, tmax, d, dv, dtype)
    return dict(q=q, k_cache=kc, v_cache=vc, length=length, k_new=kn if append else None, v_new=vn if append else None,
                layout=layout, splits=splits)


# ---------------------------------------------------------------------- a two-block grouped-query language model, greedy
# token_oracle's block applied twice to the PLAIN parameters (plain_params: the grouped model's key / value column blocks
# repeated over the group — the same function), token_oracle's embedding, norm_oracle's final layer norm, a Dense head.
LM = dict(B=2, V=13, E=16, H=4, Hkv=2, hidden=32, max_len=12, eps=1e-5, blocks=2, prompt=4, new=7)
LM_MARGIN = 4.0           # decode_oracle.MARGIN: the summation orders of two float32 evaluations differ


def lm_shapes():
    import norm_oracle as no
    c = LM
    kv = c["E"] // c["H"] * c["Hkv"]
    shapes = [("emb.tok", (c["V"], c["E"])), ("emb.pos", (c["max_len"], c["E"]))]
    for i in range(c["blocks"]):
        for name, shape in no.block_shapes(c["E"], c["hidden"]).items():
            if name in ("attn.wk", "attn.wv", "attn.bk", "attn.bv"):
                shape = (shape[0], kv)
            shapes.append(("block%d.%s" % (i, name), shape))
    return shapes + [("ln.gamma", (1, c["E"])), ("ln.beta", (1, c["E"])), ("head.w", (c["E"], c["V"])), ("head.b", (1, c["V"]))]


def lm_params(seed, head_scale):
    """{name: float64}: multiples of 2**-10 drawn as token_oracle.lm_initial draws them, the head scaled by a power of two."""
    rs = np.random.RandomState(seed)
    out = {}
    for name, shape in lm_shapes():
        if name.endswith(".gamma"):
            vals = 1.0 + 0.25 * rs.randn(*shape)
        elif name.startswith("emb."):
            vals = 0.5 * rs.randn(*shape)
        elif shape[0] == 1:
            vals = 0.1 * rs.randn(*shape)
        else:
            vals = rs.uniform(-1.0, 1.0, shape) * np.sqrt(6.0 / (shape[0] + shape[1]))
        out[name] = np.round(vals * 1024.0) / 1024.0
    out["head.w"], out["head.b"] = out["head.w"] * head_scale, out["head.b"] * head_scale
    return out


def lm_prompt(seed):
    return np.random.RandomState(seed + 1).randint(0, LM["V"], (LM["B"], LM["prompt"])).astype(np.int64)


def lm_logits(p, ids):
    """float64 logits [B, T, V] of the model for ids [B, T]."""
    import norm_oracle as no
    import token_oracle as to
    c = LM
    b, t = ids.shape
    h = to.embedding_reference(p["emb.tok"], ids, p["emb.pos"]).values["out"]
    for i in range(c["blocks"]):
        names = [n for n in p if n.startswith("block%d." % i)]
        blk = {n.split(".", 1)[1]: p[n] for n in names}
        attn = plain_params([blk["attn." + n] for n in ("wq", "bq", "wk", "bk", "wv", "bv", "wo", "bo")], c["H"], c["Hkv"])
        blk.update(zip(("attn." + n for n in ("wq", "bq", "wk", "bk", "wv", "bv", "wo", "bo")), attn))
        h, _ = to._block(blk, h, c["H"], c["eps"])
    ln = no.reference(h, p["ln.gamma"], p["ln.beta"], None, "layer", c["eps"]).values["y"].reshape(b * t, c["E"])
    return (ln @ p["head.w"] + p["head.b"]).reshape(b, t, c["V"])


def lm_generate(p, prompt, new):
    """(ids [B, P + new], last-position logits of every step [new, B, V]) of greedy generation in float64."""
    ids, steps = np.array(prompt), []
    for _ in range(new):
        last = lm_logits(p, ids)[:, -1]
        steps.append(last)
        ids = np.concatenate([ids, np.argmax(last, axis=1)[:, None]], axis=1)
    return ids, np.stack(steps)


# ---------------------------------------------------------------------- float64 grouped MultiHeadAttention replica
def plain_params(params, heads, kv_heads):
    """The parameters of a plain MultiHeadAttention(heads) that computes what the grouped layer computes: wk / wv / bk / bv with
    every key / value head's column block repeated over its group (order wq bq wk bk wv bv wo bo)."""
    group = heads // kv_heads
    out = [np.asarray(a) for a in params]
    for at in (2, 3, 4, 5):
        a = out[at]
        hd = a.shape[1] // kv_heads
        out[at] = np.repeat(a.reshape(a.shape[0], kv_heads, hd), group, axis=1).reshape(a.shape[0], heads * hd)
    return out


def fold_columns(g, heads, kv_heads):
    """The group sums of a plain layer's [rows, H hd] gradient column blocks -> [rows, Hkv hd]."""
    group = heads // kv_heads
    hd = g.shape[1] // heads
    return np.asarray(g).reshape(g.shape[0], kv_heads, group, hd).sum(axis=2).reshape(g.shape[0], kv_heads * hd)
