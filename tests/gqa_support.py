"""TEST INFRASTRUCTURE shared by tests/gen_gqa_golden.py (CPU twin) and tests/test_gpu_gqa.py (MI355X): the raw calls of one
route as numpy arrays, and gqa_oracle's two-block grouped-query language model as a Net."""

import os

import numpy as np

import decode_support as ds
import gqa_oracle as go
import token_support as ts
import tinynn_autograd_amd as tn
from norm_support import dev
from tinynn_autograd_amd import device_array as da
from tinynn_autograd_amd.core.layers import BLOCK_PARAM_ORDER, Dense, Embedding, LayerNorm, TransformerBlock
from tinynn_autograd_amd.core.nn import Net
from tinynn_autograd_amd.core.tensor import Tensor

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gqa_cases.npz")
bits = ds.bits


def load_golden():
    with np.load(GOLDEN) as data:
        return dict(data)


def run_training(route, q, k, v, do_, causal, scale, dtype, unaligned=False, need=(True, True, True)):
    """The three raw calls of one route -> {name: numpy array or None}."""
    qd, kd, vd, dod = (dev(a, dtype, unaligned) for a in (q, k, v, do_))
    opts = dict(causal=causal, scale=scale, route=route)
    o, lse = da.gqa_attention(qd, kd, vd, **opts)
    dq, delta = da.gqa_attention_bwd_q(qd, kd, vd, o, dod, lse, need_dq=need[0], **opts)
    dk, dv = da.gqa_attention_bwd_kv(qd, kd, vd, dod, lse, delta, need_dk=need[1], need_dv=need[2], **opts)
    out = dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv)
    return {n: None if a is None else np.asarray(a) for n, a in out.items()}


def ragged_poisoned(case, lens, dtype):
    """The caches with every sequence's rows from its own length on (from row 0 for a negative length) set to NaN."""
    kc, vc = (np.array(case[n], dtype=dtype) for n in ("k_cache", "v_cache"))
    for b, n in enumerate(lens):
        for c in (kc, vc):
            (c[b, max(n, 0):] if case["layout"] == "bthd" else c[b, :, max(n, 0):])[...] = np.nan
    return kc, vc


def run_decode(route, case, dtype, splits=None, unaligned=False, lens=None):
    """One raw call of one route -> (o, k_cache, v_cache) as numpy arrays, the caches AFTER the call; the rows beyond the live
    prefix (the row about to be appended included) hold NaN before it.  lens: the ragged call with these lengths (the
    poison then starts at every sequence's own length)."""
    layout = case["layout"]
    if lens is None:
        kc, vc = (ds.poisoned(case[n], layout, case["length"], dtype) for n in ("k_cache", "v_cache"))
    else:
        kc, vc = ragged_poisoned(case, lens, dtype)
    kd, vd, qd = dev(kc, dtype, unaligned), dev(vc, dtype, unaligned), dev(case["q"], dtype, unaligned)
    kn, vn = dev(case["k_new"], dtype, unaligned), dev(case["v_new"], dtype, unaligned)
    o = da.gqa_decode(qd, kd, vd, None if lens is not None else case["length"], kn, vn,
                      lens=None if lens is None else da.lengths(lens), scale=case.get("scale"), layout=layout, route=route,
                      splits=splits)
    return np.asarray(o), np.asarray(kd), np.asarray(vd)


def make_decode_case(seed, layout, b, h, hkv, tmax, length, d, dv, append, dtype):
    q, kc, vc, kn, vn = go.decode_inputs(np.random.RandomState(seed), layout, b, h, hkv, tmax, d, dv, dtype)
    return dict(q=q, k_cache=kc, v_cache=vc, length=length, k_new=kn if append else None, v_new=vn if append else None, layout=layout)


def decode_reference(case, dtype, splits):
    return go.decode_reference(case["q"], case["k_cache"], case["v_cache"], case["length"], case["k_new"], case["v_new"],
                               case.get("scale"), case["layout"], dtype, splits)


def lm_net(params, dtype=np.float32, fused=True):
    """gqa_oracle.LM as a Net with the parameters `params` ({name: float64}, gqa_oracle.lm_params)."""
    c = go.LM
    rows = ts.load_example().Rows
    blocks = [TransformerBlock(c["H"], hidden=c["hidden"], num_in=c["E"], causal=True, eps=c["eps"], fused=fused,
                               kv_heads=c["Hkv"]) for _ in range(c["blocks"])]
    net = Net([Embedding(c["V"], c["E"], max_len=c["max_len"], fused=fused)] + blocks +
              [LayerNorm(c["E"], eps=c["eps"], fused=fused), rows(), Dense(c["V"], num_in=c["E"], fused=fused)])
    tensor = lambda name: Tensor(params[name].astype(dtype), requires_grad=True, dtype=dtype)
    net.set_parameters([{"tok": tensor("emb.tok"), "pos": tensor("emb.pos")}] +
                       [{name: tensor("block%d.%s" % (i, name)) for name in BLOCK_PARAM_ORDER} for i in range(c["blocks"])] +
                       [{"gamma": tensor("ln.gamma"), "beta": tensor("ln.beta")}, {}, {"w": tensor("head.w"), "b": tensor("head.b")}])
    return net


def lm_last_logits(net, ids, dtype=np.float32):
    """The last-position logits [B, V] of a full forward (no cache) as float64."""
    from tinynn_autograd_amd import generation as gen
    tn.set_default_float(dtype)
    out = np.asarray(gen._forward(net.layers, Tensor(np.asarray(ids, dtype=np.int64)), 0, None).values, dtype=np.float64)
    return out.reshape(ids.shape[0], ids.shape[1], -1)[:, -1]
