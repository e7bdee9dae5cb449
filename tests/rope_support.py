"""TEST INFRASTRUCTURE shared by tests/gen_rope_golden.py and tests/test_rope_host.py (CPU twin) and tests/test_gpu_rope.py
(MI355X): the raw rope call of one route as numpy arrays, and rope_oracle's two-block rotary language model as a Net."""

import os

import numpy as np

import decode_support as ds
import rope_oracle as ro
import token_support as ts
import tinynn_autograd_amd as tn
from norm_support import dev
from tinynn_autograd_amd import device_array as da
from tinynn_autograd_amd import rope as rp
from tinynn_autograd_amd.core.layers import BLOCK_PARAM_ORDER, Dense, Embedding, LayerNorm, TransformerBlock
from tinynn_autograd_amd.core.nn import Net
from tinynn_autograd_amd.core.tensor import Tensor

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rope_cases.npz")
bits = ds.bits
_ROTARIES = {}


def load_golden():
    with np.load(GOLDEN) as data:
        return dict(data)


def rotary(R, pairing="half", max_len=ro.P):
    """ONE Rotary per (R, pairing, max_len) for the whole run: its device tables are uploaded once per dtype."""
    key = (R, pairing, max_len, tn.backend_name())
    if key not in _ROTARIES:
        _ROTARIES[key] = rp.Rotary(max_len, R, ro.BASE, pairing)
    return _ROTARIES[key]


def run(route, xa, xb, rot, dtype, offset=0, positions=None, layout="bthd", inverse=False, blocks=0, unaligned=False,
        inplace=False):
    """One raw call of one route -> (ya, yb or None) as numpy arrays."""
    xad, xbd = dev(xa, dtype, unaligned), dev(xb, dtype, unaligned)
    out = da.rope(xad, xbd, rotary=rot, offset=offset, positions=None if positions is None else da.lengths(positions),
                  layout=layout, inverse=inverse, route=route, blocks=blocks, out="inplace" if inplace else None)
    ya, yb = (out, None) if xb is None else out
    if inplace:
        assert ya is xad and (xb is None or yb is xbd)
    return np.asarray(ya), None if yb is None else np.asarray(yb)


def references(xa, xb, rot, dtype, offset=0, positions=None, layout="bthd", inverse=False):
    """(oracle result of xa, of xb or None) with the Rotary's own rounded tables."""
    R = rot.width(xa.shape[3])
    cos_t, sin_t = rot.host_tables(R, dtype)
    one = lambda x: None if x is None else ro.reference(x, cos_t, sin_t, offset, positions, layout, rot.pairing, inverse, dtype)
    return one(xa), one(xb)


def lm_net(params, dtype=np.float32, fused=True, max_len=None):
    """rope_oracle.LM as a Net with the parameters `params` ({name: float64}, rope_oracle.lm_params): an Embedding without a
    position table, blocks that share ONE Rotary."""
    c = ro.LM
    rows = ts.load_example().Rows
    rot = rp.Rotary(c["max_len"] if max_len is None else max_len, None, ro.BASE, "half")
    blocks = [TransformerBlock(c["H"], hidden=c["hidden"], num_in=c["E"], causal=True, eps=c["eps"], fused=fused,
                               kv_heads=c["Hkv"], rope=rot) for _ in range(c["blocks"])]
    net = Net([Embedding(c["V"], c["E"], fused=fused)] + blocks +
              [LayerNorm(c["E"], eps=c["eps"], fused=fused), rows(), Dense(c["V"], num_in=c["E"], fused=fused)])
    tensor = lambda name: Tensor(params[name].astype(dtype), requires_grad=True, dtype=dtype)
    net.set_parameters([{"tok": tensor("emb.tok")}] +
                       [{name: tensor("block%d.%s" % (i, name)) for name in BLOCK_PARAM_ORDER} for i in range(c["blocks"])] +
                       [{"gamma": tensor("ln.gamma"), "beta": tensor("ln.beta")}, {}, {"w": tensor("head.w"), "b": tensor("head.b")}])
    return net


def lm_last_logits(net, ids, dtype=np.float32):
    """The last-position logits [B, V] of a full forward (no cache) as float64."""
    from tinynn_autograd_amd import generation as gen
    tn.set_default_float(dtype)
    out = np.asarray(gen._forward(net.layers, Tensor(np.asarray(ids, dtype=np.int64)), 0, None).values, dtype=np.float64)
    return out.reshape(ids.shape[0], ids.shape[1], -1)[:, -1]


def attention_grads(route, q, k, v, do_, rot, dtype):
    """loss = sum(do * attention_gqa(rope(q), rope(k), v)), causal, through the autograd nodes -> (dq, dk, the device's rotated
    q and k) as numpy arrays."""
    from tinynn_autograd_amd.core import ops
    tn.set_default_float(dtype)
    qt, kt, vt = (Tensor(np.asarray(a, dtype=dtype), requires_grad=True, dtype=dtype) for a in (q, k, v))
    qr, kr = ops.rope_(qt, kt, rotary=rot, route=route)
    out = ops.attention_gqa_(qr, kr, vt, causal=True, route=route)
    (out * Tensor(np.asarray(do_, dtype=dtype), dtype=dtype)).sum().backward()
    return np.asarray(qt.grad), np.asarray(kt.grad), np.asarray(qr.values), np.asarray(kr.values)
