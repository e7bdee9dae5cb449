"""TEST INFRASTRUCTURE shared by tests/test_decode_host.py (CPU twin) and tests/test_gpu_decode.py (MI355X): the raw calls of
one route as numpy arrays, and the fixture's language model as a Net."""

import os

import numpy as np

import decode_oracle as do
import token_oracle as to
import token_support as ts
import tinynn_autograd_amd as tn
from norm_support import dev
from tinynn_autograd_amd import device_array as da
from tinynn_autograd_amd.core.layers import BLOCK_PARAM_ORDER
from tinynn_autograd_amd.core.tensor import Tensor

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_cases.npz")


def load_golden():
    with np.load(GOLDEN) as data:
        return dict(data)


def poisoned(cache, layout, live, dtype):
    """The cache with every row from `live` on set to NaN: rows beyond the live prefix must never be read."""
    out = np.array(cache, dtype=dtype)
    if layout == "bthd":
        out[:, live:] = np.nan
    else:
        out[:, :, live:] = np.nan
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def run_decode(route, case, dtype, splits=None, unaligned=False, poison=True):
    """One raw call of one route -> (o, k_cache, v_cache) as numpy arrays, the caches AFTER the call.  poison: the rows
    beyond the live prefix (the row about to be appended included) hold NaN before the call."""
    layout, length = case["layout"], case["length"]
    kc, vc = (poisoned(case[n], layout, length, dtype) if poison else np.asarray(case[n], dtype=dtype) for n in ("k_cache", "v_cache"))
    kd, vd, qd = dev(kc, dtype, unaligned), dev(vc, dtype, unaligned), dev(case["q"], dtype, unaligned)
    kn, vn = dev(case["k_new"], dtype, unaligned), dev(case["v_new"], dtype, unaligned)
    o = da.attention_decode(qd, kd, vd, length, kn, vn, scale=case.get("scale"), layout=layout, route=route, splits=splits)
    return np.asarray(o), np.asarray(kd), np.asarray(vd)


def expected_caches(case, dtype, poison=True):
    """What the caches must hold after the call, bit for bit: row `length` replaced by k_new / v_new, nothing else touched."""
    layout, length = case["layout"], case["length"]
    kc, vc = (poisoned(case[n], layout, length, dtype) if poison else np.asarray(case[n], dtype=dtype) for n in ("k_cache", "v_cache"))
    if case["k_new"] is not None:
        kc = do.put_row(kc, layout, length, np.asarray(case["k_new"], dtype=dtype))
        vc = do.put_row(vc, layout, length, np.asarray(case["v_new"], dtype=dtype))
    return kc, vc


def make_case(seed, layout, b, h, tmax, length, d, dv, append, dtype):
    q, kc, vc, kn, vn = do.decode_inputs(np.random.RandomState(seed), layout, b, h, tmax, d, dv, dtype)
    return dict(q=q, k_cache=kc, v_cache=vc, length=length, k_new=kn if append else None, v_new=vn if append else None, layout=layout)


def reference(case, dtype, splits):
    return do.decode_reference(case["q"], case["k_cache"], case["v_cache"], case["length"], case["k_new"], case["v_new"],
                               case.get("scale"), case["layout"], dtype, splits)


def run_sample(route, x, u, temperature, top_k, dtype):
    xd = dev(x, dtype)
    ud = None if u is None else dev(u, dtype)
    ids = da.sample_rows(xd, ud, temperature=temperature, top_k=top_k, route=route)
    assert ids.dtype == np.int64 and tuple(ids.shape) == (x.shape[0],)
    return np.asarray(ids)


def lm_net(golden, fused, dtype):
    """The fixture's language model (token_oracle.LM_CASE, head scaled by lm.head_scale) as a Net in phase TRAIN."""
    net = ts.lm_net(fused, dtype)
    values = do.lm_params(float(golden["lm.head_scale"]))
    tensor = lambda name: Tensor(values[name].astype(dtype), requires_grad=True, dtype=dtype)
    net.set_parameters([{"tok": tensor("emb.tok"), "pos": tensor("emb.pos")},
                        {name: tensor("block." + name) for name in BLOCK_PARAM_ORDER},
                        {"gamma": tensor("ln.gamma"), "beta": tensor("ln.beta")}, {},
                        {"w": tensor("head.w"), "b": tensor("head.b")}])
    return net
