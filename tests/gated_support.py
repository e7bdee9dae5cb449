"""TEST INFRASTRUCTURE shared by tests/test_gated_golden.py and tests/test_gated_host.py (CPU twin) and
tests/test_gpu_gated.py (MI355X): the fixture, raw tnn_gated_fwd / tnn_gated_bwd calls on operands laid out with chosen row
strides and base offsets inside sentinel-filled buffers, and a gated TransformerBlock with given parameters."""

import os

import numpy as np

import tinynn_autograd_amd as tn
from tinynn_autograd_amd import _lib
from tinynn_autograd_amd import device_array as da
from tinynn_autograd_amd import gated as gt
from tinynn_autograd_amd.core.layers import BLOCK_PARAM_ORDER, TransformerBlock
from tinynn_autograd_amd.core.tensor import Tensor

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gated_cases.npz")
SENTINEL = -123456.0


def load_golden():
    with np.load(GOLDEN) as data:
        return dict(data)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


class Buf(object):
    """[M, width] rows with row stride `ld`, `shift` elements into a 1-D device buffer that holds SENTINEL everywhere else."""

    def __init__(self, M, width, ld, shift, dtype, init=None):
        self.M, self.width, self.ld, self.shift, self.dtype = M, width, ld, shift, np.dtype(dtype)
        host = np.full(shift + M * ld, SENTINEL, dtype=dtype)
        self.rows = (shift + np.arange(M)[:, None] * ld + np.arange(width)[None, :]).reshape(-1)
        if init is not None:
            host[self.rows] = np.asarray(init, dtype=dtype).reshape(-1)
        self.before = host
        self.dev = tn.asarray(host, dtype=dtype)
        self.ptr = self.dev._ptr + shift * self.dtype.itemsize

    def column(self, c):
        return self.ptr + c * self.dtype.itemsize

    def read(self):
        """(the rows as [M, width], True when nothing outside them has changed)."""
        host = np.asarray(self.dev)
        outside = np.ones(host.size, dtype=bool)
        outside[self.rows] = False
        return host[self.rows].reshape(self.M, self.width), bool(np.array_equal(bits(host[outside]), bits(self.before[outside])))


def code(dtype):
    return _lib.F32 if np.dtype(dtype) == np.float32 else _lib.F64


def raw_fwd(act, dtype, gate, up=None, packed=False, ld_extra=0, shift=0, blocks=0):
    """ONE tnn_gated_fwd call -> (y [M, F], padding and surroundings untouched).  packed: gate and up are the halves of one
    [M, 2 F] buffer (ld = 2 F + ld_extra); otherwise every operand has ld = F + ld_extra.  shift: elements every base is moved by."""
    M, F = gate.shape
    if packed:
        z = Buf(M, 2 * F, 2 * F + ld_extra, shift, dtype, np.concatenate([gate, up], axis=1))
        g_ptr, u_ptr, ld_in = z.ptr, z.column(F), z.ld
    else:
        gb = Buf(M, F, F + ld_extra, shift, dtype, gate)
        ub = None if up is None else Buf(M, F, F + ld_extra, shift, dtype, up)
        g_ptr, u_ptr, ld_in = gb.ptr, None if ub is None else ub.ptr, gb.ld
    yb = Buf(M, F, F + ld_extra, shift, dtype)
    _lib.get().gated_fwd(g_ptr, u_ptr, yb.ptr, M, F, da._i64arr((ld_in, ld_in, yb.ld)), gt.ACTS.index(act), blocks, code(dtype))
    return yb.read()


def raw_bwd(act, dtype, gate, up, dy, packed=False, ld_extra=0, shift=0, blocks=0, need=(True, True)):
    """ONE tnn_gated_bwd call -> (dgate, dup, untouched); packed: the inputs AND the outputs are halves of [M, 2 F] buffers."""
    M, F = gate.shape
    need_dgate, need_dup = need
    if packed:
        z = Buf(M, 2 * F, 2 * F + ld_extra, shift, dtype, np.concatenate([gate, up], axis=1))
        g_ptr, u_ptr, ld_in = z.ptr, z.column(F), z.ld
        dz = Buf(M, 2 * F, 2 * F + ld_extra, shift, dtype)
        dg_ptr, du_ptr, ld_out = dz.ptr, dz.column(F), dz.ld
    else:
        gb = Buf(M, F, F + ld_extra, shift, dtype, gate)
        ub = None if up is None else Buf(M, F, F + ld_extra, shift, dtype, up)
        g_ptr, u_ptr, ld_in = gb.ptr, None if ub is None else ub.ptr, gb.ld
        dgb = Buf(M, F, F + ld_extra, shift, dtype) if need_dgate else None
        dub = Buf(M, F, F + ld_extra, shift, dtype) if need_dup else None
        dg_ptr, du_ptr, ld_out = (None if dgb is None else dgb.ptr), (None if dub is None else dub.ptr), F + ld_extra
    dyb = Buf(M, F, F + ld_extra, shift, dtype, dy)
    _lib.get().gated_bwd(g_ptr, u_ptr, dyb.ptr, dg_ptr, du_ptr, M, F, da._i64arr((ld_in, ld_in, dyb.ld, ld_out, ld_out)),
                         gt.ACTS.index(act), blocks, code(dtype))
    if packed:
        both, clean = dz.read()
        return both[:, :F], both[:, F:], clean
    dgate, c1 = dgb.read() if dgb is not None else (None, True)
    dup, c2 = dub.read() if dub is not None else (None, True)
    return dgate, dup, c1 and c2


def composed(act, dtype, gate, up, dy):
    """{y, dgate, dup} of the composed route as numpy arrays."""
    g, u, d = (None if a is None else tn.asarray(np.asarray(a, dtype=dtype), dtype=dtype) for a in (gate, up, dy))
    y = da.gated(g, u, act=act, route="composed")
    dgate, dup = da.gated_bwd(g, u, d, act=act, route="composed")
    return dict(y=np.asarray(y), dgate=np.asarray(dgate), dup=None if dup is None else np.asarray(dup))


def block(params, heads, hidden, dtype, mlp="swiglu", fused=True, causal=True, eps=1e-5):
    """A TransformerBlock(mlp=) holding `params` ({name of BLOCK_PARAM_ORDER: array})."""
    e = params["ln1.gamma"].shape[-1]
    blk = TransformerBlock(heads, hidden=hidden, num_in=e, causal=causal, eps=eps, fused=fused, mlp=mlp)
    for name in BLOCK_PARAM_ORDER:
        assert tuple(blk.params[name].shape) == tuple(params[name].shape), name
        blk.params[name] = Tensor(np.asarray(params[name], dtype=dtype), requires_grad=True, dtype=dtype)
    return blk


def block_grads(blk, x, y, dtype):
    """(loss, {name: gradient}) of ((block(x) - y) ** 2).sum() / B through the autograd graph, as float64."""
    tn.set_default_float(dtype)
    for name in BLOCK_PARAM_ORDER:
        blk.params[name].zero_grad()
    out = blk.forward(Tensor(np.asarray(x, dtype=dtype), dtype=dtype))
    err = out - Tensor(np.asarray(y, dtype=dtype), dtype=dtype)
    loss = (err * err).sum() / float(x.shape[0])
    loss.backward()
    return float(np.asarray(loss.values)), {n: np.asarray(blk.params[n].grad, dtype=np.float64) for n in BLOCK_PARAM_ORDER}


LM = dict(V=11, E=16, H=2, hidden=24, max_len=16, B=2, prompt=4, new=6, eps=1e-5)


def lm_net(dtype=np.float32, fused=True, mlp="swiglu", seed=5):
    """A one-block language model with a gated feed-forward and parameters drawn from `seed`: Embedding with learned positions,
    TransformerBlock(mlp=), LayerNorm, the example's Rows, a Dense head.  The head's weights are of order 1, so that the greedy
    choice does not hang on rounding."""
    import gated_oracle as go
    import token_support as ts
    from tinynn_autograd_amd.core.layers import Dense, Embedding, LayerNorm
    from tinynn_autograd_amd.core.nn import Net
    c = LM
    rs = np.random.RandomState(seed)
    rows = ts.load_example().Rows
    net = Net([Embedding(c["V"], c["E"], max_len=c["max_len"], fused=fused),
               TransformerBlock(c["H"], hidden=c["hidden"], num_in=c["E"], causal=True, eps=c["eps"], fused=fused, mlp=mlp),
               LayerNorm(c["E"], eps=c["eps"], fused=fused), rows(), Dense(c["V"], num_in=c["E"], fused=fused)])
    tensor = lambda a: Tensor(np.asarray(a, dtype=dtype), requires_grad=True, dtype=dtype)
    blk = go.block_params(seed, c["E"], c["hidden"], scale=2.0)
    net.set_parameters([{"tok": tensor(rs.randn(c["V"], c["E"])), "pos": tensor(0.5 * rs.randn(c["max_len"], c["E"]))},
                        {name: tensor(blk[name]) for name in BLOCK_PARAM_ORDER},
                        {"gamma": tensor(1.0 + 0.1 * rs.randn(1, c["E"])), "beta": tensor(0.1 * rs.randn(1, c["E"]))}, {},
                        {"w": tensor(rs.randn(c["E"], c["V"])), "b": tensor(0.1 * rs.randn(1, c["V"]))}])
    prompt = rs.randint(0, c["V"], size=(c["B"], c["prompt"])).astype(np.int64)
    return net, prompt


def lm_margin(net, ids, dtype=np.float32):
    """The smallest top-2 margin of the last-position logits [B, V] of a full forward over `ids`."""
    from tinynn_autograd_amd import generation as gen
    tn.set_default_float(dtype)
    out = np.asarray(gen._forward(net.layers, Tensor(np.asarray(ids, dtype=np.int64)), 0, None).values, dtype=np.float64)
    last = np.sort(out.reshape(ids.shape[0], ids.shape[1], -1)[:, -1], axis=-1)
    return float((last[:, -1] - last[:, -2]).min())


def count_calls(monkeypatch):
    """Wrap every bound entry point of the loaded library that launches or copies (the gated and rotary ones included);
    returns the list the names of the calls are appended to."""
    lib, seen = _lib.get(), []
    tables = [getattr(_lib, name) for name in dir(_lib) if name.endswith("_SIGNATURES")]
    quiet = {"malloc", "free", "last_error", "pool_stats", "stream_sync", "backend_kind"}
    for table in tables:
        for name in table:
            short = name[4:]
            if short in quiet or not hasattr(lib, short):
                continue
            real = getattr(lib, short)

            def call(*args, _real=real, _short=short):
                seen.append(_short)
                return _real(*args)
            monkeypatch.setattr(lib, short, call)
    return seen
