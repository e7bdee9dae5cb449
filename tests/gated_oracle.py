"""TEST INFRASTRUCTURE — the yardstick of the gated activations (include/tnn_gated.h): numpy only.  SiLU is evaluated in
numpy.longdouble, the two GELU forms by norm_oracle's float64 formulas (the functions the kernels share with tnn_gelu_*), and
every bound is DERIVED by propagating first-order rounding errors through the header's fixed expressions — computed from the
reference quantities, never from a result under test.  u, the libm gates, MEDIAN_GATE and assert_within are norm_oracle's.

With u = the unit roundoff of the dtype, X = EXP_ULP ulps (1 ulp = 2 u), g = gate, |.| elementwise:

  silu     e = exp(-|g|)                 b_e   = 2 X u e
           d = 1 + e                     b_d   = b_e + u d
           sig = 1 / d       (g >= 0)    b_sig = b_d / d^2 + u sig
           sig = e / d       (g < 0)     b_sig = b_e / d + e b_d / d^2 + u sig
           a = g sig                     b_a   = |g| b_sig + u |a| + tiny |g|          (e, and with it sig, is subnormal for
                                                                                        large |g|: one tiny(dtype) of absolute error)
           t = 1 - sig                   b_t   = b_sig + u |t|
           w = fma(g, t, 1)              b_w   = |g| b_t + u |w|
           s = sig w       (= act')      b_s   = |w| b_sig + sig b_w + u |s| + tiny (1 + |g|)
  gelu     b_a and b_s are norm_oracle.gelu_reference's bounds of y and of the slope (its dx for dy = 1, less the u |dx| of
           that product).
  outputs  y = a up                      b_y     = |up| b_a + u |y|                     (no up: y = a, b_y = b_a)
           dup = dy a                    b_dup   = |dy| b_a + u |dup|
           p = dy up, dgate = p s        b_dgate = |s| u |p| + |p| b_s + u |dgate|      (no up: p = dy exactly)

The bounds are worst-case; assert_within's median gate keeps them from hiding a defect."""

import numpy as np

from norm_oracle import EXP_ULP, MEDIAN_GATE, assert_within, gelu_reference, unit     # noqa: F401  (re-exported)

ACTS = ("silu", "gelu_tanh", "gelu")
_GELU_FORM = {"gelu_tanh": "tanh", "gelu": "none"}
SPECIALS = np.array([0.0, -0.0, 10.0, -10.0, 40.0, -40.0, 100.0, -100.0])


class Result(object):
    """values: name -> float64 array (None where the call has no such output); bounds: the same names."""

    def __init__(self):
        self.values, self.bounds = {}, {}


def act_reference(g, act, dtype):
    """(a, b_a, s, b_s) as float64 arrays: act(g), act'(g) and their bounds for an evaluation in `dtype`."""
    u = unit(dtype)
    tiny = float(np.finfo(np.dtype(dtype)).tiny)
    g64 = np.asarray(g, dtype=np.float64)
    if act == "silu":
        ld = np.longdouble
        gl = g64.astype(ld)
        e = np.exp(-np.abs(gl))
        d = 1 + e
        pos = gl >= 0
        sig = np.where(pos, 1 / d, e / d)
        b_e = 2 * EXP_ULP * u * e
        b_d = b_e + u * d
        b_sig = np.where(pos, b_d / d ** 2, b_e / d + e * b_d / d ** 2) + u * sig
        a = gl * sig
        b_a = np.abs(gl) * b_sig + u * np.abs(a) + tiny * np.abs(gl)
        t = 1 - sig
        b_t = b_sig + u * np.abs(t)
        w = gl * t + 1
        b_w = np.abs(gl) * b_t + u * np.abs(w)
        s = sig * w
        b_s = np.abs(w) * b_sig + sig * b_w + u * np.abs(s) + tiny * (1 + np.abs(gl))
        return tuple(np.asarray(v, dtype=np.float64) for v in (a, b_a, s, b_s))
    res = gelu_reference(g64, np.ones_like(g64), _GELU_FORM[act], dtype)
    s = res.values["dx"]
    return res.values["y"], res.bounds["y"], s, res.bounds["dx"] - u * np.abs(s)


def reference(gate, up=None, dy=None, act="silu", dtype=np.float32):
    """y and, with dy, dgate and dup (None without up) — values and bounds for an evaluation in `dtype` of inputs that are
    taken as exact."""
    u = unit(dtype)
    a, b_a, s, b_s = act_reference(gate, act, dtype)
    res = Result()
    up64 = None if up is None else np.asarray(up, dtype=np.float64)
    if up64 is None:
        res.values["y"], res.bounds["y"] = a, b_a
    else:
        y = a * up64
        res.values["y"], res.bounds["y"] = y, np.abs(up64) * b_a + u * np.abs(y)
    if dy is None:
        return res
    d = np.asarray(dy, dtype=np.float64)
    if up64 is None:
        p, b_p = d, np.zeros_like(d)
        res.values["dup"] = res.bounds["dup"] = None
    else:
        p = d * up64
        b_p = u * np.abs(p)
        dup = d * a
        res.values["dup"], res.bounds["dup"] = dup, np.abs(d) * b_a + u * np.abs(dup)
    dgate = p * s
    res.values["dgate"], res.bounds["dgate"] = dgate, np.abs(s) * b_p + np.abs(p) * b_s + u * np.abs(dgate)
    return res


def check(got, res, what, factor=1.0, verbose=False):
    """got: {name: array or None}; every named output that is there against the oracle."""
    for name in ("y", "dgate", "dup"):
        if got.get(name) is not None:
            want = res.values[name]
            assert want is not None, "%s: the call has no %s" % (what, name)
            assert_within(np.asarray(got[name]).reshape(np.shape(want)), want, res.bounds[name], "%s %s" % (what, name),
                          factor, verbose)


# ---------------------------------------------------------------------- inputs
def case_seed(name):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % (2 ** 31)


def make_inputs(M, F, seed, dtype=np.float32, specials=True):
    """(gate, up, dy), each [M, F]: gate starts (row-major) with SPECIALS — as many as fit — then 3 * normal; up and dy are
    normal.  float32 numbers whatever `dtype` holds them, so one fixture serves both precisions."""
    rs = np.random.RandomState(seed)
    gate = (3.0 * rs.randn(M * F)).astype(np.float32)
    if specials:
        k = min(gate.size, SPECIALS.size)
        gate[:k] = SPECIALS[:k]
    up, dy = rs.randn(M, F).astype(np.float32), rs.randn(M, F).astype(np.float32)
    return gate.reshape(M, F).astype(dtype), up.astype(dtype), dy.astype(dtype)


# name -> (act, M, F, with up)                                      the fixture's cases (tests/gen_gated_golden.py)
GOLDEN_CASES = {
    "swiglu_3x5": ("silu", 3, 5, True),
    "swiglu_2x8": ("silu", 2, 8, True),
    "silu_4x3": ("silu", 4, 3, False),
    "geglu_tanh_3x5": ("gelu_tanh", 3, 5, True),
    "gelu_tanh_2x4": ("gelu_tanh", 2, 4, False),
    "geglu_erf_3x5": ("gelu", 3, 5, True),
}


# ---------------------------------------------------------------------- float64 TransformerBlock(mlp="swiglu" / "geglu") replica
BLOCK_ACT = {"swiglu": "silu", "geglu": "gelu_tanh"}


def act64(g, act):
    """(act(g), act'(g)) in float64 by the plain formulas."""
    if act == "silu":
        sig = 1.0 / (1.0 + np.exp(-g))
        return g * sig, sig * (1.0 + g * (1.0 - sig))
    res = gelu_reference(g, np.ones_like(g), _GELU_FORM[act], np.float64)
    return res.values["y"], res.values["dx"]


def block_params(seed, e, hidden, scale=1.0):
    """Parameters of a gated block: fc1.w [E, 2 hidden] (gate columns, then up columns), fc2.w [hidden, E]."""
    import norm_oracle as no
    rs = np.random.RandomState(seed)
    shapes = no.block_shapes(e, hidden)
    shapes["fc1.w"], shapes["fc1.b"] = (e, 2 * hidden), (1, 2 * hidden)
    out = {}
    for name in no.BLOCK_NAMES:
        shape = shapes[name]
        if name.endswith(".gamma"):
            out[name] = 1.0 + 0.25 * rs.randn(*shape)
        elif shape[0] == 1:
            out[name] = 0.1 * rs.randn(*shape)
        else:
            out[name] = scale * rs.uniform(-1.0, 1.0, shape) * np.sqrt(6.0 / (shape[0] + shape[1]))
    return {k: np.round(v * 1024.0) / 1024.0 for k, v in out.items()}


def block_loss(params, x, y, heads, causal, eps, mlp="swiglu", grads=False, with_bk_terms=False):
    """float64 loss ((out - y) ** 2).sum() / B of the pre-norm block with a gated feed-forward; grads=True: (loss, the gradient of
    every parameter) by the analytic formulas (attention and norms as in norm_oracle.block_loss_and_grads); with_bk_terms: and,
    as a third value, the sum of |terms| behind every element of attn.bk's gradient [1, E], which is mathematically zero."""
    import math
    import norm_oracle as no
    act = BLOCK_ACT[mlp]
    p = {k: np.asarray(v, dtype=np.float64) for k, v in params.items()}
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    b, t, e = x.shape
    hd = e // heads
    f = p["fc2.w"].shape[0]
    ln1 = no.reference(x, p["ln1.gamma"], p["ln1.beta"], None, "layer", eps).values["y"]
    rows = ln1.reshape(b * t, e)
    q, k, v = ((rows @ p["attn.w" + n] + p["attn.b" + n]).reshape(b, t, heads, hd).transpose(0, 2, 1, 3) for n in "qkv")
    s = q @ k.transpose(0, 1, 3, 2) / math.sqrt(hd)
    if causal:
        s = np.where(np.arange(t)[None, :] <= np.arange(t)[:, None], s, -np.inf)
    pr = np.exp(s - s.max(axis=-1, keepdims=True))
    pr /= pr.sum(axis=-1, keepdims=True)
    att = (pr @ v).transpose(0, 2, 1, 3).reshape(b * t, e)
    h = x + (att @ p["attn.wo"] + p["attn.bo"]).reshape(b, t, e)
    ln2 = no.reference(h, p["ln2.gamma"], p["ln2.beta"], None, "layer", eps).values["y"].reshape(b * t, e)
    z = ln2 @ p["fc1.w"] + p["fc1.b"]
    gate, up = z[:, :f], z[:, f:]
    a, slope = act64(gate, act)
    mid = a * up
    out = h + (mid @ p["fc2.w"] + p["fc2.b"]).reshape(b, t, e)
    err = out - y
    loss = (err ** 2).sum() / b
    if not grads:
        return loss
    g = {}
    dout = 2.0 * err / b
    d2 = dout.reshape(b * t, e)
    g["fc2.w"], g["fc2.b"] = mid.T @ d2, d2.sum(0, keepdims=True)
    dmid = d2 @ p["fc2.w"].T
    dz = np.concatenate([(dmid * up) * slope, dmid * a], axis=1)
    g["fc1.w"], g["fc1.b"] = ln2.T @ dz, dz.sum(0, keepdims=True)
    r2 = no.reference(h, p["ln2.gamma"], p["ln2.beta"], (dz @ p["fc1.w"].T).reshape(b, t, e), "layer", eps).values
    g["ln2.gamma"], g["ln2.beta"] = r2["dgamma"].reshape(1, e), r2["dbeta"].reshape(1, e)
    dh2 = (dout + r2["dx"]).reshape(b * t, e)
    g["attn.wo"], g["attn.bo"] = att.T @ dh2, dh2.sum(0, keepdims=True)
    datt = (dh2 @ p["attn.wo"].T).reshape(b, t, heads, hd).transpose(0, 2, 1, 3)
    dv = pr.transpose(0, 1, 3, 2) @ datt
    dp = datt @ v.transpose(0, 1, 3, 2)
    ds = pr * (dp - (dp * pr).sum(axis=-1, keepdims=True)) / math.sqrt(hd)
    dq, dk = ds @ k, ds.transpose(0, 1, 3, 2) @ q
    drows = np.zeros((b * t, e))
    for n, dn in (("q", dq), ("k", dk), ("v", dv)):
        dn = dn.transpose(0, 2, 1, 3).reshape(b * t, e)
        g["attn.w" + n], g["attn.b" + n] = rows.T @ dn, dn.sum(0, keepdims=True)
        if n == "k":
            bk_terms = np.abs(dn).sum(0, keepdims=True)
        drows += dn @ p["attn.w" + n].T
    r1 = no.reference(x, p["ln1.gamma"], p["ln1.beta"], drows.reshape(b, t, e), "layer", eps).values
    g["ln1.gamma"], g["ln1.beta"] = r1["dgamma"].reshape(1, e), r1["dbeta"].reshape(1, e)
    out = {name: g[name] for name in no.BLOCK_NAMES}
    return (loss, out, bk_terms) if with_bk_terms else (loss, out)
