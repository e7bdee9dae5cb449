"""TEST INFRASTRUCTURE — the float64 yardstick of layer norm, RMS norm and GELU (the reference has none): numpy only, the plain
formulas with their analytic gradients, the DERIVED first-order error bounds of the tests, and a float64 replica of one
TransformerBlock (squared-error loss of core/losses.py).

Bounds.  u = 2**-24 (float32) or 2 * 2**-53 (float64); |.| elementwise; mean_N / sum_M over the row / the rows; every bound
is computed from the float64 quantities, never from a result under test.  x is [M, N], d = x - mean.

  layer norm forward
    b_mean = (N + 1) u mean_N|x|                                      N - 1 additions and a division, any order
    b_d    = u |d| + u |mean| + b_mean
    b_var  = mean_N(2 |d| b_d) + (N + 3) u var                        squares, N - 1 additions, a division
    b_rstd = rstd (b_var / (2 (var + eps)) + 3 u)                     + eps, sqrt, 1 / .
    b_y    = |gamma| (b_d rstd + |d| b_rstd + 3 u |d| rstd) + u |y|   two products, the addition of beta
  RMS norm forward: the same with mean = 0, b_mean = b_d = 0 (d is x itself) and var = mean_N(x^2)
  backward (reads x, dy, gamma exactly and the mean, rstd of the forward with the errors above); xh = d rstd, g = dy gamma
    b_xh   = rstd b_d + |d| b_rstd + u |xh|
    b_g    = u |g|
    b_s1   = mean_N(b_g) + (N + 1) u mean_N|g|                         s1 = mean_N(g)          (absent for RMS norm)
    b_gx   = |g| b_xh + |xh| b_g + u |g xh|
    b_s2   = mean_N(b_gx) + (N + 1) u mean_N|g xh|                     s2 = mean_N(g xh)
    b_in   = b_g + b_s1 + b_xh |s2| + |xh| b_s2 + u |xh s2| + 2 u (|g| + |s1| + |xh s2|)
    b_dx   = b_rstd |inner| + rstd b_in + u |dx|                       dx = rstd (g - s1 - xh s2)
    b_dgamma = sum_M(|dy| b_xh + u |dy xh|) + (M + 1) u sum_M|dy xh|
    b_dbeta  = (M + 1) u sum_M|dy|
  GELU, E = ERF_ULP, T = TANH_ULP, X = EXP_ULP ulps (1 ulp = 2 u) for the device libm
    exact  z = x / sqrt(2): b_z = 2 u |z|;  e = erf(z): b_e = 2 E u |e| + erf'(z) b_z;  s = 1 + e: b_s = b_e + u |s|
           y = 0.5 x s: b_y = 0.5 |x| b_s + u |y|
           slope = 0.5 s + x pdf, pdf = exp(-x^2 / 2) / sqrt(2 pi): b_pdf = pdf (2 X u + 2 u x^2 / 2 + 2 u)
           b_slope = 0.5 b_s + |x| b_pdf + u |x pdf| + u |slope|
    tanh   w = x + A x^3: b_w = 4 u A |x|^3 + u |w|;  a = C w: b_a = C b_w + 2 u |a|;  t = tanh(a): b_t = 2 T u |t| +
           (1 - t^2) b_a;  s = 1 + t: b_s = b_t + u |s|;  y = 0.5 x s: as above
           slope = 0.5 s + 0.5 x q du, q = 1 - t^2, du = C (1 + 3 A x^2): b_q = 2 |t| b_t + u t^2 + u |q|, b_du = 4 u |du|
           b_slope = 0.5 b_s + 0.5 |x| (b_q |du| + |q| b_du) + 3 u |0.5 x q du| + u |slope|
    dx = dy slope: b_dx = |dy| b_slope + u |dx|
  ERF_ULP = 16: erf of the device libm is not among tests/kernel_sweep.ULP_GATES; 16 ulp is the accuracy the OpenCL
  specification demands of erf, which the device library is written to, and the most any gate of kernel_sweep may be.
  TANH_ULP = 3 and EXP_ULP = 2 are kernel_sweep's gates.

The bounds are worst-case and loose; so that one cannot hide a defect, assert_within also demands that the MEDIAN of
bound / (|ref| + tiny) over the elements is below MEDIAN_GATE — a condition on the inputs, not a measurement (rows without
an offset meet it at every N used here, rows of 1000 + 1.5 normal up to N = 257).  A reference that is exactly zero
everywhere is exempt: the result must then lie within the bound of zero."""

import math

import numpy as np

U32, U64 = 2.0 ** -24, 2.0 ** -53
ERF_ULP, TANH_ULP, EXP_ULP = 16.0, 3.0, 2.0
MEDIAN_GATE = 0.05
FIELDS = ("y", "mean", "rstd", "dx", "dgamma", "dbeta")
GELU_C, GELU_A = math.sqrt(2.0 / math.pi), 0.044715

try:
    from scipy.special import erf as _erf
except ImportError:                                   # numpy only: math.erf elementwise
    _erf = np.vectorize(math.erf, otypes=[np.float64])


def unit(dtype):
    return U32 if np.dtype(dtype) == np.float32 else 2.0 * U64


class Result(object):
    """values: name -> float64 array (None where the kind has no such field); bounds: the same names -> elementwise bounds."""

    def __init__(self):
        self.values, self.bounds = {}, {}


def reference(x, gamma=None, beta=None, dy=None, kind="layer", eps=1e-5, dtype=np.float32):
    """Forward, gradients for `dy` (None: forward only) and the bounds for an evaluation in `dtype`.  x: [..., N]; the
    statistics have shape x.shape[:-1]; dgamma / dbeta have shape [N]."""
    u = unit(dtype)
    shape = np.shape(x)
    n = shape[-1]
    x2 = np.asarray(x, dtype=np.float64).reshape(-1, n)
    m = x2.shape[0]
    gam = np.ones(n) if gamma is None else np.asarray(gamma, dtype=np.float64).reshape(n)
    bet = np.zeros(n) if beta is None else np.asarray(beta, dtype=np.float64).reshape(n)
    layer = kind == "layer"
    if layer:
        mean = x2.mean(axis=1, keepdims=True)
        b_mean = (n + 1) * u * np.abs(x2).mean(axis=1, keepdims=True)
        d = x2 - mean
        b_d = u * np.abs(d) + u * np.abs(mean) + b_mean
    else:
        mean, b_mean = np.zeros((m, 1)), np.zeros((m, 1))
        d, b_d = x2, np.zeros_like(x2)
    var = (d * d).mean(axis=1, keepdims=True)
    b_var = (2 * np.abs(d) * b_d).mean(axis=1, keepdims=True) + (n + 3) * u * var
    with np.errstate(divide="ignore", invalid="ignore"):
        rstd = 1.0 / np.sqrt(var + eps)
        b_rstd = rstd * (b_var / (2 * (var + eps)) + 3 * u)
    y = d * rstd * gam + bet
    b_y = np.abs(gam) * (b_d * rstd + np.abs(d) * b_rstd + 3 * u * np.abs(d) * rstd) + u * np.abs(y)
    res = Result()
    stats = shape[:-1]
    res.values["y"], res.bounds["y"] = y.reshape(shape), b_y.reshape(shape)
    res.values["mean"], res.bounds["mean"] = (mean.reshape(stats), b_mean.reshape(stats)) if layer else (None, None)
    res.values["rstd"], res.bounds["rstd"] = rstd.reshape(stats), b_rstd.reshape(stats)
    if dy is None:
        return res
    g0 = np.asarray(dy, dtype=np.float64).reshape(-1, n)
    xh = d * rstd
    b_xh = rstd * b_d + np.abs(d) * b_rstd + u * np.abs(xh)
    g = g0 * gam
    b_g = u * np.abs(g)
    if layer:
        s1 = g.mean(axis=1, keepdims=True)
        b_s1 = b_g.mean(axis=1, keepdims=True) + (n + 1) * u * np.abs(g).mean(axis=1, keepdims=True)
    else:
        s1, b_s1 = np.zeros((m, 1)), np.zeros((m, 1))
    gx = g * xh
    b_gx = np.abs(g) * b_xh + np.abs(xh) * b_g + u * np.abs(gx)
    s2 = gx.mean(axis=1, keepdims=True)
    b_s2 = b_gx.mean(axis=1, keepdims=True) + (n + 1) * u * np.abs(gx).mean(axis=1, keepdims=True)
    inner = g - s1 - xh * s2
    b_in = (b_g + b_s1 + b_xh * np.abs(s2) + np.abs(xh) * b_s2 + u * np.abs(xh * s2)
            + 2 * u * (np.abs(g) + np.abs(s1) + np.abs(xh * s2)))
    dx = rstd * inner
    b_dx = b_rstd * np.abs(inner) + rstd * b_in + u * np.abs(dx)
    dgamma = (g0 * xh).sum(axis=0)
    b_dgamma = (np.abs(g0) * b_xh + u * np.abs(g0 * xh)).sum(axis=0) + (m + 1) * u * np.abs(g0 * xh).sum(axis=0)
    res.values["dx"], res.bounds["dx"] = dx.reshape(shape), b_dx.reshape(shape)
    res.values["dgamma"], res.bounds["dgamma"] = dgamma, b_dgamma
    if layer:
        res.values["dbeta"], res.bounds["dbeta"] = g0.sum(axis=0), (m + 1) * u * np.abs(g0).sum(axis=0)
    else:
        res.values["dbeta"], res.bounds["dbeta"] = None, None
    return res


def gelu_reference(x, dy=None, approximate="none", dtype=np.float32):
    """values / bounds of "y" and, with dy, "dx"."""
    u = unit(dtype)
    x = np.asarray(x, dtype=np.float64)
    ax = np.abs(x)
    if approximate == "none":
        z = x * math.sqrt(0.5)
        e = _erf(z)
        b_e = 2 * ERF_ULP * u * np.abs(e) + 2.0 / math.sqrt(math.pi) * np.exp(-z * z) * 2 * u * np.abs(z)
        s = 1.0 + e
        b_s = b_e + u * np.abs(s)
        pdf = np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
        b_pdf = pdf * (2 * EXP_ULP * u + u * x * x + 2 * u)
        slope = 0.5 * s + x * pdf
        b_slope = 0.5 * b_s + ax * b_pdf + u * np.abs(x * pdf) + u * np.abs(slope)
    elif approximate == "tanh":
        w = x + GELU_A * x ** 3
        b_w = 4 * u * GELU_A * ax ** 3 + u * np.abs(w)
        a = GELU_C * w
        b_a = GELU_C * b_w + 2 * u * np.abs(a)
        t = np.tanh(a)
        b_t = 2 * TANH_ULP * u * np.abs(t) + (1.0 - t * t) * b_a
        s = 1.0 + t
        b_s = b_t + u * np.abs(s)
        q = 1.0 - t * t
        du = GELU_C * (1.0 + 3.0 * GELU_A * x * x)
        b_q = 2 * np.abs(t) * b_t + u * t * t + u * np.abs(q)
        b_du = 4 * u * np.abs(du)
        second = 0.5 * x * q * du
        slope = 0.5 * s + second
        b_slope = 0.5 * b_s + 0.5 * ax * (b_q * np.abs(du) + np.abs(q) * b_du) + 3 * u * np.abs(second) + u * np.abs(slope)
    else:
        raise ValueError(approximate)
    res = Result()
    y = 0.5 * x * s
    res.values["y"], res.bounds["y"] = y, 0.5 * ax * b_s + u * np.abs(y)
    if dy is not None:
        g = np.asarray(dy, dtype=np.float64)
        dx = g * slope
        res.values["dx"], res.bounds["dx"] = dx, np.abs(g) * b_slope + u * np.abs(dx)
    return res


def gelu64(x, approximate):
    return gelu_reference(x, None, approximate).values["y"]


def assert_within(got, want, bound, what, factor=1.0, verbose=False, gate=True):
    """|got - want| <= factor * bound elementwise, and the bound is tight enough to mean something (module docstring)."""
    got = np.asarray(got, dtype=np.float64)
    want, bound = np.asarray(want, dtype=np.float64), factor * np.asarray(bound, dtype=np.float64)
    assert got.shape == want.shape, "%s: shape %s vs %s" % (what, got.shape, want.shape)
    if not got.size:
        return
    err = np.abs(got - want)
    tiny = np.finfo(np.float64).tiny
    if verbose:
        ratio = float((err / np.maximum(bound, tiny)).max()) if (bound > 0).any() else 0.0
        print("%s: max error %.3e, max bound %.3e, worst error / bound %.3f" % (what, err.max(), bound.max(), ratio))
    worst = float((err - bound).max())
    assert worst <= 0.0, "%s: error exceeds the derived bound by %.3e (max error %.3e, max bound %.3e)" % (
        what, worst, float(err.max()), float(bound.max()))
    if not gate or (want == 0).all():
        return
    med = float(np.median(bound / factor / (np.abs(want) + tiny)))
    assert med < MEDIAN_GATE, "%s: the bound is too loose to test anything (median bound / |ref| = %.3g)" % (what, med)


def check(got, res, what, fields=FIELDS, factor=1.0, verbose=False):
    """got: {name: array or None}; every named field that is there against the oracle."""
    for name in fields:
        if got.get(name) is not None:
            assert res.values[name] is not None, "%s: %s has no %s" % (what, what, name)
            want = res.values[name]
            assert_within(np.asarray(got[name]).reshape(np.shape(want)), want, res.bounds[name], "%s %s" % (what, name),
                          factor, verbose)


# ---------------------------------------------------------------------- inputs
def case_seed(name):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % (2 ** 31)


def make_inputs(rs, shape, dtype=np.float32, offset=0.0, spread=1.5, params=True, drift=0.0):
    """(x, gamma, beta, dy): x = offset + spread * normal; gamma around 1, beta around 0 ([N]); dy = normal + drift * (1 + the
    normal behind x).  drift > 0 gives the sums over MANY rows — dbeta = sum dy, dgamma = sum dy xh — an expectation of
    their own; with drift = 0 they are sums of terms of random sign, whose smallness is cancellation that the tightness
    gate of their bounds refuses once the rows are thousands."""
    n = shape[-1]
    z = rs.randn(*shape)
    x = (offset + spread * z).astype(dtype)
    gamma = (1.0 + 0.5 * rs.randn(n)).astype(dtype) if params else None
    beta = (0.5 * rs.randn(n)).astype(dtype) if params else None
    dy = (rs.randn(*shape) + drift * (1.0 + z)).astype(dtype)
    return x, gamma, beta, dy


# name -> (kind, shape, offset, eps, with parameters)                       the fixture's cases (tests/gen_norm_golden.py)
NORM_CASES = {
    "layer_single": ("layer", (3, 1), 0.0, 1e-5, True),
    "layer_three": ("layer", (2, 2, 3), 0.0, 1e-5, True),
    "layer_five_plain": ("layer", (4, 5), 0.0, 1e-5, False),
    "layer_64": ("layer", (2, 64), 0.0, 1e-5, True),
    "layer_65_eps": ("layer", (2, 65), 0.0, 1e-2, True),
    "layer_offset_64": ("layer", (2, 64), 1000.0, 1e-5, True),
    "layer_offset_257": ("layer", (1, 257), 1000.0, 1e-5, True),
    "rms_single": ("rms", (3, 1), 0.0, 0.5, True),       # (N = 1: dx = g (1 - xh^2) cancels to eps / (x^2 + eps); eps is not small)
    "rms_five": ("rms", (2, 2, 5), 0.0, 1e-6, True),
    "rms_65_plain": ("rms", (2, 65), 0.0, 1e-6, False),
    "rms_offset_64": ("rms", (2, 64), 1000.0, 1e-6, True),
}
GELU_CASES = {"gelu_exact": "none", "gelu_tanh": "tanh"}
GELU_SPECIALS = np.array([0.0, -0.0, 10.0, -10.0, 40.0, -40.0])


def case_input(name, dtype=np.float32):
    """(x, gamma, beta, dy, kind, eps) of a NORM_CASES entry (beta is None for RMS norm).  The values are float32 numbers
    whatever `dtype` holds them, so one fixture serves both precisions."""
    kind, shape, offset, eps, params = NORM_CASES[name]
    x, gamma, beta, dy = (None if a is None else a.astype(dtype) for a in make_inputs(
        np.random.RandomState(case_seed(name)), shape, np.float32, offset, params=params))
    return x, gamma, (beta if kind == "layer" else None), dy, kind, eps


def case_fields(name):
    """The fields the fixture holds for a case, in FIELDS order, with their shapes: [(field, shape), ...]."""
    kind, shape, _, _, _ = NORM_CASES[name]
    n = shape[-1]
    shapes = dict(y=shape, mean=shape[:-1], rstd=shape[:-1], dx=shape, dgamma=(n,), dbeta=(n,))
    return [(f, shapes[f]) for f in FIELDS if kind == "layer" or f not in ("mean", "dbeta")]


def pack(values, layout):
    """One flat float64 array of the named arrays in `layout` order ([(name, shape), ...]) — how the fixture stores a case."""
    return np.concatenate([np.asarray(values[name], dtype=np.float64).reshape(-1) for name, _ in layout])


def unpack(flat, layout):
    out, off = {}, 0
    for name, shape in layout:
        size = int(np.prod(shape, dtype=np.int64))
        out[name] = np.asarray(flat[off:off + size]).reshape(shape)
        off += size
    assert off == flat.size, "the fixture's array holds %d elements, the layout %d" % (flat.size, off)
    return out


def block_layout():
    shapes = block_shapes(BLOCK_CASE["E"], BLOCK_CASE["hidden"])
    return [(name, shapes[name]) for name in BLOCK_NAMES]


def gelu_input(n, seed, dtype=np.float32):
    """(x, dy) of n elements: the special values first (as many as fit), then 3 * normal; float32 numbers in `dtype`."""
    rs = np.random.RandomState(seed)
    x = (3.0 * rs.randn(n)).astype(np.float32)
    k = min(n, GELU_SPECIALS.size)
    x[:k] = GELU_SPECIALS[:k]
    return x.astype(dtype), rs.randn(n).astype(np.float32).astype(dtype)


# ---------------------------------------------------------------------- float64 TransformerBlock replica
BLOCK_CASE = dict(B=2, T=17, E=32, H=4, hidden=64, causal=True, eps=1e-5, lr=1e-3, steps=3)
BLOCK_NAMES = ("ln1.gamma", "ln1.beta", "attn.wq", "attn.bq", "attn.wk", "attn.bk", "attn.wv", "attn.bv", "attn.wo", "attn.bo",
               "ln2.gamma", "ln2.beta", "fc1.w", "fc1.b", "fc2.w", "fc2.b")


def block_shapes(e, hidden):
    shapes = {"fc1.w": (e, hidden), "fc1.b": (1, hidden), "fc2.w": (hidden, e), "fc2.b": (1, e)}
    for name in BLOCK_NAMES:
        if name not in shapes:
            shapes[name] = (e, e) if name.startswith("attn.w") else (1, e)
    return shapes


def block_data(dtype=np.float32):
    """(x, y) of the fixture's block case, regenerated from a seed (float32 numbers in `dtype`)."""
    c = BLOCK_CASE
    rs = np.random.RandomState(case_seed("transformer_block"))
    return tuple(rs.randn(c["B"], c["T"], c["E"]).astype(np.float32).astype(dtype) for _ in range(2))


def block_initial():
    """Initial parameters of the block case: multiples of 2**-10 (exact in float16, float32 and float64 alike; the fixture
    stores them as float16).  Weights uniform within the Xavier half-width, gamma around 1, biases and beta small."""
    c = BLOCK_CASE
    rs = np.random.RandomState(case_seed("transformer_block_parameters"))
    out = {}
    for name, shape in block_shapes(c["E"], c["hidden"]).items():
        if name.endswith(".gamma"):
            vals = 1.0 + 0.25 * rs.randn(*shape)
        elif shape[0] == 1:
            vals = 0.1 * rs.randn(*shape)
        else:
            vals = rs.uniform(-1.0, 1.0, shape) * math.sqrt(6.0 / (shape[0] + shape[1]))
        out[name] = (np.round(vals * 1024.0) / 1024.0).astype(np.float16)
    return {name: out[name] for name in BLOCK_NAMES}


def block_loss_and_grads(params, x, y, heads, causal, eps, with_bk_terms=False):
    """float64 loss ((out - y) ** 2).sum() / B of the pre-norm block (tanh GELU) and the gradient of every parameter, by the
    analytic formulas of this module.  The gradient of attn.bk is mathematically ZERO (bk shifts all scores of a row alike,
    which the softmax does not see): what an evaluation returns there is the rounding left over from a sum of terms that
    cancel, so its own size says nothing and it is judged against the sum of |terms| behind every element, which
    with_bk_terms=True returns as a third value ([1, E])."""
    p = {k: np.asarray(v, dtype=np.float64) for k, v in params.items()}
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    b, t, e = x.shape
    hd = e // heads
    g = {}
    ln1 = reference(x, p["ln1.gamma"], p["ln1.beta"], None, "layer", eps).values["y"]
    rows = ln1.reshape(b * t, e)
    q, k, v = ((rows @ p["attn.w" + n] + p["attn.b" + n]).reshape(b, t, heads, hd).transpose(0, 2, 1, 3) for n in "qkv")
    s = q @ k.transpose(0, 1, 3, 2) / math.sqrt(hd)
    if causal:
        s = np.where(np.arange(t)[None, :] <= np.arange(t)[:, None], s, -np.inf)
    pr = np.exp(s - s.max(axis=-1, keepdims=True))
    pr /= pr.sum(axis=-1, keepdims=True)
    att = (pr @ v).transpose(0, 2, 1, 3).reshape(b * t, e)
    h = x + (att @ p["attn.wo"] + p["attn.bo"]).reshape(b, t, e)
    ln2 = reference(h, p["ln2.gamma"], p["ln2.beta"], None, "layer", eps).values["y"].reshape(b * t, e)
    z = ln2 @ p["fc1.w"] + p["fc1.b"]
    act = gelu64(z, "tanh")
    out = h + (act @ p["fc2.w"] + p["fc2.b"]).reshape(b, t, e)
    err = out - y
    loss = (err ** 2).sum() / b
    dout = 2.0 * err / b
    d2 = dout.reshape(b * t, e)
    g["fc2.w"], g["fc2.b"] = act.T @ d2, d2.sum(0, keepdims=True)
    dz = gelu_reference(z, d2 @ p["fc2.w"].T, "tanh").values["dx"]
    g["fc1.w"], g["fc1.b"] = ln2.T @ dz, dz.sum(0, keepdims=True)
    r2 = reference(h, p["ln2.gamma"], p["ln2.beta"], (dz @ p["fc1.w"].T).reshape(b, t, e), "layer", eps).values
    g["ln2.gamma"], g["ln2.beta"] = r2["dgamma"].reshape(1, e), r2["dbeta"].reshape(1, e)
    dh = dout + r2["dx"]
    dh2 = dh.reshape(b * t, e)
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
    r1 = reference(x, p["ln1.gamma"], p["ln1.beta"], drows.reshape(b, t, e), "layer", eps).values
    g["ln1.gamma"], g["ln1.beta"] = r1["dgamma"].reshape(1, e), r1["dbeta"].reshape(1, e)
    grads = {name: g[name] for name in BLOCK_NAMES}
    return (loss, grads, bk_terms) if with_bk_terms else (loss, grads)


def block_adam_losses(params, x, y, heads, causal, eps, lr, steps, beta1=0.9, beta2=0.999, adam_eps=1e-8):
    """The losses of `steps` Adam steps (core/optimizer.py: epsilon outside the square root, after bias correction)."""
    p = {k: np.array(v, dtype=np.float64) for k, v in params.items()}
    m = {k: np.zeros_like(v) for k, v in p.items()}
    v2 = {k: np.zeros_like(v) for k, v in p.items()}
    losses = []
    for step in range(1, steps + 1):
        loss, grads = block_loss_and_grads(p, x, y, heads, causal, eps)
        losses.append(loss)
        for k in p:
            m[k] += (1.0 - beta1) * (grads[k] - m[k])
            v2[k] += (1.0 - beta2) * (grads[k] ** 2 - v2[k])
            p[k] -= lr * (m[k] / (1 - beta1 ** step)) / ((v2[k] / (1 - beta2 ** step)) ** 0.5 + adam_eps)
    return np.array(losses)
