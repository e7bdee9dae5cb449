"""TEST INFRASTRUCTURE — the float64 yardstick of scaled-dot-product attention (the reference has none): numpy only, the
plain softmax(scale q k^T) v with its analytic gradients, the DERIVED first-order error bounds of the tests, and a float64
replica of one MultiHeadAttention training step (squared-error loss of core/losses.py, Adam of oracle/closed_form.py).

Bounds.  u = 2**-24 (float32) or 2 * 2**-53 (float64); X = 2, the exp gate of tests/kernel_sweep.ULP_GATES; |.| elementwise;
sums over kept keys only.

    E_i      = (D + 3) u scale max_j sum_d |q_id| |k_jd|        score error of a length-D dot product plus the scaling
    rho_i    = 2 E_i + (Tk + X + 4) u                           relative error of p_ij
    |o - o64|     <= (rho_i + (Tk + 2) u) (p |v|)_ic
    |lse - lse64| <= E_i + (Tk + X + 4) u + u |lse64|
    |dv - dv64|   <= sum_i (rho_i + (Tq + 2) u) p_ij |do_ic|
    F_ij     = (Dv + 2) u sum_c |do_ic| |v_jc|
    b_delta  = (Dv + 2) u sum_c |do| |o64| + sum_c |do| bound_o
    b_dS     = rho_i |dS64| + p (F + b_delta) + 2 u p (|dP64| + |delta64|)
    |dq - dq64|   <= scale [ (Tk + 3) u (|dS64| |k|) + b_dS |k| ]
    |dk - dk64|   <= scale [ (Tq + 3) u (|dS64|^T |q|) + b_dS^T |q| ]

The bounds are worst-case and loose; so that one cannot hide a defect, assert_within also demands that the MEDIAN of
bound / (|ref| + tiny) over the elements is below MEDIAN_GATE — a condition on the inputs (q amplitude <= 4, k 1, v 3, do 1
meet it), not a measurement.  A reference that is exactly zero everywhere (one key: dq = dk = 0) is exempt: the result must
then lie within the bound of zero."""

import numpy as np

U32, U64 = 2.0 ** -24, 2.0 ** -53
EXP_ULP = 2.0                 # tests/kernel_sweep.ULP_GATES["exp"]
MEDIAN_GATE = 0.05
FIELDS = ("o", "lse", "dq", "dk", "dv")


def unit(dtype):
    return U32 if np.dtype(dtype) == np.float32 else 2.0 * U64


def default_scale(q, layout="bhtd"):
    return 1.0 / np.sqrt(q.shape[-1])


def to3(x, layout):
    """[B H, T, W] float64 view of an operand of either layout."""
    x = np.asarray(x, dtype=np.float64)
    if layout == "bthd":
        x = x.transpose(0, 2, 1, 3)
    return x.reshape((-1,) + x.shape[-2:])


def from3(x3, layout, like_shape):
    """Back to the layout of an operand whose shape (up to the last axis extent) is like_shape."""
    if layout == "bthd":
        b, t, h, _ = like_shape
        return x3.reshape(b, h, t, x3.shape[-1]).transpose(0, 2, 1, 3)
    return x3.reshape(tuple(like_shape[:-1]) + (x3.shape[-1],))


def keep_mask(tq, tk, causal):
    """[Tq, Tk] booleans: key j is kept for query i iff not causal or j <= i (top-left aligned)."""
    if not causal:
        return np.ones((tq, tk), dtype=bool)
    return np.arange(tk)[None, :] <= np.arange(tq)[:, None]


def lse_shape(q_shape, layout):
    if layout == "bthd":
        return (q_shape[0], q_shape[2], q_shape[1])
    return tuple(q_shape[:-1])


class Result(object):
    """values: o, lse, dq, dk, dv (float64, in the operands' layout); bounds: the same names -> elementwise bounds."""

    def __init__(self):
        self.values, self.bounds = {}, {}


def reference(q, k, v, do=None, causal=False, scale=None, layout="bhtd", dtype=np.float32):
    """Forward, gradients for `do` (None: forward only) and the bounds for an evaluation in `dtype`."""
    scale = float(default_scale(q) if scale is None else scale)
    q3, k3, v3 = to3(q, layout), to3(k, layout), to3(v, layout)
    tq, d = q3.shape[1:]
    tk, dv_ = v3.shape[1:]
    keep = keep_mask(tq, tk, causal)[None]
    s = np.where(keep, scale * np.einsum("bid,bjd->bij", q3, k3), -np.inf)
    m = s.max(axis=-1, keepdims=True)
    e = np.exp(s - m)
    l = e.sum(axis=-1, keepdims=True)
    p = e / l
    o3 = p @ v3
    lse3 = (m + np.log(l))[..., 0]
    u = unit(dtype)
    absqk = np.where(keep, np.einsum("bid,bjd->bij", np.abs(q3), np.abs(k3)), 0.0)
    E = (d + 3) * u * abs(scale) * absqk.max(axis=-1, keepdims=True)                  # [b, i, 1]
    rho = 2 * E + (tk + EXP_ULP + 4) * u
    b_o = (rho + (tk + 2) * u) * (p @ np.abs(v3))
    b_lse = E[..., 0] + (tk + EXP_ULP + 4) * u + u * np.abs(lse3)
    res = Result()
    ls = lse_shape(np.shape(q), layout)
    res.values["o"], res.bounds["o"] = from3(o3, layout, np.shape(q)), from3(b_o, layout, np.shape(q))
    res.values["lse"], res.bounds["lse"] = lse3.reshape(ls), b_lse.reshape(ls)
    if do is None:
        return res
    g3 = to3(do, layout)
    dP = np.einsum("bic,bjc->bij", g3, v3)
    delta = (g3 * o3).sum(axis=-1, keepdims=True)
    dS = p * (dP - delta)
    dS[np.broadcast_to(keep.sum(axis=-1, keepdims=True) == 1, dS.shape)] = 0.0     # one kept key: p = 1, dP = delta exactly
    dq3 = scale * (dS @ k3)
    dk3 = scale * np.einsum("bij,bid->bjd", dS, q3)
    dv3 = np.einsum("bij,bic->bjc", p, g3)
    ag = np.abs(g3)
    b_dv = np.einsum("bij,bic->bjc", p, (rho + (tq + 2) * u) * ag)
    F = (dv_ + 2) * u * np.einsum("bic,bjc->bij", ag, np.abs(v3))
    b_delta = (dv_ + 2) * u * (ag * np.abs(o3)).sum(axis=-1, keepdims=True) + (ag * b_o).sum(axis=-1, keepdims=True)
    b_dS = rho * np.abs(dS) + p * (F + b_delta) + 2 * u * p * (np.abs(dP) + np.abs(delta))
    b_dq = abs(scale) * ((tk + 3) * u * (np.abs(dS) @ np.abs(k3)) + b_dS @ np.abs(k3))
    b_dk = abs(scale) * ((tq + 3) * u * np.einsum("bij,bid->bjd", np.abs(dS), np.abs(q3))
                         + np.einsum("bij,bid->bjd", b_dS, np.abs(q3)))
    res.values["delta"] = delta[..., 0].reshape(ls)
    for name, val, bnd, like in (("dq", dq3, b_dq, q), ("dk", dk3, b_dk, k), ("dv", dv3, b_dv, v)):
        res.values[name], res.bounds[name] = from3(val, layout, np.shape(like)), from3(bnd, layout, np.shape(like))
    return res


def assert_within(got, want, bound, what, factor=1.0, verbose=False):
    """|got - want| <= factor * bound elementwise, and the bound is tight enough to mean something (module docstring)."""
    got = np.asarray(got, dtype=np.float64)
    want, bound = np.asarray(want, dtype=np.float64), factor * np.asarray(bound, dtype=np.float64)
    assert got.shape == want.shape, "%s: shape %s vs %s" % (what, got.shape, want.shape)
    if not got.size:
        return
    err = np.abs(got - want)
    ratio = float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max()) if (bound > 0).any() else 0.0
    if verbose:
        print("%s: max error %.3e, max bound %.3e, worst error / bound %.3f" % (what, err.max(), bound.max(), ratio))
    worst = float((err - bound).max())
    assert worst <= 0.0, "%s: error exceeds the derived bound by %.3e (max error %.3e, max bound %.3e)" % (
        what, worst, float(err.max()), float(bound.max()))
    if (want == 0).all():
        return                                    # e.g. one key: dq = dk = 0 exactly; the result lies within the bound of 0
    tiny = np.finfo(np.float64).tiny
    med = float(np.median(bound / factor / (np.abs(want) + tiny)))
    assert med < MEDIAN_GATE, "%s: the bound is too loose to test anything (median bound / |ref| = %.3g)" % (what, med)


def check(got, res, what, fields=FIELDS, factor=1.0, verbose=False):
    """got: {name: array}; every named field against the oracle."""
    for name in fields:
        if name in got and got[name] is not None:
            assert_within(got[name], res.values[name], res.bounds[name], "%s %s" % (what, name), factor, verbose)


# ---------------------------------------------------------------------- inputs
def case_seed(name):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % (2 ** 31)


def shapes(layout, b, h, tq, tk, d, dv):
    if layout == "bthd":
        return (b, tq, h, d), (b, tk, h, d), (b, tk, h, dv), (b, tq, h, dv)
    return (b, h, tq, d), (b, h, tk, d), (b, h, tk, dv), (b, h, tq, dv)


def make_inputs(rs, layout, b, h, tq, tk, d, dv, dtype=np.float32, q_amp=4.0):
    """(q, k, v, do) with the amplitudes the median gate is stated for: q <= 4, k 1, v 3, do 1."""
    qs, ks, vs, os_ = shapes(layout, b, h, tq, tk, d, dv)
    return ((rs.randn(*qs) * q_amp).astype(dtype), rs.randn(*ks).astype(dtype), (rs.randn(*vs) * 3).astype(dtype),
            rs.randn(*os_).astype(dtype))


# name -> (layout, B, H, Tq, Tk, D, Dv, causal, scale (None: 1 / sqrt(D)))       the fixture's cases (tests/gen_attn_golden.py)
ATTN_CASES = {
    "single_element": ("bhtd", 1, 1, 1, 1, 1, 1, False, None),
    "one_key": ("bhtd", 2, 1, 5, 1, 3, 4, False, None),
    "square_small": ("bhtd", 2, 2, 7, 7, 5, 3, False, None),
    "causal_square": ("bhtd", 1, 3, 17, 17, 8, 8, True, None),
    "causal_more_queries": ("bhtd", 2, 1, 20, 9, 4, 6, True, 0.7),
    "causal_more_keys": ("bthd", 2, 2, 9, 20, 6, 4, True, None),
    "bthd_heads": ("bthd", 2, 3, 11, 13, 16, 16, False, None),
    "past_one_block": ("bthd", 1, 2, 65, 70, 5, 9, True, None),
    "wide_heads": ("bhtd", 1, 1, 9, 20, 128, 65, False, 0.05),
}


def case_input(name, dtype=np.float32):
    layout, b, h, tq, tk, d, dv, causal, scale = ATTN_CASES[name]
    rs = np.random.RandomState(case_seed(name))
    return make_inputs(rs, layout, b, h, tq, tk, d, dv, dtype, q_amp=2.0) + (causal, scale, layout)


# ---------------------------------------------------------------------- float64 MultiHeadAttention replica
class MHA64(object):
    """Self-attention over [B, T, E] with H heads: rows @ wq + bq etc., softmax(q k^T / sqrt(E / H)) v per head (optionally
    causal), an output projection, the squared-error loss ((out - y) ** 2).sum() / B and Adam.  Parameters in the layer's
    order: wq bq wk bk wv bv wo bo."""

    def __init__(self, params, heads, causal=False, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8):
        self.p = [np.array(a, dtype=np.float64) for a in params]
        self.heads, self.causal = heads, causal
        n = sum(a.size for a in self.p)
        self.m, self.v, self.t = np.zeros(n), np.zeros(n), 0
        self.lr, self.b1, self.b2, self.eps = lr, beta1, beta2, eps

    def loss_and_grads(self, x, y):
        wq, bq, wk, bk, wv, bv, wo, bo = self.p
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        b, t, e = x.shape
        h = self.heads
        rows = x.reshape(b * t, e)
        q, k, v = ((rows @ w + c).reshape(b, t, h, e // h) for w, c in ((wq, bq), (wk, bk), (wv, bv)))
        fwd = reference(q, k, v, None, self.causal, None, "bthd")
        att = fwd.values["o"].reshape(b * t, e)
        out = (att @ wo + bo).reshape(b, t, e)
        err = out - y
        loss = (err ** 2).sum() / b
        dout = (2.0 * err / b).reshape(b * t, e)
        g, scales = [None] * 8, [None] * 8
        g[6], g[7] = att.T @ dout, dout.sum(0, keepdims=True)
        scales[6], scales[7] = np.abs(att).T @ np.abs(dout), np.abs(dout).sum(0, keepdims=True)
        datt = (dout @ wo.T).reshape(b, t, h, e // h)
        bwd = reference(q, k, v, datt, self.causal, None, "bthd")
        for at, name in ((0, "dq"), (2, "dk"), (4, "dv")):
            dz = bwd.values[name].reshape(b * t, e)
            g[at], g[at + 1] = rows.T @ dz, dz.sum(0, keepdims=True)
            scales[at], scales[at + 1] = np.abs(rows).T @ np.abs(dz), np.abs(dz).sum(0, keepdims=True)
        # the sums of |terms| behind every gradient element: the scale an error of that element is judged against (the
        # gradient of bk is mathematically zero — a shift of all scores of a row — so its own size says nothing)
        self.grad_scales = scales
        return loss, out, g

    def step(self, x, y):
        loss, _, grads = self.loss_and_grads(x, y)
        flat = np.concatenate([np.ravel(g) for g in grads])
        self.t += 1
        self.m = self.m + (1.0 - self.b1) * (flat - self.m)
        self.v = self.v + (1.0 - self.b2) * (flat ** 2 - self.v)
        upd = -self.lr * (self.m / (1 - self.b1 ** self.t)) / ((self.v / (1 - self.b2 ** self.t)) ** 0.5 + self.eps)
        off = 0
        for a in self.p:
            a += upd[off:off + a.size].reshape(a.shape)
            off += a.size
        return loss, grads
