"""TEST INFRASTRUCTURE — the yardstick of the rotary position embedding: numpy only (long double), independent of
tinynn_autograd_amd.rope.rope_host.

Two accuracy statements, kept apart:

  tables    tinynn_autograd_amd.rope.tables against 50-digit values (tests/gen_rope_golden.py evaluates the spots with mpmath
            and stores them as double-double pairs): |table - exact| <= u + 4 eps_longdouble p theta_i, with u the dtype's
            unit roundoff (the final rounding of a value of magnitude <= 1) and theta_i = base^(-2 i / R); the second term
            allows a few long-double roundings of the angle p theta_i, whose error passes into cos and sin with slope <= 1.
            A float64 angle would be off by ~ p theta_i 2^-53 = 4.5e-13 at p = 4095, thirty times the float64 bound there.

  kernel    relative to the ROUNDED tables it was given.  The oracle takes the same rounded tables and evaluates
            y_lo = x_lo c - x_hi s, y_hi = x_hi c + x_lo s in long double (relative error <= 2^-62 of the sum of the
            magnitudes of the two terms: two products and a sum at 2^-64 each, rounded up).  The device's fixed expression
            is one rounded product and one fma: y = fl(a - fl(b)) with a = x_lo c exact inside the fma and b = x_hi s, so
                |y - (a - b)| <= u |b| + u (|a| + |b| (1 + u)) <= gamma_2 (|a| + |b|),   gamma_2 = 2 u / (1 - 2 u).
            The composed route's three roundings, fl(fl(a) - fl(b)), meet the same bound: u |a| + u |b| + u (|a| + |b|)(1 + u)
            <= gamma_2 (|a| + |b|) (1 + u), which the oracle term covers.  So
                bound = (gamma_2 + 2^-62) (|x_lo c| + |x_hi s|)      (y_hi: |x_hi c| + |x_lo s|)
            and the elements [R, D) and the zero rows of an out-of-range position are exact (bound 0).  A rotated vjp is the
            same statement with s -> -s.  tests/gen_rope_golden.py checks for every case that the bound is below 1e-3 of the
            median output magnitude — a wrong sign, a swapped pair or a wrong table row misses it by orders of magnitude.
"""

import numpy as np

import gqa_oracle as go
import norm_oracle as no

LD = np.longdouble
ORACLE_REL = 2.0 ** -62
P = 4096                  # the table length of the cases
BASE = 10000.0
PAIRINGS = ("half", "interleaved")
LAYOUTS = ("bthd", "bhtd")
case_seed = go.case_seed


def unit(dtype):
    """The unit roundoff of `dtype`."""
    return 2.0 ** -24 if np.dtype(dtype) == np.float32 else 2.0 ** -53


def gamma2(dtype):
    u = unit(dtype)
    return 2 * u / (1 - 2 * u)


def pair_slices(pairing, R):
    return (slice(0, R // 2), slice(R // 2, R)) if pairing == "half" else (slice(0, R, 2), slice(1, R, 2))


class Result(object):
    """values: long double, in the operand's layout; bounds: elementwise, float64."""

    def __init__(self, values, bounds):
        self.values, self.bounds = values, bounds


def reference(x, cos_t, sin_t, offset=0, positions=None, layout="bthd", pairing="half", inverse=False, dtype=np.float32):
    """The rotation of x (values of `dtype`) with the ROUNDED tables cos_t / sin_t [P, R / 2] (values of `dtype`), in long
    double, and the bound for an evaluation in `dtype`.  positions: host integers [B] (T == 1) or None (offset + t)."""
    x = np.asarray(x)
    xv = (x if layout == "bthd" else x.transpose(0, 2, 1, 3)).astype(LD)            # [B, T, H, D]
    ct, st = np.asarray(cos_t).astype(LD), np.asarray(sin_t).astype(LD)
    rows, half = ct.shape
    R = 2 * half
    B, T = xv.shape[:2]
    if positions is None:
        pos = np.broadcast_to(int(offset) + np.arange(T), (B, T))
    else:
        pos = np.asarray(positions, dtype=np.int64).reshape(B, 1)
    valid = (pos >= 0) & (pos < rows)
    safe = np.where(valid, pos, 0)
    c, s = ct[safe][:, :, None, :], st[safe][:, :, None, :]
    if inverse:
        s = -s
    lo, hi = pair_slices(pairing, R)
    values, bounds = xv.copy(), np.zeros(xv.shape)
    x_lo, x_hi = xv[..., lo], xv[..., hi]
    values[..., lo] = x_lo * c - x_hi * s
    values[..., hi] = x_hi * c + x_lo * s
    rel = gamma2(dtype) + ORACLE_REL
    bounds[..., lo] = (rel * (np.abs(x_lo * c) + np.abs(x_hi * s))).astype(np.float64)
    bounds[..., hi] = (rel * (np.abs(x_hi * c) + np.abs(x_lo * s))).astype(np.float64)
    values[~valid] = 0
    bounds[~valid] = 0
    if layout == "bhtd":
        values, bounds = values.transpose(0, 2, 1, 3), bounds.transpose(0, 2, 1, 3)
    return Result(np.ascontiguousarray(values), np.ascontiguousarray(bounds))


def propagate(bound, cos_t, sin_t, offset=0, layout="bthd", pairing="half"):
    """An elementwise error bound on the INPUT of a rotation -> the bound it causes on the output:
    |c| b_lo + |s| b_hi and |c| b_hi + |s| b_lo (float64, widened by 2^-50 for its own roundings)."""
    bound = np.asarray(bound, dtype=np.float64)
    bv = bound if layout == "bthd" else bound.transpose(0, 2, 1, 3)
    half = np.shape(cos_t)[1]
    T = bv.shape[1]
    c = np.abs(np.asarray(cos_t, dtype=np.float64))[offset:offset + T][None, :, None, :]
    s = np.abs(np.asarray(sin_t, dtype=np.float64))[offset:offset + T][None, :, None, :]
    lo, hi = pair_slices(pairing, 2 * half)
    out = bv.copy()
    out[..., lo] = (c * bv[..., lo] + s * bv[..., hi]) * (1 + 2.0 ** -50)
    out[..., hi] = (c * bv[..., hi] + s * bv[..., lo]) * (1 + 2.0 ** -50)
    return out if layout == "bthd" else np.ascontiguousarray(out.transpose(0, 2, 1, 3))


def roundtrip(x, y_got, back_got, cos_t, sin_t, offset, layout, pairing, dtype, what):
    """inverse(forward(x)) against x, for evaluations y_got = forward(x) and back_got = inverse(y_got) in `dtype`:
        back_got = inv(y_got) + e2,          |e2| <= bound of the inverse call on y_got        (one kernel bound)
        inv(y_got) = inv(y) + inv(e1),       |inv(e1)| <= propagate(bound of the forward call)  (the other one, rotated)
        inv(y) = x (c^2 + s^2),              |c^2 + s^2 - 1| <= 2 u + 2 u^2 for entries rounded to `dtype`
    so |back_got - x| <= bound_inv + propagate(bound_fwd) + (2 u + 2 u^2) |x|: twice the kernel bound and the tables' own term."""
    fwd = reference(x, cos_t, sin_t, offset, None, layout, pairing, False, dtype)
    assert_within(y_got, fwd, what + " forward")
    inv = reference(y_got, cos_t, sin_t, offset, None, layout, pairing, True, dtype)
    assert_within(back_got, inv, what + " inverse")
    u = unit(dtype)
    total = inv.bounds + propagate(fwd.bounds, cos_t, sin_t, offset, layout, pairing) + (2 * u + 2 * u * u) * np.abs(x)
    err = np.abs(np.asarray(back_got).astype(LD) - np.asarray(x).astype(LD)).astype(np.float64)
    assert (err <= total).all(), "%s round trip: %.3e beyond the bound" % (what, float((err - total).max()))


def assert_within(got, res, what, factor=1.0, verbose=False):
    """|got - values| <= factor * bounds elementwise (an element with bound 0 must be exact)."""
    got = np.asarray(got)
    assert got.shape == res.values.shape, "%s: shape %s vs %s" % (what, got.shape, res.values.shape)
    if not got.size:
        return
    err = np.abs(got.astype(LD) - res.values).astype(np.float64)
    bound = factor * res.bounds
    if verbose:
        ratio = float((err / np.maximum(bound, np.finfo(np.float64).tiny))[bound > 0].max()) if (bound > 0).any() else 0.0
        print("%s: max error %.3e, max bound %.3e, worst error / bound %.3f" % (what, err.max(), bound.max(), ratio))
    worst = float((err - bound).max())
    assert worst <= 0.0, "%s: error exceeds the derived bound by %.3e (max error %.3e, max bound %.3e)" % (
        what, worst, float(err.max()), float(bound.max()))


# ---------------------------------------------------------------------- cases
# name -> (B, T, Ha, Hb, D, R); Hb == 0: a single tensor
CASES = {
    "one_pair": (1, 1, 1, 0, 2, 2),
    "odd_d_partial": (2, 5, 3, 1, 3, 2),
    "one_f32_vector": (1, 5, 2, 2, 8, 8),
    "aligned_tail": (3, 1, 4, 2, 16, 8),
    "half_six": (1, 65, 4, 1, 24, 12),
    "d64": (2, 3, 8, 1, 64, 64),
    "d128": (1, 2, 2, 2, 128, 128),
    "d130": (1, 2, 1, 1, 130, 128),
}
GOLDEN_OFFSET = 7         # the offset of the fixture's results


def case_input(name, dtype=np.float32, layout="bthd"):
    """(xa, xb or None) of a case in `layout`, amplitudes 1 and 3."""
    B, T, Ha, Hb, D, R = CASES[name]
    rs = np.random.RandomState(case_seed("rope." + name))
    xa = rs.randn(B, T, Ha, D).astype(dtype)
    xb = (rs.randn(B, T, Hb, D) * 3).astype(dtype) if Hb else None
    if layout == "bhtd":
        xa = np.ascontiguousarray(xa.transpose(0, 2, 1, 3))
        xb = None if xb is None else np.ascontiguousarray(xb.transpose(0, 2, 1, 3))
    return xa, xb


def dd_split(value):
    """A 50-digit mpmath number as a double-double pair (hi, lo)."""
    hi = float(value)
    return hi, float(value - hi)


def dd_join(hi, lo):
    return np.asarray(hi).astype(LD) + np.asarray(lo).astype(LD)


# (p, i) spots of the table test for P = 4096, R = 128: the first and last positions and frequencies among them
TABLE_R = 128
TABLE_SPOTS = [(p, i) for p in (0, 1, 7, 100, 1000, 2048, 4095) for i in (0, 1, 31, 62, 63)]


def table_bound(p, i, R, dtype, base=BASE):
    theta = float(base) ** (-2.0 * i / R)
    return unit(dtype) + 4 * float(np.finfo(LD).eps) * p * theta


# ---------------------------------------------------------------------- a two-block grouped-query language model with rotary
# positions, greedy: gqa_oracle's model (its shapes, parameters and prompt) WITHOUT the learned position table, q and k of
# every block rotated at the positions 0 .. T - 1 (full rotary width E / H, pairing "half").
LM = dict(go.LM)
LM_MARGIN = go.LM_MARGIN


def lm_tables():
    from tinynn_autograd_amd import rope as rp
    c = LM
    return rp.tables(c["max_len"], c["E"] // c["H"], BASE, np.float64)


def lm_params(seed, head_scale):
    p = go.lm_params(seed, head_scale)
    del p["emb.pos"]
    return p


lm_prompt = go.lm_prompt


def _block(p, x, heads, kv_heads, eps, cos_t, sin_t):
    b, t, e = x.shape
    hd = e // heads
    ln1 = no.reference(x, p["ln1.gamma"], p["ln1.beta"], None, "layer", eps).values["y"]
    rows = ln1.reshape(b * t, e)
    q, k, v = ((rows @ p["attn.w" + n] + p["attn.b" + n]).reshape(b, t, heads if n == "q" else kv_heads, hd) for n in "qkv")
    q, k = (reference(a, cos_t, sin_t, dtype=np.float64).values.astype(np.float64) for a in (q, k))
    k, v = (np.repeat(a, heads // kv_heads, axis=2) for a in (k, v))
    q, k, v = (a.transpose(0, 2, 1, 3) for a in (q, k, v))
    s = q @ k.transpose(0, 1, 3, 2) / np.sqrt(hd)
    s = np.where(np.arange(t)[None, :] <= np.arange(t)[:, None], s, -np.inf)
    pr = np.exp(s - s.max(axis=-1, keepdims=True))
    pr /= pr.sum(axis=-1, keepdims=True)
    att = (pr @ v).transpose(0, 2, 1, 3).reshape(b * t, e)
    h = x + (att @ p["attn.wo"] + p["attn.bo"]).reshape(b, t, e)
    ln2 = no.reference(h, p["ln2.gamma"], p["ln2.beta"], None, "layer", eps).values["y"].reshape(b * t, e)
    act = no.gelu64(ln2 @ p["fc1.w"] + p["fc1.b"], "tanh")
    return h + (act @ p["fc2.w"] + p["fc2.b"]).reshape(b, t, e)


def lm_logits(p, ids):
    """float64 logits [B, T, V] of the model for ids [B, T]."""
    c = LM
    b, t = ids.shape
    cos_t, sin_t = lm_tables()
    h = p["emb.tok"][ids]
    for i in range(c["blocks"]):
        blk = {n.split(".", 1)[1]: a for n, a in p.items() if n.startswith("block%d." % i)}
        h = _block(blk, h, c["H"], c["Hkv"], c["eps"], cos_t, sin_t)
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
