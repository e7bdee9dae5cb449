"""TEST INFRASTRUCTURE — the float64 yardstick of one decoding step (the reference has none): numpy only.  Decode attention
over a key / value cache with elementwise DERIVED bounds (attn_oracle.reference on Tq = 1 plus the term of the key split),
the sampling rule with the float64 interval [lo, hi) of every kept token on the normalised CDF and a DERIVED bound on the CDF
error of an evaluation in the operand dtype, and a one-block language model (token_oracle's) generated greedily.

Decode attention.  attn_oracle bounds a two-pass softmax: |o - o64| <= (rho + (Tk + 2) u) (p |v|), rho = 2 E + (Tk + X + 4) u,
with the summation terms (Tk u) good for ANY order of the additions.  The kernel is an online softmax cut over lane groups,
waves and splits: every partial (l, acc) is multiplied by f = exp(m_old - m_new) each time its maximum moves.  In exact
arithmetic the factors telescope to exp(s_j - m_final); in the operand dtype each one carries a relative error of at most
2 X u (the exp: X ulps of 2 u) + u |m_old - m_new| (the rounding of its argument, |m_old - m_new| <= 2 S with S = |scale| max_j sum_d |q_d| |k_jd|
>= every |score|) + u (the product).  A contribution meets at most

    R = ceil(run / (UNROLL * 4)) + 6 + 1 + 1        run = the keys of the longest split's run of chunks

of them: the steps of its workgroup's loop (a step takes UNROLL keys per lane group and a workgroup holds at least 4 groups),
the exchange tree over at most 64 groups of a wave (6 levels), the waves' meeting and the splits' combine.  Numerator and
denominator each carry them, so

    |o - o64| <= (rho + (Tk + 2) u + 2 R ((2 X + 1) u + 2 u S)) (p |v|)

The composed route (a two-pass softmax) lies within the plain bound, hence within this one.

Sampling.  z = x / temperature is formed in the OPERAND dtype (-0 counted as +0) — it DEFINES the ties, so the oracle starts
from those z.  t_v = z_v - max z <= 0, w_v = exp(t_v), W = sum over the kept set, F(v) = (sum of w_j, kept j <= v) / W; token v
owns [lo, hi) = [F(v) - w_v / W, F(v)) and is chosen for u in it.  In the dtype, with n kept columns:

    fl(t_v) = t_v (1 + d), |d| <= u           -> the argument of exp is off by at most u |t_v|
    w^_v = w_v (1 + th_v), |th_v| <= (|t_v| + 2 X) u                 (X = 2: the gate of the device exp, in ulps of 2 u)
    a running sum of at most n non-negative terms, ANY order:  relative error <= n u       (likewise W, + 2 u for the ties' product)
    the comparison  P^(v) > fl(u W^)  is  P^(v) / W^ (1 + d') > u

    |P^(v) / W^ - F(v)| <= 2 u sum_kept p_j (|t_j| + 2 X) + (2 n + 3) u  =: cdf_bound     (p_j = w_j / W, F <= 1)

A u that lies more than the bound from both ends of its token's interval therefore gives that token; the tests demand
4 x (MARGIN) because summation orders differ.  Two ends are EXACT and exempt: lo == 0 (the running sum before the first
column of positive weight is a sum of exact zeros, and u W >= 0) and hi == 1 of the LAST column of positive weight (no
later column can be chosen: either its running sum exceeds u W or the rule's fallback — the largest kept v with w_v > 0 —
picks it).  -inf logits weigh exactly 0 in every precision."""

import math

import numpy as np

import attn_oracle as ao
import norm_oracle as no
import token_oracle as to

EXP_ULP = ao.EXP_ULP
MARGIN = 4.0
CHUNK, UNROLL, MAX_SPLITS = 64, 4, 256          # include/tnn_decode.h (tests/test_decode_abi.py ties them to the header)
unit, case_seed, pack, unpack = ao.unit, ao.case_seed, no.pack, no.unpack


# ---------------------------------------------------------------------- decode attention
def cache_shape(layout, b, h, tmax, w):
    return (b, tmax, h, w) if layout == "bthd" else (b, h, tmax, w)


def live_rows(cache, layout, n):
    return cache[:, :n] if layout == "bthd" else cache[:, :, :n]


def put_row(cache, layout, row, new):
    """cache with row `row` of every (b, h) replaced by new [B, H, W] (a copy)."""
    out = np.array(cache)
    if layout == "bthd":
        out[:, row] = new
    else:
        out[:, :, row] = new
    return out


def rescales(keys, splits):
    chunks = -(-keys // CHUNK)
    run = max((s + 1) * chunks // splits - s * chunks // splits for s in range(splits)) * CHUNK
    return -(-run // (UNROLL * 4)) + 6 + 1 + 1


def decode_reference(q, k_cache, v_cache, length, k_new=None, v_new=None, scale=None, layout="bthd", dtype=np.float32, splits=1):
    """Result: values["o"] [B, H, Dv] float64, bounds["o"], and the caches after the append (values["k_cache"], ["v_cache"])."""
    append = k_new is not None
    if append:
        k_cache, v_cache = put_row(k_cache, layout, length, k_new), put_row(v_cache, layout, length, v_new)
    n = length + (1 if append else 0)
    b, h, d = q.shape
    q4 = np.asarray(q).reshape((b, 1, h, d) if layout == "bthd" else (b, h, 1, d))
    k, v = live_rows(k_cache, layout, n), live_rows(v_cache, layout, n)
    res = ao.reference(q4, k, v, None, False, scale, layout, dtype)
    scale = float(ao.default_scale(q4) if scale is None else scale)
    q3, k3, v3 = ao.to3(q4, layout), ao.to3(k, layout), ao.to3(v, layout)
    S = abs(scale) * np.einsum("bid,bjd->bij", np.abs(q3), np.abs(k3)).max(axis=-1, keepdims=True)        # [BH, 1, 1]
    s = scale * np.einsum("bid,bjd->bij", q3, k3)
    p = np.exp(s - s.max(axis=-1, keepdims=True))
    p /= p.sum(axis=-1, keepdims=True)
    u = unit(dtype)
    extra = 2 * rescales(n, splits) * ((2 * EXP_ULP + 1) * u + 2 * u * S) * (p @ np.abs(v3))           # [BH, 1, Dv]
    out = ao.Result()
    dv = v3.shape[-1]
    out.values["o"] = np.asarray(res.values["o"]).reshape(b, h, dv)       # (Tq = 1 in either layout)
    bound = np.asarray(res.bounds["o"]).reshape(b, h, dv)
    out.bounds["o"] = bound + extra.reshape(b, h, dv)
    out.values["k_cache"], out.values["v_cache"] = np.asarray(k_cache), np.asarray(v_cache)
    return out


# name -> (layout, B, H, Tmax, length, D, Dv, append, splits)       the fixture's cases (tests/gen_decode_golden.py)
DECODE_CASES = {
    "append_bthd": ("bthd", 2, 3, 96, 70, 16, 24, True, 2),
    "append_bhtd": ("bhtd", 1, 3, 140, 129, 17, 5, True, 3),
    "first_token": ("bthd", 1, 1, 8, 0, 4, 3, True, 1),
    "no_append": ("bhtd", 3, 1, 64, 64, 64, 65, False, 1),
}


def decode_inputs(rs, layout, b, h, tmax, d, dv, dtype=np.float32, q_amp=4.0):
    """(q, k_cache, v_cache, k_new, v_new) with attn_oracle's amplitudes: q <= 4, k 1, v 3."""
    return ((rs.randn(b, h, d) * q_amp).astype(dtype), rs.randn(*cache_shape(layout, b, h, tmax, d)).astype(dtype),
            (rs.randn(*cache_shape(layout, b, h, tmax, dv)) * 3).astype(dtype), rs.randn(b, h, d).astype(dtype),
            (rs.randn(b, h, dv) * 3).astype(dtype))


def decode_case(name, dtype=np.float32):
    layout, b, h, tmax, length, d, dv, append, splits = DECODE_CASES[name]
    q, kc, vc, kn, vn = decode_inputs(np.random.RandomState(case_seed(name)), layout, b, h, tmax, d, dv, dtype)
    return dict(q=q, k_cache=kc, v_cache=vc, length=length, k_new=kn if append else None, v_new=vn if append else None,
                layout=layout, splits=splits)


# ---------------------------------------------------------------------- sampling
def tempered(logits, temperature, dtype):
    """z of the rule: x / temperature in the operand dtype, -0 counted as +0, as float64."""
    x = np.asarray(logits, dtype=dtype)
    with np.errstate(divide="ignore"):
        return (x / np.dtype(dtype).type(temperature)).astype(np.float64) + 0.0


def kept_set(z, top_k):
    """Booleans: every column for top_k None / 0 / >= V, else the top_k largest z with ties at the threshold to the LOWEST indices."""
    v = z.shape[0]
    if not top_k or top_k >= v:
        return np.ones(v, dtype=bool)
    order = np.lexsort((np.arange(v), -z))
    kept = np.zeros(v, dtype=bool)
    kept[order[:top_k]] = True
    return kept


class SampleRows(object):
    """Per row: kept [V], lo / hi [V] (the interval of every kept token on the normalised CDF; lo == hi off the kept set) and
    cdf_bound (a scalar)."""

    def __init__(self):
        self.kept, self.lo, self.hi, self.cdf_bound, self.argmax = [], [], [], [], []

    def tokens(self, u):
        """The rule's token per row for u [M] (float64 arithmetic on the exact intervals)."""
        out = np.empty(len(self.lo), dtype=np.int64)
        for r, ur in enumerate(np.asarray(u, dtype=np.float64)):
            hit = np.nonzero(self.kept[r] & (self.hi[r] > self.lo[r]) & (self.hi[r] > ur))[0]
            out[r] = hit[0] if hit.size else np.nonzero(self.kept[r] & (self.hi[r] > self.lo[r]))[0][-1]
        return out

    def margins(self, u, tokens=None):
        """Per row: the distance of u from the nearer NON-EXEMPT end of its token's interval, in units of cdf_bound (inf when
        both ends are exempt)."""
        tokens = self.tokens(u) if tokens is None else tokens
        out = np.empty(len(self.lo))
        for r, (ur, t) in enumerate(zip(np.asarray(u, dtype=np.float64), tokens)):
            lo, hi = self.lo[r][t], self.hi[r][t]
            positive = np.nonzero(self.kept[r] & (self.hi[r] > self.lo[r]))[0]
            d_lo = np.inf if lo == 0.0 else ur - lo
            d_hi = np.inf if t == positive[-1] else hi - ur
            out[r] = min(d_lo, d_hi) / self.cdf_bound[r]
        return out


def sample_reference(logits, temperature, top_k, dtype=np.float32):
    x = np.asarray(logits, dtype=dtype)
    res = SampleRows()
    res.argmax = np.argmax(x, axis=1).astype(np.int64)
    if temperature == 0.0:
        return res
    z = tempered(x, temperature, dtype)
    u = unit(dtype)
    for r in range(x.shape[0]):
        kept = kept_set(z[r], top_k)
        t = np.where(kept, z[r] - z[r][kept].max(), -np.inf)
        w = np.where(kept, np.exp(t), 0.0)
        run = np.cumsum(w)
        W = run[-1]
        hi = run / W
        lo = np.concatenate([[0.0], hi[:-1]])                 # (exactly 0 up to the first column of positive weight)
        last = np.nonzero(w > 0)[0][-1]
        hi[last:] = 1.0
        lo[last + 1:] = 1.0
        finite = w > 0
        res.kept.append(kept)
        res.lo.append(lo)
        res.hi.append(hi)
        res.cdf_bound.append(2 * u * float((w[finite] / W * (np.abs(t[finite]) + 2 * EXP_ULP)).sum()) + (2 * int(kept.sum()) + 3) * u)
    return res


def draw_u(res, rs, dtype, tries=1000):
    """u [M] in the operand dtype, each more than MARGIN bounds inside its token's interval: redrawn until it is."""
    m = len(res.lo)
    u = rs.random_sample(m).astype(dtype).astype(np.float64)
    for _ in range(tries):
        u = np.minimum(u, float(np.nextafter(np.dtype(dtype).type(1), np.dtype(dtype).type(0))))
        bad = res.margins(u) <= MARGIN
        if not bad.any():
            return u.astype(dtype)
        u[bad] = rs.random_sample(int(bad.sum())).astype(dtype).astype(np.float64)
    raise AssertionError("no u with the margin found in %d draws" % tries)


# name -> (M, V, temperature, top_k, spread)       the fixture's sampling cases
SAMPLE_CASES = {
    "plain": (5, 65, 1.0, None, 2.0),
    "top3_hot": (3, 1025, 2.0, 3, 3.0),
    "top_half_cold": (3, 64, 0.5, 32, 1.0),
}


def sample_inputs(rs, m, v, spread=2.0, dtype=np.float32):
    return (spread * rs.randn(m, v)).astype(dtype)


def sample_case(name, dtype=np.float32):
    m, v, temperature, top_k, spread = SAMPLE_CASES[name]
    return sample_inputs(np.random.RandomState(case_seed(name)), m, v, spread, dtype), temperature, top_k


# ---------------------------------------------------------------------- a one-block language model generated greedily
LM_PROMPT, LM_NEW = 4, 8          # token_oracle.LM_CASE: max_len 12


def lm_params(head_scale):
    """token_oracle.lm_initial() with the head's weights scaled by a power of two (still exact in float16)."""
    p = {k: np.asarray(v, dtype=np.float64) for k, v in to.lm_initial().items()}
    p["head.w"] = p["head.w"] * head_scale
    p["head.b"] = p["head.b"] * head_scale
    assert all(np.array_equal(v.astype(np.float16).astype(np.float64), v) for v in p.values())
    return p


def lm_logits(p, ids):
    """float64 logits [B, T, V] of the model for ids [B, T]."""
    c = to.LM_CASE
    b, t = ids.shape
    emb = to.embedding_reference(p["emb.tok"], ids, p["emb.pos"]).values["out"]
    blk = {k[len("block."):]: v for k, v in p.items() if k.startswith("block.")}
    h, _ = to._block(blk, emb, c["H"], c["eps"])
    ln = no.reference(h, p["ln.gamma"], p["ln.beta"], None, "layer", c["eps"]).values["y"].reshape(b * t, c["E"])
    return (ln @ p["head.w"] + p["head.b"]).reshape(b, t, c["V"])


def lm_prompt():
    return np.ascontiguousarray(to.lm_data()[0][:, :LM_PROMPT])


def lm_generate(p, prompt, new):
    """(ids [B, P + new], last-position logits of every step [new, B, V]) of greedy generation in float64."""
    ids, steps = np.array(prompt), []
    for _ in range(new):
        last = lm_logits(p, ids)[:, -1]
        steps.append(last)
        ids = np.concatenate([ids, np.argmax(last, axis=1)[:, None]], axis=1)
    return ids, np.stack(steps)


def top2_margin(step_logits):
    srt = np.sort(step_logits, axis=-1)
    return float((srt[..., -1] - srt[..., -2]).min())
