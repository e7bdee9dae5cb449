"""TEST INFRASTRUCTURE — the float64 yardstick of the token embedding and the per-row cross-entropy (the reference has
neither): numpy only, the plain formulas (np.add.at for the table's gradient), the analytic gradients, the DERIVED first-order
error bounds of the tests, and a float64 replica of one small language model (embedding + positions -> causal pre-norm
TransformerBlock -> LayerNorm -> Dense head -> mean cross-entropy) built on tests/norm_oracle.py.

Bounds.  u = 2**-24 (float32) or 2 * 2**-53 (float64), as in norm_oracle; |.| elementwise; every bound is computed from the
float64 quantities, never from a result under test.  X = EXP_ULP = 2 and L = LOG_ULP = 4 (float32) / 2 (float64) are the
gates of tests/kernel_sweep.ULP_GATES for the device exp and log, in ulps (1 ulp = 2 u).

  embedding
    out    without pos: a copy, BIT-EXACT (bound 0); with pos: one addition, b = u |out|
    dtable[v] = sum of the c_v rows dy[m], ids[m] == v:   b = (c_v + 1) u sum|dy[m]|        c_v - 1 additions, ANY order
    dpos[t]   = sum over the B sequences:                 b = (B + 1) u sum_b|dy|
  cross-entropy of a row x (V columns), mx = max x, entries of -inf contribute exactly 0 everywhere
    d = x - mx:            b_d = u |d|
    e = exp(d):            b_e = e (b_d + 2 X u)
    s = sum e:             b_s = sum b_e + (V + 1) u s + R (2 X + 2 + range) u s
                           R = `rescales`: the times an implementation multiplies a partial sum by exp(old max - new max)
                           (0 for a two-pass evaluation; the streaming kernel: its steps over the row + 2 for the lanes and
                           the waves), range = mx - the least finite x bounds the exponent's own rounding
    lse = mx + log(s):     b_lse = b_s / s + 2 L u |log s| + u |lse|
    losses = lse - x[t]:   b_losses = b_lse + u |losses|                                    ignored rows: exactly 0
    loss = sum losses (/ n):  b_loss = (sum b_losses + (M + 1) u sum|losses|) (/ n) + u |loss|   n = counted rows, exact
    a = x - lse:           b_a = b_lse + u |a|
    p = exp(a):            b_p = p (b_a + 2 X u)
    dlogits = (p - [v == t]) g / n:   b = |g / n| (b_p + u |p - [v == t]|) + 3 u |dlogits|   ignored rows: exactly 0

The bounds are worst-case and loose; so that one cannot hide a defect, assert_within (norm_oracle's) also demands that the
MEDIAN of bound / (|ref| + tiny) over the elements is below MEDIAN_GATE — a condition on the inputs, not a measurement:
logits of a few units, with or without an offset of 1000, and gradients dy of unit scale meet it at every shape used by the
tests (checked on the CPU by tests/test_token_golden.py)."""

import math

import numpy as np

import norm_oracle as no

EXP_ULP = 2.0
LOG_ULP = {np.dtype(np.float32): 4.0, np.dtype(np.float64): 2.0}
MEDIAN_GATE = no.MEDIAN_GATE
unit, assert_within, check, case_seed, pack, unpack = no.unit, no.assert_within, no.check, no.case_seed, no.pack, no.unpack
Result = no.Result
EMBED_FIELDS = ("out", "dtable", "dpos")
XENT_FIELDS = ("lse", "losses", "loss", "count", "dlogits")


# ---------------------------------------------------------------------- embedding
def embedding_reference(table, ids, pos=None, dy=None, padding_idx=None, dtype=np.float32):
    """values / bounds of "out" and, with dy, "dtable" and "dpos" (None without pos).  ids outside [0, V) — which only
    device-resident ids can hold — give a zero token row and are skipped by the gradient; pos may hold more rows than
    ids.shape[-1]: the rest gets a zero gradient."""
    u = unit(dtype)
    table = np.asarray(table, dtype=np.float64)
    ids = np.asarray(ids, dtype=np.int64)
    v, e = table.shape
    flat = ids.reshape(-1)
    m = flat.size
    ok = (flat >= 0) & (flat < v)
    out = np.zeros((m, e))
    out[ok] = table[flat[ok]]
    res = Result()
    t = ids.shape[-1] if ids.ndim else 1
    if pos is not None:
        pos = np.asarray(pos, dtype=np.float64)
        out = (out.reshape(-1, t, e) + pos[:t]).reshape(m, e)
        res.bounds["out"] = (u * np.abs(out)).reshape(ids.shape + (e,))
    else:
        res.bounds["out"] = np.zeros(ids.shape + (e,))
    res.values["out"] = out.reshape(ids.shape + (e,))
    res.values["dtable"] = res.values["dpos"] = res.bounds["dtable"] = res.bounds["dpos"] = None
    if dy is None:
        return res
    g = np.asarray(dy, dtype=np.float64).reshape(m, e)
    take = ok if padding_idx is None else ok & (flat != padding_idx)
    dtable, mass = np.zeros((v, e)), np.zeros((v, e))
    np.add.at(dtable, flat[take], g[take])
    np.add.at(mass, flat[take], np.abs(g[take]))
    counts = np.bincount(flat[take], minlength=v).astype(np.float64)
    res.values["dtable"], res.bounds["dtable"] = dtable, (counts[:, None] + 1.0) * u * mass
    if pos is not None:
        g3 = g.reshape(-1, t, e)
        dpos, b_dpos = np.zeros(pos.shape), np.zeros(pos.shape)
        dpos[:t] = g3.sum(axis=0)
        b_dpos[:t] = (g3.shape[0] + 1) * u * np.abs(g3).sum(axis=0)
        res.values["dpos"], res.bounds["dpos"] = dpos, b_dpos
    return res


# ---------------------------------------------------------------------- cross-entropy
def cross_entropy_reference(logits, targets, ignore_index=None, reduction="mean", g=1.0, dtype=np.float32, rescales=0):
    """values / bounds of "lse", "losses", "loss", "count" and "dlogits" (for the upstream gradient g of the loss).  A target
    equal to ignore_index, or outside [0, V), is not counted."""
    u = unit(dtype)
    lg = LOG_ULP[np.dtype(dtype)]
    x = np.asarray(logits, dtype=np.float64)
    shape = x.shape
    v = shape[-1]
    x = x.reshape(-1, v)
    m = x.shape[0]
    t = np.asarray(targets, dtype=np.int64).reshape(m)
    valid = (t >= 0) & (t < v)
    if ignore_index is not None:
        valid &= t != ignore_index
    n = int(valid.sum())
    fin = np.isfinite(x)
    mx = x.max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        d = np.where(fin, x - mx, 0.0)
        e = np.where(fin, np.exp(d), 0.0)
        b_e = e * (u * np.abs(d) + 2 * EXP_ULP * u)
        s = e.sum(axis=1, keepdims=True)
        span = mx - np.where(fin, x, np.inf).min(axis=1, keepdims=True)
        b_s = b_e.sum(axis=1, keepdims=True) + (v + 1) * u * s + rescales * (2 * EXP_ULP + 2 + span) * u * s
        lse = mx + np.log(s)
        b_lse = b_s / s + 2 * lg * u * np.abs(np.log(s)) + u * np.abs(lse)
        safe_t = np.where(valid, t, 0)
        xt = x[np.arange(m), safe_t][:, None]
        losses = np.where(valid[:, None], lse - xt, 0.0)
        b_losses = np.where(valid[:, None], b_lse + u * np.abs(losses), 0.0)
        total, b_total = losses.sum(), b_losses.sum() + (m + 1) * u * np.abs(losses).sum()
        div = float(n) if (reduction == "mean" and n) else 1.0
        loss = total / div if n else 0.0
        b_loss = (b_total / div + u * abs(loss)) if n else 0.0
        a = np.where(fin, x - lse, 0.0)
        b_a = b_lse + u * np.abs(a)
        p = np.where(fin, np.exp(a), 0.0)
        b_p = p * (b_a + 2 * EXP_ULP * u)
        hot = (np.arange(v)[None, :] == t[:, None]) & valid[:, None]
        scale = float(g) / div if n else 0.0
        q = np.where(valid[:, None], p - hot, 0.0)
        dl = q * scale
        b_dl = np.where(valid[:, None], abs(scale) * (b_p + u * np.abs(q)) + 3 * u * np.abs(dl), 0.0)
    res = Result()
    rows = shape[:-1]
    res.values["lse"], res.bounds["lse"] = lse.reshape(rows), b_lse.reshape(rows)
    res.values["losses"], res.bounds["losses"] = losses.reshape(rows), b_losses.reshape(rows)
    res.values["loss"], res.bounds["loss"] = np.float64(loss), np.float64(b_loss)
    res.values["count"], res.bounds["count"] = np.float64(n), np.float64(0.0)
    res.values["dlogits"], res.bounds["dlogits"] = dl.reshape(shape), b_dl.reshape(shape)
    return res


def loss64(logits, targets, ignore_index=None, reduction="mean"):
    return float(cross_entropy_reference(logits, targets, ignore_index, reduction, dtype=np.float64).values["loss"])


# ---------------------------------------------------------------------- inputs and the fixture's cases
def embed_inputs(rs, v, e, ids_shape, max_len=None, dtype=np.float32):
    """(table, pos or None, dy): unit normals; float32 numbers in `dtype`."""
    table = rs.randn(v, e).astype(np.float32).astype(dtype)
    pos = None if max_len is None else rs.randn(max_len, e).astype(np.float32).astype(dtype)
    dy = rs.randn(*(tuple(ids_shape) + (e,))).astype(np.float32).astype(dtype)
    return table, pos, dy


def xent_inputs(rs, m, v, offset=0.0, spread=2.0, dtype=np.float32):
    """(logits [m, v], targets [m]): offset + spread * normal; targets uniform, the first at 0 and the last at v - 1."""
    x = (offset + spread * rs.randn(m, v)).astype(np.float32).astype(dtype)
    t = rs.randint(0, v, m).astype(np.int64)
    t[0], t[-1] = 0, v - 1
    return x, t


# name -> (V, E, ids shape, max_len or None, padding_idx or None, id pattern)
EMBED_CASES = {
    "embed_repeat": (5, 4, (4,), None, None, "fixed"),          # ids [3, 1, 3, 3]: the case getitem_'s vjp gets wrong
    "embed_pos": (7, 5, (3, 6), 8, None, "random"),
    "embed_padding": (7, 3, (2, 9), 9, 2, "random"),
    "embed_all_equal": (3, 65, (2, 70), None, None, "equal"),   # one token owns 140 positions: more than two segments
}
# name -> (M, V, offset, ignore_index or None, reduction, g, rows ignored)
XENT_CASES = {
    "xent_small": (4, 5, 0.0, None, "mean", 1.0, ()),
    "xent_sum_g": (5, 64, 0.0, None, "sum", -0.75, ()),
    "xent_ignore": (6, 65, 0.0, 3, "mean", 2.5, (1, 4)),
    "xent_all_ignored": (3, 7, 0.0, 2, "mean", 1.0, (0, 1, 2)),
    "xent_offset": (4, 63, 1000.0, None, "mean", 1.0, ()),
    "xent_neg_inf": (3, 9, 0.0, None, "mean", 1.0, ()),
    "xent_single_class": (3, 1, 0.0, None, "mean", 1.0, ()),
}


def embed_case(name, dtype=np.float32):
    """(table, ids, pos, dy, padding_idx) of an EMBED_CASES entry."""
    v, e, ids_shape, max_len, padding_idx, pattern = EMBED_CASES[name]
    rs = np.random.RandomState(case_seed(name))
    table, pos, dy = embed_inputs(rs, v, e, ids_shape, max_len, dtype)
    if pattern == "fixed":
        ids = np.array([3, 1, 3, 3], dtype=np.int64)
    elif pattern == "equal":
        ids = np.full(ids_shape, v - 1, dtype=np.int64)
    else:
        ids = rs.randint(0, v, ids_shape).astype(np.int64)
    return table, ids, pos, dy, padding_idx


def xent_case(name, dtype=np.float32):
    """(logits, targets, ignore_index, reduction, g) of an XENT_CASES entry."""
    m, v, offset, ignore_index, reduction, g, ignored = XENT_CASES[name]
    rs = np.random.RandomState(case_seed(name))
    x, t = xent_inputs(rs, m, v, offset, dtype=dtype)
    if ignore_index is not None:
        t[t == ignore_index] = (ignore_index + 1) % v
        t[list(ignored)] = ignore_index
    if name == "xent_neg_inf":
        x[:, 1::3] = -np.inf
        t[:] = [0, 2, 8]
    return x, t, ignore_index, reduction, g


def embed_fields(name):
    v, e, ids_shape, max_len, _, _ = EMBED_CASES[name]
    layout = [("out", tuple(ids_shape) + (e,)), ("dtable", (v, e))]
    return layout + ([("dpos", (max_len, e))] if max_len is not None else [])


def xent_fields(name):
    m, v = XENT_CASES[name][:2]
    return [("lse", (m,)), ("losses", (m,)), ("loss", ()), ("count", ()), ("dlogits", (m, v))]


# ---------------------------------------------------------------------- float64 language-model replica
LM_CASE = dict(B=3, T=9, V=11, E=16, H=2, hidden=32, max_len=12, eps=1e-5, lr=1e-3)
LM_NAMES = ("emb.tok", "emb.pos") + tuple("block." + n for n in no.BLOCK_NAMES) + ("ln.gamma", "ln.beta", "head.w", "head.b")


def lm_shapes():
    c = LM_CASE
    shapes = {"emb.tok": (c["V"], c["E"]), "emb.pos": (c["max_len"], c["E"]), "ln.gamma": (1, c["E"]), "ln.beta": (1, c["E"]),
              "head.w": (c["E"], c["V"]), "head.b": (1, c["V"])}
    for name, shape in no.block_shapes(c["E"], c["hidden"]).items():
        shapes["block." + name] = shape
    return shapes


def lm_layout():
    shapes = lm_shapes()
    return [(name, shapes[name]) for name in LM_NAMES]


def lm_data():
    """(ids [B, T], targets [B, T]) int64: repeated ids in every sequence; two targets are the ignored class IGNORE."""
    c = LM_CASE
    rs = np.random.RandomState(case_seed("language_model"))
    stream = rs.randint(0, c["V"], (c["B"], 4))[:, np.arange(c["T"] + 1) % 4]
    return np.ascontiguousarray(stream[:, :-1]), np.ascontiguousarray(stream[:, 1:])


def lm_initial():
    """Initial parameters: multiples of 2**-10 (exact in float16, which is how the fixture stores them)."""
    rs = np.random.RandomState(case_seed("language_model_parameters"))
    out = {}
    for name, shape in lm_layout():
        if name.endswith(".gamma"):
            vals = 1.0 + 0.25 * rs.randn(*shape)
        elif name.startswith("emb."):
            vals = 0.5 * rs.randn(*shape)
        elif shape[0] == 1:
            vals = 0.1 * rs.randn(*shape)
        else:
            vals = rs.uniform(-1.0, 1.0, shape) * math.sqrt(6.0 / (shape[0] + shape[1]))
        out[name] = (np.round(vals * 1024.0) / 1024.0).astype(np.float16)
    return out


def _block(p, x, heads, eps):
    """The causal pre-norm block of norm_oracle.block_loss_and_grads, split: (out, backward) where backward(dout) gives
    ({name: gradient}, dx)."""
    b, t, e = x.shape
    hd = e // heads
    ln1 = no.reference(x, p["ln1.gamma"], p["ln1.beta"], None, "layer", eps).values["y"]
    rows = ln1.reshape(b * t, e)
    q, k, v = ((rows @ p["attn.w" + n] + p["attn.b" + n]).reshape(b, t, heads, hd).transpose(0, 2, 1, 3) for n in "qkv")
    s = q @ k.transpose(0, 1, 3, 2) / math.sqrt(hd)
    s = np.where(np.arange(t)[None, :] <= np.arange(t)[:, None], s, -np.inf)
    pr = np.exp(s - s.max(axis=-1, keepdims=True))
    pr /= pr.sum(axis=-1, keepdims=True)
    att = (pr @ v).transpose(0, 2, 1, 3).reshape(b * t, e)
    h = x + (att @ p["attn.wo"] + p["attn.bo"]).reshape(b, t, e)
    ln2 = no.reference(h, p["ln2.gamma"], p["ln2.beta"], None, "layer", eps).values["y"].reshape(b * t, e)
    z = ln2 @ p["fc1.w"] + p["fc1.b"]
    act = no.gelu64(z, "tanh")
    out = h + (act @ p["fc2.w"] + p["fc2.b"]).reshape(b, t, e)

    def backward(dout):
        g = {}
        d2 = dout.reshape(b * t, e)
        g["fc2.w"], g["fc2.b"] = act.T @ d2, d2.sum(0, keepdims=True)
        dz = no.gelu_reference(z, d2 @ p["fc2.w"].T, "tanh").values["dx"]
        g["fc1.w"], g["fc1.b"] = ln2.T @ dz, dz.sum(0, keepdims=True)
        r2 = no.reference(h, p["ln2.gamma"], p["ln2.beta"], (dz @ p["fc1.w"].T).reshape(b, t, e), "layer", eps).values
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
                g["attn.bk.terms"] = np.abs(dn).sum(0, keepdims=True)
            drows += dn @ p["attn.w" + n].T
        r1 = no.reference(x, p["ln1.gamma"], p["ln1.beta"], drows.reshape(b, t, e), "layer", eps).values
        g["ln1.gamma"], g["ln1.beta"] = r1["dgamma"].reshape(1, e), r1["dbeta"].reshape(1, e)
        return g, dh + r1["dx"]
    return out, backward


LM_IGNORE = 10     # the class of LM_CASE that the fixture's loss ignores (two targets are set to it)


def lm_targets(targets):
    t = np.array(targets)
    t[0, 0] = t[-1, -1] = LM_IGNORE
    return t


def lm_loss_and_grads(params, ids, targets, with_bk_terms=False):
    """float64 mean cross-entropy (ignore_index LM_IGNORE) of the model and the gradient of every parameter.  The gradient of
    block.attn.bk is mathematically zero (norm_oracle.block_loss_and_grads): with_bk_terms=True also returns the sum of
    |terms| behind each of its elements, which is what it is judged against."""
    c = LM_CASE
    p = {k: np.asarray(v, dtype=np.float64) for k, v in params.items()}
    b, t = ids.shape
    emb = embedding_reference(p["emb.tok"], ids, p["emb.pos"]).values["out"]
    blk = {k[len("block."):]: v for k, v in p.items() if k.startswith("block.")}
    h, block_bwd = _block(blk, emb, c["H"], c["eps"])
    ln = no.reference(h, p["ln.gamma"], p["ln.beta"], None, "layer", c["eps"]).values["y"].reshape(b * t, c["E"])
    logits = ln @ p["head.w"] + p["head.b"]
    xe = cross_entropy_reference(logits, targets.reshape(-1), LM_IGNORE, "mean", dtype=np.float64).values
    g = {}
    dl = xe["dlogits"]
    g["head.w"], g["head.b"] = ln.T @ dl, dl.sum(0, keepdims=True)
    r = no.reference(h, p["ln.gamma"], p["ln.beta"], (dl @ p["head.w"].T).reshape(b, t, c["E"]), "layer", c["eps"]).values
    g["ln.gamma"], g["ln.beta"] = r["dgamma"].reshape(1, -1), r["dbeta"].reshape(1, -1)
    gb, demb = block_bwd(r["dx"])
    for k, v in gb.items():
        g["block." + k] = v
    er = embedding_reference(p["emb.tok"], ids, p["emb.pos"], demb, dtype=np.float64).values
    g["emb.tok"], g["emb.pos"] = er["dtable"], er["dpos"]
    grads = {name: g[name] for name in LM_NAMES}
    return (float(xe["loss"]), grads, g["block.attn.bk.terms"]) if with_bk_terms else (float(xe["loss"]), grads)
