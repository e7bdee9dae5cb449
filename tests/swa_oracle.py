"""TEST INFRASTRUCTURE — the float64 yardstick of sliding-window causal attention (include/tnn_swa.h): numpy only, the rule
(query i keeps key j iff i - W < j <= i) with its analytic gradients, for plain and grouped heads.  Bounds: the error model
of tests/attn_oracle.py (same MFMA, same online softmax, fewer terms per row) with the row's kept-key count
n_i = min(i + 1, W) in place of Tk and the count c_j = min(T - j, W) of the queries that see key j in place of Tq."""

import numpy as np

import attn_oracle as ao


def keep(T, W):
    i, j = np.arange(T)[:, None], np.arange(T)[None, :]
    return (j <= i) & (j > i - W)


def reference(q, k, v, do, W, layout, group=1, scale=None, dtype=np.float32):
    """ao.Result of forward and gradients; k and v hold H / group heads (layout "bthd" when group > 1), and dk, dv are summed
    over each key / value head's group of query heads."""
    scale = float(ao.default_scale(q) if scale is None else scale)
    rep = (lambda x: np.repeat(x, group, axis=2)) if group > 1 else (lambda x: x)
    q3, k3, v3, g3 = ao.to3(q, layout), ao.to3(rep(k), layout), ao.to3(rep(v), layout), ao.to3(do, layout)
    T, d = q3.shape[1:]
    dv_ = v3.shape[2]
    kp = keep(T, W)[None]
    n = kp.sum(axis=-1, keepdims=True).astype(np.float64)             # [1, T, 1] kept keys of a row
    c = kp.sum(axis=-2)[..., None].astype(np.float64)                 # [1, T, 1] queries that see a key
    s = np.where(kp, scale * np.einsum("bid,bjd->bij", q3, k3), -np.inf)
    m = s.max(axis=-1, keepdims=True)
    e = np.exp(s - m)
    l = e.sum(axis=-1, keepdims=True)
    p = e / l
    o3 = p @ v3
    lse3 = (m + np.log(l))[..., 0]
    u = ao.unit(dtype)
    absqk = np.where(kp, np.einsum("bid,bjd->bij", np.abs(q3), np.abs(k3)), 0.0)
    E = (d + 3) * u * abs(scale) * absqk.max(axis=-1, keepdims=True)
    rho = 2 * E + (n + ao.EXP_ULP + 4) * u
    b_o = (rho + (n + 2) * u) * (p @ np.abs(v3))
    b_lse = E[..., 0] + (n[..., 0] + ao.EXP_ULP + 4) * u + u * np.abs(lse3)
    dP = np.einsum("bic,bjc->bij", g3, v3)
    delta = (g3 * o3).sum(axis=-1, keepdims=True)
    dS = p * (dP - delta)
    dS[np.broadcast_to(n == 1, dS.shape)] = 0.0                        # one kept key: p = 1, dP = delta exactly
    dq3 = scale * (dS @ k3)
    dk3 = scale * np.einsum("bij,bid->bjd", dS, q3)
    dv3 = np.einsum("bij,bic->bjc", p, g3)
    ag = np.abs(g3)
    cg = group * c                                                    # terms summed into a key's dk / dv: c per query head
    b_dv = np.einsum("bij,bic->bjc", p, rho * ag) + (cg + 2) * u * np.einsum("bij,bic->bjc", p, ag)
    F = (dv_ + 2) * u * np.einsum("bic,bjc->bij", ag, np.abs(v3))
    b_delta = (dv_ + 2) * u * (ag * np.abs(o3)).sum(axis=-1, keepdims=True) + (ag * b_o).sum(axis=-1, keepdims=True)
    b_dS = rho * np.abs(dS) + p * (F + b_delta) + 2 * u * p * (np.abs(dP) + np.abs(delta))
    b_dq = abs(scale) * ((n + 3) * u * (np.abs(dS) @ np.abs(k3)) + b_dS @ np.abs(k3))
    b_dk = abs(scale) * ((cg + 3) * u * np.einsum("bij,bid->bjd", np.abs(dS), np.abs(q3))
                         + np.einsum("bij,bid->bjd", b_dS, np.abs(q3)))
    res = ao.Result()
    ls = ao.lse_shape(np.shape(q), layout)
    res.values["lse"], res.bounds["lse"] = lse3.reshape(ls), b_lse.reshape(ls)
    fold = (lambda x: x.reshape(x.shape[0], x.shape[1], -1, group, x.shape[3]).sum(axis=3)) if group > 1 else (lambda x: x)
    for name, val, bnd, like, sum_ in (("o", o3, b_o, q, False), ("dq", dq3, b_dq, q, False), ("dk", dk3, b_dk, rep(k), True),
                                       ("dv", dv3, b_dv, rep(v), True)):
        val, bnd = ao.from3(val, layout, np.shape(like)), ao.from3(bnd, layout, np.shape(like))
        res.values[name], res.bounds[name] = (fold(val), fold(bnd)) if sum_ else (val, bnd)
    return res


def decode(q, k_rows, v_rows, group=1, scale=None):
    """o [B, H, Dv] of one query per head over an explicit list of rows k_rows [B, n, Hkv, D], v_rows [B, n, Hkv, Dv]."""
    scale = float(1.0 / np.sqrt(q.shape[-1]) if scale is None else scale)
    k, v = (np.repeat(np.asarray(x, dtype=np.float64), group, axis=2) for x in (k_rows, v_rows))
    s = scale * np.einsum("bhd,bnhd->bhn", np.asarray(q, dtype=np.float64), k)
    p = np.exp(s - s.max(axis=-1, keepdims=True))
    return np.einsum("bhn,bnhc->bhc", p / p.sum(axis=-1, keepdims=True), v)


def ring_of(hist, n, R):
    """[B, R, ...]: the last min(n, R) of the first n rows of hist [B, T, ...], row t in slot t mod R, zeros elsewhere."""
    ring = np.zeros((hist.shape[0], R) + hist.shape[2:], hist.dtype)
    for t in range(max(0, n - R), n):
        ring[:, t % R] = hist[:, t]
    return ring
