"""TEST INFRASTRUCTURE — the float64 yardstick of the fused linear + cross-entropy (include/tnn_lce.h): numpy only, the plain
loss of z = h w + b against integer targets from the float32 operands, its analytic gradients, and the DERIVED first-order
bounds for an evaluation in float32, in the shape of tests/attn_oracle.py with the contraction length K in place of D, V in
place of Tk, and the bias.

Bounds.  u = 2**-24; X = 2, the exp / log gate of tests/kernel_sweep.ULP_GATES; |.| elementwise; S = the splits merged (at
most lce.MAX_SPLITS); n = the backward's chunks.  Columns whose bias is -inf have z = -inf, p = 0 and dz = 0 exactly.

    E_mv     = (K + 3) u (sum_k |h_mk| |w_kv| + |b_v|)          error of one logit: a length-K dot product plus the bias
    E_m      = max_v E_mv
    tail     = (V + S + 2 X + 8) u                              the row sum, the merge of S pairs, exp and log
    |lse - lse64|       <= E_m + tail + u |lse64|
    |losses - losses64| <= bound_lse + E_mt + u |losses64|      (0 for a row that is not counted)
    |loss - loss64|     <= [sum_m bound_losses + (M + 2) u sum_m |losses64|] / count + 2 u |loss64|      ("sum": count = 1)
    rho_m    = 2 E_m + tail + u |lse64| + (X + 1) u             relative error of p_mv = exp(z - lse)
    |dz - dz64|         <= |g / count| (rho_m p + 3 u |p - [v == t]|)
    |dh - dh64|         <= (V + 3) u (|dz64| |w|^T) + bound_dz |w|^T
    |dw - dw64|         <= (M + n + 3) u (|h|^T |dz64|) + |h|^T bound_dz          (n: one more rounding per beta = 1 pass)
    |db - db64|         <= (M + n + 3) u sum_m |dz64| + sum_m bound_dz

assert_within is attn_oracle's: it also holds the MEDIAN of bound / |ref| under MEDIAN_GATE, a condition on the inputs that
inputs() meets (tests/test_lce_host.py checks it on the reference alone); an all-zero reference (V = 1) is exempt, as there."""

import numpy as np

from attn_oracle import EXP_ULP, U32, Result, assert_within      # noqa: F401  (assert_within: what the tests call)

def inputs(rs, m, k, v, bias=True):
    """(h, w, b) float32 with the amplitudes the median gate is stated for: h 1, w 1, b 2."""
    return (rs.randn(m, k).astype(np.float32), rs.randn(k, v).astype(np.float32),
            (rs.randn(1, v) * 2).astype(np.float32) if bias else None)


def reference(h, w, b, targets, ignore_index=None, reduction="mean", g=1.0, splits=64, chunks=1):
    """Forward, gradients for the upstream gradient g, and the bounds of the module docstring."""
    h, w = np.asarray(h, dtype=np.float64), np.asarray(w, dtype=np.float64)
    m, k = h.shape
    v = w.shape[1]
    bias = np.zeros(v) if b is None else np.asarray(b, dtype=np.float64).reshape(v)
    t = np.asarray(targets).reshape(m)
    counted = (t >= 0) & (t < v) & (t != (-1 if ignore_index is None else ignore_index))
    tc = np.where(counted, t, 0)
    u, finite = U32, np.isfinite(bias)
    z = h @ w + bias
    E = np.where(finite, (k + 3) * u * (np.abs(h) @ np.abs(w) + np.where(finite, np.abs(bias), 0.0)), 0.0)
    Em = E.max(axis=1)
    mx = z.max(axis=1, keepdims=True)
    p = np.exp(z - mx)
    lse = mx[:, 0] + np.log(p.sum(axis=1))
    p = p / p.sum(axis=1, keepdims=True)
    tail = (v + splits + 2 * EXP_ULP + 8) * u
    res = Result()
    b_lse = Em + tail + u * np.abs(lse)
    losses = np.where(counted, lse - z[np.arange(m), tc], 0.0)
    b_losses = np.where(counted, b_lse + E[np.arange(m), tc] + u * np.abs(losses), 0.0)
    n = int(counted.sum())
    div = float(n) if reduction == "mean" else 1.0
    loss = losses.sum() / div if n else 0.0
    b_loss = (b_losses.sum() + (m + 2) * u * np.abs(losses).sum()) / div + 2 * u * abs(loss) if n else 0.0
    scale = g / div if n else 0.0
    onehot = (np.arange(v)[None, :] == t[:, None]) & counted[:, None]
    dz = np.where(counted[:, None], (p - onehot) * scale, 0.0)
    rho = (2 * Em + tail + u * np.abs(lse) + (EXP_ULP + 1) * u)[:, None]
    b_dz = np.where(counted[:, None], abs(scale) * (rho * p + 3 * u * np.abs(p - onehot)), 0.0)
    aw, ah, adz = np.abs(w), np.abs(h), np.abs(dz)
    res.values.update(lse=lse, losses=losses, loss=np.float64(loss), count=float(n), dz=dz, dh=dz @ w.T, dw=h.T @ dz,
                      db=dz.sum(axis=0))
    res.bounds.update(lse=b_lse, losses=b_losses, loss=np.float64(b_loss), dz=b_dz,
                      dh=(v + 3) * u * (adz @ aw.T) + b_dz @ aw.T,
                      dw=(m + chunks + 3) * u * (ah.T @ adz) + ah.T @ b_dz,
                      db=(m + chunks + 3) * u * adz.sum(axis=0) + b_dz.sum(axis=0))
    return res


def check(got, res, what, factor=1.0, verbose=False):
    """got: {name: array}; every named field that is not None against the oracle."""
    for name in got:
        if got[name] is not None and name in res.bounds:
            assert_within(np.reshape(got[name], np.shape(res.values[name])), res.values[name], res.bounds[name],
                          "%s %s" % (what, name), factor, verbose)
