"""TEST INFRASTRUCTURE — the float64 yardstick of cache-extending attention (the reference has none): numpy only, built on
attn_oracle.reference.  T new rows at the absolute positions length .. length + T - 1 attend over the keys j <= their position:
that is the causal attention of Tq = Tk = length + T rows whose first `length` queries do not matter, so the live cache rows
and the new rows are concatenated, `length` zero queries are put in front, attn_oracle.reference runs with causal=True, and
the last T rows of its values and of its DERIVED bounds are the answer.  No new tolerance: the bounds and assert_within's
median gate are attn_oracle's.  (A row's bound grows with Tk = length + T — the bound of the longest row — which is what the
online softmax over all key blocks is entitled to.)  Grouped heads: k and v repeated over the group."""

import numpy as np

import attn_oracle as ao

unit, case_seed = ao.unit, ao.case_seed
AXES = {"bthd": (1, 2), "bhtd": (2, 1)}       # layout -> the (row, head) axes


def operand_shape(layout, b, h, rows, w):
    return (b, rows, h, w) if layout == "bthd" else (b, h, rows, w)


def rows_of(x, layout, start, stop):
    return x[:, start:stop] if layout == "bthd" else x[:, :, start:stop]


def put_rows(cache, layout, row, new):
    """cache with rows [row, row + T) of every (b, h) replaced by new (a copy)."""
    out = np.array(cache)
    t = new.shape[AXES[layout][0]]
    if layout == "bthd":
        out[:, row:row + t] = new
    else:
        out[:, :, row:row + t] = new
    return out


def extend_reference(q, k_cache, v_cache, length, k_new, v_new, scale=None, layout="bthd", dtype=np.float32):
    """Result: values["o"] (float64, q's layout and rows) with bounds["o"], and the caches after the append
    (values["k_cache"], values["v_cache"], in the dtype they came in)."""
    t_axis, h_axis = AXES[layout]
    t, h, hkv = q.shape[t_axis], q.shape[h_axis], k_cache.shape[h_axis]
    n = length + t
    k_after, v_after = put_rows(k_cache, layout, length, k_new), put_rows(v_cache, layout, length, v_new)
    k = np.repeat(rows_of(k_after, layout, 0, n), h // hkv, axis=h_axis)
    v = np.repeat(rows_of(v_after, layout, 0, n), h // hkv, axis=h_axis)
    front = list(q.shape)
    front[t_axis] = length
    q_all = np.concatenate([np.zeros(front, dtype=np.float64), np.asarray(q, dtype=np.float64)], axis=t_axis)
    scale = float(ao.default_scale(q) if scale is None else scale)
    res = ao.reference(q_all, k, v, None, True, scale, layout, dtype)
    out = ao.Result()
    out.values["o"] = np.ascontiguousarray(rows_of(res.values["o"], layout, length, n))
    out.bounds["o"] = np.ascontiguousarray(rows_of(res.bounds["o"], layout, length, n))
    out.values["k_cache"], out.values["v_cache"] = k_after, v_after
    return out


def extend_inputs(rs, layout, b, h, hkv, tmax, t, d, dv, dtype=np.float32, q_amp=4.0):
    """(q, k_cache, v_cache, k_new, v_new) with attn_oracle's amplitudes: q <= 4, k 1, v 3."""
    return ((rs.randn(*operand_shape(layout, b, h, t, d)) * q_amp).astype(dtype),
            rs.randn(*operand_shape(layout, b, hkv, tmax, d)).astype(dtype),
            (rs.randn(*operand_shape(layout, b, hkv, tmax, dv)) * 3).astype(dtype),
            rs.randn(*operand_shape(layout, b, hkv, t, d)).astype(dtype),
            (rs.randn(*operand_shape(layout, b, hkv, t, dv)) * 3).astype(dtype))


# name -> (layout, B, H, Hkv, Tmax, length, T, D, Dv, scale (None: 1 / sqrt(D)))     the fixture's cases (tests/gen_extend_golden.py)
EXTEND_CASES = {
    "extend_bthd": ("bthd", 2, 2, 2, 80, 70, 9, 8, 6, None),
    "extend_bhtd_grouped": ("bhtd", 1, 4, 2, 140, 65, 11, 5, 3, None),
    "prefill_into_cache": ("bthd", 1, 2, 1, 8, 0, 5, 4, 3, 0.7),
    "last_row_fills_the_cache": ("bhtd", 2, 1, 1, 64, 63, 1, 8, 8, None),
}


def extend_case(name, dtype=np.float32):
    layout, b, h, hkv, tmax, length, t, d, dv, scale = EXTEND_CASES[name]
    q, kc, vc, kn, vn = extend_inputs(np.random.RandomState(case_seed(name)), layout, b, h, hkv, tmax, t, d, dv, dtype)
    return dict(q=q, k_cache=kc, v_cache=vc, length=length, k_new=kn, v_new=vn, layout=layout, scale=scale)
