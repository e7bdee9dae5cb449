"""TEST INFRASTRUCTURE of attention with per-sequence lengths, shared by tests/gen_varlen_golden.py, the CPU tests and
tests/test_gpu_varlen.py: the oracle — tests/attn_oracle.py (gqa_oracle for grouped heads) applied PER SEQUENCE to the operands
cut to lens[b] rows, zeros elsewhere, its derived bounds the tolerances (a dead element's bound is 0: it must be exactly 0) —
the raw calls of one route as numpy arrays, the NaN poison of dead rows, and the named cases of the fixture."""

import os

import numpy as np

import attn_oracle as ao
import gqa_oracle as go
import tinynn_autograd_amd as tn
from norm_support import dev
from tinynn_autograd_amd import device_array as da

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "varlen_cases.npz")
FIELDS = ("o", "lse", "delta", "dq", "dk", "dv")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def load_golden():
    with np.load(GOLDEN) as data:
        return dict(data)


def rows(x, layout, b, n):
    """Rows [0, n) of sequence b as a batch of one."""
    return x[b:b + 1, :n]              # "bthd" [B, T, H, W] and three-axis "bhtd" [B, T, W] both have T on axis 1


def reference(q, k, v, do_, lens, causal=False, scale=None, layout="bthd", dtype=np.float32):
    """The oracle per sequence on the operands cut to lens[b] rows; zeros (values and bounds) elsewhere.  scale None:
    1 / sqrt(D), as everywhere."""
    q, k, v, do_ = (np.asarray(a) for a in (q, k, v, do_))
    res = ao.Result()
    shapes = dict(o=do_.shape, dq=q.shape, dk=k.shape, dv=v.shape, lse=ao.lse_shape(q.shape, layout),
                  delta=ao.lse_shape(q.shape, layout))
    for name, shape in shapes.items():
        res.values[name], res.bounds[name] = np.zeros(shape), np.zeros(shape)
    scale = float(ao.default_scale(q) if scale is None else scale)
    for b, n in enumerate(int(x) for x in lens):
        if n == 0:
            continue
        cut = [rows(a, layout, b, n) for a in (q, k, v, do_)]
        one = (go.reference(*cut, causal=causal, scale=scale, dtype=dtype) if layout == "bthd"
               else ao.reference(*cut, causal=causal, scale=scale, layout="bhtd", dtype=dtype))
        for name in ("o", "dq", "dk", "dv"):
            res.values[name][b:b + 1, :n] = one.values[name]
            res.bounds[name][b:b + 1, :n] = one.bounds[name]
        res.values["lse"][b, ..., :n], res.bounds["lse"][b, ..., :n] = one.values["lse"][0], one.bounds["lse"][0]
        res.values["delta"][b, ..., :n] = one.values["delta"][0]
    # attn_oracle's b_delta (its docstring), which it folds into the bounds of dq and dk, stated for delta itself
    u, ag = ao.unit(dtype), np.abs(np.asarray(do_, dtype=np.float64))
    b_delta = ((v.shape[-1] + 2) * u * ag * np.abs(res.values["o"]) + ag * res.bounds["o"]).sum(axis=-1)
    res.bounds["delta"] = b_delta.transpose(0, 2, 1) if layout == "bthd" else b_delta
    return res


def dead(shape_like, lens, field, layout):
    """Boolean array of the dead elements of a field."""
    lens = np.asarray(lens).reshape(-1)
    t = shape_like.shape[-1] if field in ("lse", "delta") else shape_like.shape[1]
    gone = np.arange(t)[None, :] >= lens[:, None]                      # [B, T]
    if field in ("lse", "delta"):
        gone = gone if shape_like.ndim == 2 else gone[:, None, :]
    else:
        gone = gone.reshape(gone.shape + (1,) * (shape_like.ndim - 2))
    return np.broadcast_to(gone, shape_like.shape)


def assert_dead_are_plus_zero(got, lens, layout, what):
    for name, a in got.items():
        if a is None:
            continue
        gone = dead(a, lens, name, layout)
        assert not bits(a)[gone].any(), "%s %s: a dead element is not +0" % (what, name)


def poisoned(arrays, lens, layout):
    """Copies with NaN in every dead row."""
    out = []
    for a in arrays:
        a = np.array(a)
        for b, n in enumerate(int(x) for x in lens):
            a[b, n:] = np.nan
        out.append(a)
    return out


def run(route, q, k, v, do_, lens, causal, scale, layout, dtype, unaligned=False, need=(True, True, True), o_poison=False,
        lens_dev=None):
    """The three raw calls of one route with lens= -> {name: numpy array or None}.  The grouped functions serve layout "bthd"
    (Hkv == H included: tnn_varlen_* is one family), the plain ones three-axis "bhtd".  o_poison: NaN is written into the dead
    rows of the forward's o before the backward reads it."""
    qd, kd, vd, dod = (dev(a, dtype, unaligned) for a in (q, k, v, do_))
    ld = da.lengths(lens) if lens_dev is None else lens_dev
    opts = dict(causal=causal, scale=scale, route=route, lens=ld)
    if layout == "bthd":
        fwd, bq, bkv = da.gqa_attention, da.gqa_attention_bwd_q, da.gqa_attention_bwd_kv
    else:
        fwd, bq, bkv = da.attention, da.attention_bwd_q, da.attention_bwd_kv
        opts["layout"] = "bhtd"
    o, lse = fwd(qd, kd, vd, **opts)
    o_in = o
    if o_poison:
        o_in = tn.asarray(poisoned([np.asarray(o)], lens, layout)[0], dtype=dtype)
    dq, delta = bq(qd, kd, vd, o_in, dod, lse, need_dq=need[0], **opts)
    dk, dv = bkv(qd, kd, vd, dod, lse, delta, need_dk=need[1], need_dv=need[2], **opts)
    out = dict(o=o, lse=lse, delta=delta, dq=dq, dk=dk, dv=dv)
    return {n: None if a is None else np.asarray(a) for n, a in out.items()}


def run_plain(route, q, k, v, do_, lens, causal, scale, dtype, **kw):
    """run() through the PLAIN functions in layout "bthd" (Hkv == H)."""
    qd, kd, vd, dod = (dev(a, dtype) for a in (q, k, v, do_))
    opts = dict(causal=causal, scale=scale, route=route, lens=da.lengths(lens), layout="bthd")
    o, lse = da.attention(qd, kd, vd, **opts)
    dq, delta = da.attention_bwd_q(qd, kd, vd, o, dod, lse, **opts)
    dk, dv = da.attention_bwd_kv(qd, kd, vd, dod, lse, delta, **opts)
    return {n: np.asarray(a) for n, a in dict(o=o, lse=lse, delta=delta, dq=dq, dk=dk, dv=dv).items()}


def check(got, res, what, factor=1.0, fields=FIELDS, verbose=False):
    for name in fields:
        if got.get(name) is None:
            continue
        if name == "delta":            # (a sum that may cancel: the elementwise bound alone, without the median gate)
            err = np.abs(got[name].astype(np.float64) - res.values[name])
            assert (err <= factor * res.bounds[name]).all(), "%s delta: error exceeds the derived bound by %.3e" % (
                what, float((err - factor * res.bounds[name]).max()))
            continue
        ao.assert_within(got[name], res.values[name], res.bounds[name], "%s %s" % (what, name), factor, verbose)


def make_inputs(seed, layout, b, h, hkv, t, d, dv, dtype=np.float32, q_amp=4.0):
    """(q, k, v, do) with attn_oracle's amplitudes; layout "bhtd": three axes (h == hkv == 1)."""
    rs = np.random.RandomState(seed)
    if layout == "bthd":
        return go.make_inputs(rs, b, h, hkv, t, t, d, dv, dtype, q_amp)
    assert h == hkv == 1
    q, k, v, do_ = ao.make_inputs(rs, "bhtd", b, 1, t, t, d, dv, dtype, q_amp)
    return tuple(a.reshape(b, t, a.shape[-1]) for a in (q, k, v, do_))


# name -> (layout, B, H, Hkv, T, D, Dv, lens, causal, scale (None: 1 / sqrt(D)))        the fixture's cases
VARLEN_CASES = {
    "bthd_causal": ("bthd", 4, 2, 2, 9, 5, 3, (9, 0, 1, 6), True, None),
    "bthd_full": ("bthd", 3, 2, 2, 7, 4, 6, (3, 7, 5), False, 0.6),
    "bthd_grouped": ("bthd", 3, 4, 2, 11, 8, 8, (11, 4, 0), True, None),
    "bthd_mqa_block": ("bthd", 2, 4, 1, 70, 5, 3, (70, 37), False, None),
    "bhtd_three_axes": ("bhtd", 4, 1, 1, 13, 6, 4, (1, 13, 8, 0), True, None),
}


def case_input(name, dtype=np.float32):
    layout, b, h, hkv, t, d, dv, lens, causal, scale = VARLEN_CASES[name]
    return make_inputs(ao.case_seed(name), layout, b, h, hkv, t, d, dv, dtype, q_amp=2.0) + (np.array(lens), causal, scale, layout)
