"""TEST INFRASTRUCTURE shared by tests/test_ragged_host.py (CPU twin) and tests/test_gpu_ragged.py (MI355X): an independent
numpy model of the step's bookkeeping, the expected output of a ragged generation built from decode_oracle's float64
generations of every sequence ALONE, and the runs that pin the kernels (batch slices through the uniform kernel)."""

import numpy as np

import decode_oracle as do
import decode_support as ds
import tinynn_autograd_amd as tn
from norm_support import dev
from tinynn_autograd_amd import device_array as da

PROMPT_LENS = (4, 2, 3)        # of the fixture's three sequences (do.lm_prompt() is [3, 4])
EOS, PAD = 0, 5                # sequence 0 ends on its first new token, sequence 1 on its third, sequence 2 never


def advance_model(state, picked, eos, pad):
    """include/tnn_ragged.h's rule, vectorised (written apart from ragged.advance_host, which loops).  state: a dict of
    numpy arrays lens, start, done, out, cur and, optionally, u_all / u_cur; returns the new dict."""
    s = {k: np.array(v) for k, v in state.items()}
    B, Tout = s["out"].shape
    L = s["lens"] + 1
    s["lens"] = L
    tok = np.where(s["done"] != 0, pad, picked)
    rows = np.nonzero((L >= 0) & (L < Tout))[0]
    s["out"][rows, L[rows]] = tok[rows]
    s["cur"] = tok.astype(np.int64)
    if eos >= 0:
        s["done"] = np.where(tok == eos, 1, s["done"])
    if "u_all" in s:
        n = L + 1 - s["start"]
        rows = np.nonzero((n >= 0) & (n < s["u_all"].shape[0]))[0]
        s["u_cur"][rows] = s["u_all"][n[rows], rows]
    return s


def lm_alone(golden, prompt, lens, new):
    """[(ids [P_b + new], step logits [new, 1, V])] of every sequence generated ALONE, greedily, in float64."""
    params = do.lm_params(float(golden["lm.head_scale"]))
    out = []
    for b, p in enumerate(lens):
        ids, steps = do.lm_generate(params, prompt[b:b + 1, :p], new)
        out.append((ids[0], steps))
    return out


def expected_ids(alone, lens, pmax, new, eos=None, pad=0):
    """The layout of generate's ragged result: the prompt, `new` tokens (pad after an eos), trailing pads -> (ids, lengths)."""
    out = np.full((len(lens), pmax + new), pad, dtype=np.int64)
    lengths = np.empty(len(lens), dtype=np.int64)
    for b, p in enumerate(lens):
        row = np.array(alone[b][0])
        lengths[b] = p + new
        if eos is not None:
            hit = np.nonzero(row[p:] == eos)[0]
            if hit.size:
                row[p + hit[0] + 1:] = pad
                lengths[b] = p + hit[0] + 1
        out[b, :p + new] = row
    return out, lengths


def ragged_case(seed, layout, b, h, tmax, d, dv, dtype):
    q, kc, vc, kn, vn = do.decode_inputs(np.random.RandomState(seed), layout, b, h, tmax, d, dv, dtype)
    return dict(q=q, k_cache=kc, v_cache=vc, k_new=kn, v_new=vn, layout=layout)


def poisoned_ragged(cache, layout, lens, dtype):
    """Rows from lens[b] on (the row about to be appended included) of every sequence b set to NaN."""
    out = np.array(cache, dtype=dtype)
    for b, n in enumerate(lens):
        n = min(max(int(n), 0), out.shape[1 if layout == "bthd" else 2])
        if layout == "bthd":
            out[b, n:] = np.nan
        else:
            out[b, :, n:] = np.nan
    return out


def run_ragged(route, case, lens, dtype, splits=None, unaligned=False):
    """One call on the whole batch -> (o, k_cache, v_cache) as numpy arrays, the caches AFTER the call."""
    layout = case["layout"]
    kd = dev(poisoned_ragged(case["k_cache"], layout, lens, dtype), dtype, unaligned)
    vd = dev(poisoned_ragged(case["v_cache"], layout, lens, dtype), dtype, unaligned)
    qd, kn, vn = (dev(case[n], dtype, unaligned) for n in ("q", "k_new", "v_new"))
    o = da.attention_decode_ragged(qd, kd, vd, da.lengths(lens), kn, vn, scale=case.get("scale"), layout=layout, route=route,
                                   splits=splits)
    return np.asarray(o), np.asarray(kd), np.asarray(vd)


def slice_case(case, b, length):
    """Sequence b alone, as a case of decode_support.run_decode / reference."""
    one = {n: np.ascontiguousarray(case[n][b:b + 1]) for n in ("q", "k_cache", "v_cache", "k_new", "v_new")}
    one.update(layout=case["layout"], length=int(length), scale=case.get("scale"))
    return one


def expected_ragged_caches(case, lens, dtype):
    """Bit for bit: row lens[b] of sequence b replaced by its new row, nothing else touched; an invalid length: untouched."""
    layout = case["layout"]
    kc, vc = (poisoned_ragged(case[n], layout, lens, dtype) for n in ("k_cache", "v_cache"))
    tmax = kc.shape[1 if layout == "bthd" else 2]
    for b, n in enumerate(lens):
        if 0 <= n < tmax:
            if layout == "bthd":
                kc[b, n], vc[b, n] = case["k_new"][b].astype(dtype), case["v_new"][b].astype(dtype)
            else:
                kc[b, :, n], vc[b, :, n] = case["k_new"][b].astype(dtype), case["v_new"][b].astype(dtype)
    return kc, vc
