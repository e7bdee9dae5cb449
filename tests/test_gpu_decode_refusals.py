"""The host checks of the four decode attention entry points (tnn_decode_attn, tnn_ragged_decode_attn, tnn_gqa_decode_attn,
tnn_gqa_ragged_decode_attn) and of the two workspace entry points, called raw, past the planners: ONE table of calls, each with
the FULL message the library must leave — every rule in the order the source makes it, a call that breaks two rules reporting
the earlier one, and an empty batch passing with its operands unseen.  No row reaches a launch.  The shapes are those of
test_the_library_refuses_what_the_planner_refuses (B 1, H 1 — grouped: H 2 over Hkv 1 —, Tmax 8, D = Dv = 4, float32); the
rows about the workspace claim a cache of 128 rows, the fewest that allow two splits."""

import ctypes

import numpy as np
import pytest

import tinynn_autograd_amd as tn
from tinynn_autograd_amd import _lib, device_array as da

pytestmark = pytest.mark.gpu

ENTRIES = {                      # name -> (ragged, grouped)
    "tnn_decode_attn": (False, False),
    "tnn_ragged_decode_attn": (True, False),
    "tnn_gqa_decode_attn": (False, True),
    "tnn_gqa_ragged_decode_attn": (True, True),
}
POINTERS = ("q", "k_new", "v_new", "k_cache", "v_cache", "o", "workspace", "lens", "strides")
BASE = dict(workspace=None, workspace_bytes=0, B=1, H=1, Hkv=1, len=3, Tmax=8, D=4, Dv=4, scale=0.5, splits=1, dtype=0)
TWO_SPLITS = dict(Tmax=128, len=64, splits=2)          # 65 keys (ragged: a cache of 128 rows): 2 chunks of 64


def table(name):
    """(id, what the call changes, the message after the entry point's name — None: the call succeeds)."""
    ragged, grouped = ENTRIES[name]
    heads = "Hkv" if grouped else "H"
    extents = "B %%d, %s 1, D %%d, Dv %%d (B %s < 65536, 1 <= D, Dv <= 128)" % (heads, heads)
    chunks = "(a cache of 1 chunks of 64 keys)" if ragged else "(1 chunks of 64 keys)"
    need = 96 if grouped else 48                               # round16(B H splits (Dv + 2) 4)
    rows = []
    if grouped:
        rows += [("H 0 over Hkv 1", dict(H=0), "H 0 query heads over Hkv 1 key / value heads"),
                 ("H 3 over Hkv 2", dict(H=3, Hkv=2), "H 3 is no multiple of Hkv 2"),
                 ("group 9", dict(H=9), "group 9 = H 9 / Hkv 1 exceeds TNN_GQA_MAX_GROUP = 8")]
    rows += [("dtype", dict(dtype=2), "dtype 2 (float32 and float64 only)"),
             ("D 0", dict(D=0), extents % (1, 0, 4)),
             ("D 129", dict(D=129), extents % (1, 129, 4)),
             ("Dv 129", dict(Dv=129), extents % (1, 4, 129)),
             ("65536 rows", dict(B=65536), extents % (65536, 4, 4))]
    if ragged:
        rows += [("no k_new", dict(k_new=None), "k_new and v_new are required (the step appends its row)"),
                 ("Tmax 0", dict(Tmax=0), "a cache of 0 rows")]
    else:
        rows += [("k_new without v_new", dict(v_new=None), "k_new and v_new come together or not at all"),
                 ("full cache", dict(len=8), "len 8 with a cache of 8 rows (the appended row needs len < Tmax)"),
                 ("len 0, no append", dict(len=0, k_new=None, v_new=None),
                  "len 0 with a cache of 8 rows (without k_new / v_new: 1 <= len <= Tmax)"),
                 ("len > Tmax", dict(len=9), "len 9 with a cache of 8 rows (the appended row needs len < Tmax)"),
                 ("Tmax 0", dict(len=0, Tmax=0), "len 0 with a cache of 0 rows (the appended row needs len < Tmax)")]
    rows += [("splits 0", dict(splits=0), "splits 0 outside [1, 1] " + chunks),
             ("splits most + 1", dict(splits=2), "splits 2 outside [1, 1] " + chunks),
             ("null q", dict(q=None), "null operand")]
    if ragged:
        rows += [("null lens", dict(lens=None), "null operand")]
    rows += [("null workspace", dict(TWO_SPLITS, workspace_bytes=need),
              "workspace of %d bytes, %d needed (16-byte aligned)" % (need, need)),
             ("workspace one byte short", dict(TWO_SPLITS, workspace="ws", workspace_bytes=need - 1),
              "workspace of %d bytes, %d needed (16-byte aligned)" % (need - 1, need))]
    # two rules broken: the earlier one speaks
    if grouped:
        rows += [("group before dtype", dict(H=9, dtype=2), "group 9 = H 9 / Hkv 1 exceeds TNN_GQA_MAX_GROUP = 8")]
    else:
        rows += [("dtype before extents", dict(dtype=2, D=0), "dtype 2 (float32 and float64 only)")]
    if ragged:
        rows += [("append before splits", dict(v_new=None, splits=0), "k_new and v_new are required (the step appends its row)")]
    else:
        rows += [("append before splits", dict(len=8, splits=0), "len 8 with a cache of 8 rows (the appended row needs len < Tmax)")]
    rows += [("splits before null", dict(splits=0, q=None), "splits 0 outside [1, 1] " + chunks)]
    # an empty batch: nothing is looked at (the ragged forms ask for k_new and v_new before they know)
    empty = dict.fromkeys(POINTERS if not ragged else [p for p in POINTERS if p not in ("k_new", "v_new")])
    rows += [("B 0, null operands", dict(empty, B=0), None)]
    return [(name, i, change, msg) for i, change, msg in rows]


ROWS = [row for name in ENTRIES for row in table(name)]


@pytest.fixture(scope="module")
def operands():
    """Caches of 128 rows behind the claimed 8: the two-split rows stay inside them whatever the library does."""
    q, k, v, o = (tn.zeros(s, np.float32) for s in ((1, 2, 4), (1, 128, 1, 4), (1, 128, 1, 4), (1, 2, 4)))
    keep = dict(q=q, k_new=q, v_new=q, k_cache=k, v_cache=v, o=o, ws=tn.zeros((64,), np.float32),
                lens=tn.asarray(np.array([3], dtype=np.int64)))
    ptrs = {n: a._ptr for n, a in keep.items()}
    ptrs["strides"] = da._i64arr((8, 4, 0) + (4, 4, 0) * 2 + (512, 4, 4) * 2 + (8, 4, 0))
    return keep, ptrs


@pytest.mark.parametrize("name,what,change,msg", ROWS, ids=["%s: %s" % (r[0][4:], r[1]) for r in ROWS])
def test_a_raw_call_is_refused_with_the_full_message(operands, name, what, change, msg):
    ragged, grouped = ENTRIES[name]
    _, ptrs = operands
    a = dict(BASE, **{p: p for p in POINTERS if p != "workspace"})
    if grouped:
        a["H"] = 2
    a.update(change)
    p = {n: (None if a[n] is None else ptrs[a[n]]) for n in POINTERS}
    heads = (a["H"], a["Hkv"]) if grouped else (a["H"],)
    args = (p["q"], p["k_new"], p["v_new"], p["k_cache"], p["v_cache"], p["o"], p["workspace"], a["workspace_bytes"])
    args += ((p["lens"], a["B"]) + heads if ragged else (a["B"],) + heads + (a["len"],))
    args += (a["Tmax"], a["D"], a["Dv"], p["strides"], a["scale"], a["splits"], a["dtype"])
    call = getattr(_lib.get(), name[4:])
    if msg is None:
        assert call(*args) is None
        return
    with pytest.raises(_lib.TnnError) as err:
        call(*args)
    assert str(err.value) == "%s failed (rc=2): %s: %s" % (name, name, msg)


@pytest.mark.parametrize("name", ["tnn_decode_attn_workspace", "tnn_gqa_decode_workspace"])
def test_the_workspace_entry_points(name):
    call = getattr(_lib.get(), name[4:])
    size = ctypes.c_int64(-1)
    for args, msg in (((1, 2, 2, 4, 0, None), "null result pointer"),
                      ((1, 2, 2, 4, 2, size), "dtype 2 (float32 and float64 only)"),
                      ((1, 2, 2, 129, 0, size), "B 1, H 2, Dv 129, splits 2 (Dv <= 128, splits <= 256)"),
                      ((1, 2, 257, 4, 0, size), "B 1, H 2, Dv 4, splits 257 (Dv <= 128, splits <= 256)")):
        with pytest.raises(_lib.TnnError) as err:
            call(*args[:5], None if args[5] is None else ctypes.byref(args[5]))
        assert str(err.value) == "%s failed (rc=2): %s: %s" % (name, name, msg)
    assert size.value == -1
    call(1, 2, 2, 4, 0, ctypes.byref(size))
    assert size.value == 96                                    # round16(1 2 2 (4 + 2) 4)
    call(3, 2, 1, 4, 1, ctypes.byref(size))
    assert size.value == 0                                     # one split: no records
