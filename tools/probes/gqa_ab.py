"""Grouped-query attention against the expanded multi-head form, in one process, warmed, device-event timed, the legs
alternating (the pattern of tools/probes/decode_ab.py, whose helpers it uses), float32, layout "bthd":

    (a) decode     tnn_gqa_decode_attn on caches of Hkv heads against tnn_decode_attn — unchanged from before the grouped
                   kernels existed — on the SAME q with the caches expanded to H heads; B H x len x D of DESIGN §4d's table at
                   group 2, 4 and 8; microseconds and TB/s of live bytes for both (live bytes: B Hkv len (D + Dv) 4 grouped,
                   B H len (D + Dv) 4 expanded).  Shapes up to the 256 MiB last-level cache rotate over operand sets that
                   together exceed it.
    (b) training   tnn_gqa_bwd_kv against tnn_attn_bwd_kv on expanded operands plus the sum over the group axis
    (c) generation tokens/s of examples/charlm_run.py's model (§4d(c): batch 8, prompt 32, 224 new tokens, width 128,
                   4 heads), cache=True, with and without --kv-heads

    python tools/probes/gqa_ab.py [--repeats 5] [--inner 4] [--out profiles/gqa_vs_expanded.txt] [--quick | --subset]

--host-path LABEL prints instead the wall time per call of the six training entry points of device_array (plain and grouped) at
a shape where the launch is negligible and the Python path dominates, one line per entry point, and nothing else: run it once
per process from the two trees to compare, alternating (profiles/attn_host_path.txt).
"""

import argparse
import importlib.util
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np                                          # noqa: E402

import decode_ab as ab                                      # noqa: E402  (timed, alternate, cell, filled, copy_rate)
import tinynn_autograd_amd as tn                            # noqa: E402
from tinynn_autograd_amd import _lib, gqa                   # noqa: E402
from tinynn_autograd_amd import device_array as da          # noqa: E402

HEADS = ab.HEADS
GROUPS = (2, 4, 8)
TRAIN = ((4, 8, 1024, 64), (4, 8, 2048, 128))               # B, H, T, D: causal self-attention


class DecodeShape(object):
    """The operands of one (B H, len, D, group): caches of H heads (expanded) and of H / group heads (grouped), one q."""

    def __init__(self, bh, length, d, group, rs):
        self.b, self.h, self.hkv, self.length, self.d = bh // HEADS, HEADS, HEADS // group, length, d
        tmax = length + 1
        self.bytes_expanded = bh * length * 2 * d * 4
        self.bytes_grouped = self.bytes_expanded // group
        block = tn.asarray(rs.standard_normal((1 << 14, d)).astype(np.float32))
        sets = lambda nbytes: 1 if nbytes > ab.CACHE_BYTES else ab.CACHE_BYTES // nbytes + 2
        big, small = (self.b, tmax, self.h, d), (self.b, tmax, self.hkv, d)
        self.expanded = [(ab.filled(big, block), ab.filled(big, block)) for _ in range(sets(self.bytes_expanded))]
        self.grouped = [(ab.filled(small, block), ab.filled(small, block)) for _ in range(sets(self.bytes_grouped))]
        one = lambda heads: tn.asarray(rs.standard_normal((self.b, heads, d)).astype(np.float32))
        self.q, self.new_e, self.new_g = one(self.h), (one(self.h), one(self.h)), (one(self.hkv), one(self.hkv))
        self.turn = 0

    def run_expanded(self):
        self.turn += 1
        k, v = self.expanded[self.turn % len(self.expanded)]
        return da.attention_decode(self.q, k, v, self.length, *self.new_e, layout="bthd", route="native")

    def run_grouped(self):
        self.turn += 1
        k, v = self.grouped[self.turn % len(self.grouped)]
        return da.gqa_decode(self.q, k, v, self.length, *self.new_g, layout="bthd", route="native")


def training_legs(b, h, t, d, group, rs):
    hkv = h // group
    arr = lambda heads, amp=1.0: tn.asarray((rs.standard_normal((b, t, heads, d)) * amp).astype(np.float32))
    q, k, v, g = arr(h), arr(hkv), arr(hkv), arr(h)
    ke, ve = da._gqa_expand(k, group), da._gqa_expand(v, group)
    o, lse = da.gqa_attention(q, k, v, True, route="native")
    _, delta = da.gqa_attention_bwd_q(q, k, v, o, g, lse, True, route="native", need_dq=False)

    def grouped():
        return da.gqa_attention_bwd_kv(q, k, v, g, lse, delta, True, route="native")

    def expanded():
        dk, dv = da.attention_bwd_kv(q, ke, ve, g, lse, delta, True, None, "bthd", "native")
        return dk.reshape(b, t, hkv, group, d).sum(axis=3), dv.reshape(b, t, hkv, group, d).sum(axis=3)
    return {"expanded": expanded, "grouped": grouped}


HOST_SHAPE = (2, 6, 2, 9, 12, 5, 7)          # B, H, Hkv, Tq, Tk, D, Dv of tests/test_attn_host_paths.py


def host_path(label, batches=9, calls=2000, warm=500):
    """us per call, native route, float32, causal: `warm` calls, then `batches` times `calls` calls back to back with one
    synchronise at the end of each; the plain form runs H heads of k and v, the grouped one Hkv."""
    b, h, hkv, tq, tk, d, dv = HOST_SHAPE
    rs = np.random.RandomState(0)
    arr = lambda *shape: tn.asarray(rs.standard_normal(shape).astype(np.float32))
    q, g = arr(b, tq, h, d), arr(b, tq, h, dv)
    for name, heads, fwd, bwd_q, bwd_kv, layout in (
            ("attention", h, da.attention, da.attention_bwd_q, da.attention_bwd_kv, {"layout": "bthd"}),
            ("gqa_attention", hkv, da.gqa_attention, da.gqa_attention_bwd_q, da.gqa_attention_bwd_kv, {})):
        k, v = arr(b, tk, heads, d), arr(b, tk, heads, dv)
        opts = dict(layout, causal=True, route="native")
        o, lse = fwd(q, k, v, **opts)
        _, delta = bwd_q(q, k, v, o, g, lse, need_dq=False, **opts)
        for leg, fn in ((name, lambda: fwd(q, k, v, **opts)), (name + "_bwd_q", lambda: bwd_q(q, k, v, o, g, lse, **opts)),
                        (name + "_bwd_kv", lambda: bwd_kv(q, k, v, g, lse, delta, **opts))):
            for _ in range(warm):
                fn()
            took = []
            for _ in range(batches):
                _lib.synchronize()
                t0 = time.perf_counter()
                for _ in range(calls):
                    fn()
                _lib.synchronize()
                took.append((time.perf_counter() - t0) / calls * 1e6)
            print("%-7s %-24s us per call: %s  median %.3f" % (label, leg, " ".join("%.3f" % t for t in took),
                                                              float(np.median(took))), flush=True)


def generation_rates(lines, prompt, new):
    path = os.path.join(ROOT, "tinynn-autograd_amd", "examples", "charlm_run.py")
    spec = importlib.util.spec_from_file_location("charlm_run_example", path)
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    from tinynn_autograd_amd.generation import generate
    for kv in (None, 2, 1):
        argv = ["--seq", str(prompt + new), "--vocab", "64", "--width", "128", "--heads", "4"]
        args = example.parse(argv + (["--kv-heads", str(kv)] if kv else []))
        model, _ = example.build(args)
        ids = np.random.RandomState(0).randint(0, args.vocab, (8, prompt))
        generate(model, ids, 8, temperature=0.0, cache=True)                       # warm-up
        took = []
        for _ in range(3):
            _lib.synchronize()
            t0 = time.perf_counter()
            generate(model, ids, new, temperature=0.0, cache=True)
            took.append(time.perf_counter() - t0)
        lines.append("charlm     batch 8, prompt %d, %d new tokens, width 128, 4 heads, 2 blocks, cache=True, kv_heads=%-4s  %s tokens/s "
                     "(wall clock, 3 runs)" % (prompt, new, kv, ab.cell([8 * new / t for t in took])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gqa_vs_expanded.txt"))
    ap.add_argument("--quick", action="store_true", help="the smallest shape of every section only (a dry run of the probe)")
    ap.add_argument("--subset", action="store_true", help="B H 8 and 64, len 4096 and 32768, D 128 only (a shorter table)")
    ap.add_argument("--host-path", metavar="LABEL", help="only the host time per call of the six training entry points")
    args = ap.parse_args()
    assert tn.backend_name() != "cpu-twin(test only)"
    assert _lib.get().has_gqa and _lib.get().has_decode
    if args.host_path:
        return host_path(args.host_path)
    props = _lib.device_props()
    device = props["name"].strip() or "%d CUs" % props["cus"]
    rate = ab.copy_rate()
    rs = np.random.RandomState(0)

    class Lines(list):
        def append(self, line):
            list.append(self, line)
            print(line, flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    f.write("\n".join(self) + "\n")
    lines = Lines()
    for line in ["# device: %s; float32; layout bthd, %d query heads; %d repeats of %d calls, device events, legs alternating; median "
                 "(min..max) in us" % (device, HEADS, args.repeats, args.inner),
                 "# copy rate of this box, measured in this run (1 GiB device-to-device, read + written): %.2f TB/s" % (rate / 1e12),
                 "# (a) decode: expanded = tnn_decode_attn on caches of %d heads; grouped = tnn_gqa_decode_attn on caches of %d / group "
                 "heads; TB/s of each leg's own live bytes; SLOWER: grouped's median exceeds expanded's by more than the spread" % (HEADS, HEADS),
                 "%-5s %-6s %-4s %-5s %-6s %26s %26s %8s %8s %8s %8s %s" % ("B H", "len", "D", "group", "splits", "expanded us",
                                                                          "grouped us", "speedup", "1/group", "exp TB/s", "grp TB/s", "")]:
        lines.append(line)
    shapes = [(bh, n, d) for bh in ab.BH for n in ab.LENS for d in ab.DIMS]
    if args.subset:
        shapes = [(bh, n, 128) for bh in (8, 64) for n in (4096, 32768)]
    if args.quick:
        shapes = shapes[:1]
    lost = 0
    for bh, n, d in shapes:
        for group in (GROUPS[:1] if args.quick else GROUPS):
            s = DecodeShape(bh, n, d, group, rs)
            plan = gqa.plan_gqa_decode((s.b, s.h, d), (s.b, n + 1, s.hkv, d), (s.b, n + 1, s.hkv, d), n)
            t = ab.alternate({"expanded": s.run_expanded, "grouped": s.run_grouped}, args.repeats, args.inner)
            med = {k: float(np.median(v)) for k, v in t.items()}
            spread = max(max(v) - min(v) for v in t.values())
            slower = med["grouped"] > med["expanded"] + spread
            lost += slower
            lines.append("%-5d %-6d %-4d %-5d %-6d %26s %26s %7.2fx %7.2fx %8.2f %8.2f %s" % (
                bh, n, d, group, plan.splits, ab.cell(t["expanded"]), ab.cell(t["grouped"]), med["expanded"] / med["grouped"],
                float(group), s.bytes_expanded / (med["expanded"] * 1e-6) / 1e12, s.bytes_grouped / (med["grouped"] * 1e-6) / 1e12,
                "SLOWER" if slower else ""))
            del s
            da.trim_cache()
    lines.append("# cells at which the grouped call is slower than the expanded one beyond the spread: %d" % lost)
    lines.append("# (b) training, causal, Tq = Tk = T: expanded = tnn_attn_bwd_kv on k, v repeated over the group + the sum over the "
                 "group axis; grouped = tnn_gqa_bwd_kv")
    for b, h, t_, d in (TRAIN[:1] if args.quick else TRAIN):
        for group in (GROUPS[:1] if args.quick else GROUPS):
            t = ab.alternate(training_legs(b, h, t_, d, group, rs), args.repeats, args.inner)
            med = {k: float(np.median(v)) for k, v in t.items()}
            lines.append("bwd_kv B %d H %d T %-5d D %-4d group %d  expanded %26s  grouped %26s  %.2fx" % (
                b, h, t_, d, group, ab.cell(t["expanded"]), ab.cell(t["grouped"]), med["expanded"] / med["grouped"]))
            da.trim_cache()
    lines.append("# (c) generation")
    generation_rates(lines, 32, 8 if args.quick else 224)


if __name__ == "__main__":
    main()
