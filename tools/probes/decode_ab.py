"""Decode attention: tnn_decode_attn (csrc/tnn_decode.hip) against the route that existed before it — a sliced append of the new
row plus tnn_attn_fwd with Tq = 1, non-causal, striding into the same cache — in one process, warmed, device-event timed
inside one fenced region, the two legs alternating, float32, cache layout "bthd" with 8 heads (what generation.KVCache
allocates).  Shapes up to the 256 MiB last-level cache rotate over several operand sets that together exceed it; larger
ones exceed it alone.  The box's copy rate is measured in the same run (a device-to-device copy of 1 GiB, read + written
bytes per second) and each shape's bytes / time is put against it: bytes = B H len (D + Dv) 4, every live K and V element once.

    (a) B H x len x D: existing route vs tnn_decode_attn at the planner's split         (the yardstick is the parent's code)
    (b) a sweep of `splits` at three shapes — decoding.TARGET is taken from it
    (c) examples/charlm_run.py's model, untrained: generate() tokens/s with and without the cache, prompt 32, 224 new tokens

    python tools/probes/decode_ab.py [--repeats 5] [--inner 4] [--out profiles/decode_vs_fwd.txt] [--quick]
"""

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np                                          # noqa: E402

import tinynn_autograd_amd as tn                            # noqa: E402
from tinynn_autograd_amd import _lib, attention, decoding   # noqa: E402
from tinynn_autograd_amd import device_array as da          # noqa: E402

HEADS = 8
BH = (8, 64, 512)
LENS = (256, 4096, 32768)
DIMS = (64, 128)
SWEEP = ((8, 4096, 128), (8, 32768, 128), (64, 4096, 64))
CACHE_BYTES = 256 << 20


def timed(fn, inner):
    e0, e1 = _lib.Event(), _lib.Event()
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    _lib.synchronize()
    return e0.elapsed_ms(e1) * 1e3 / inner


def copy_rate():
    """Bytes read + written per second by a device-to-device copy of 1 GiB (median of 5 after a warm-up)."""
    src = tn.zeros((1 << 28,), np.float32)
    src.copy()
    _lib.synchronize()
    times = [timed(src.copy, 2) for _ in range(5)]
    return 2.0 * src.nbytes / (float(np.median(times)) * 1e-6)


def filled(shape, block):
    """A device array of `shape` whose rows repeat `block` [rows, D] (random): filled by device-to-device copies."""
    out = tn.zeros(shape, np.float32)
    flat = out.reshape(-1, shape[-1])
    n = block.shape[0]
    for start in range(0, flat.shape[0], n):
        stop = min(start + n, flat.shape[0])
        flat[start:stop] = block[:stop - start]
    return out


class Shape(object):
    """The operands of one (B H, len, D): `sets` caches with room for one more row, q / k_new / v_new, both legs."""

    def __init__(self, bh, length, d, rs):
        self.b, self.h, self.length, self.d = bh // HEADS, HEADS, length, d
        self.tmax = length + 1
        self.bytes = bh * length * 2 * d * 4
        nsets = 1 if self.bytes > CACHE_BYTES else CACHE_BYTES // self.bytes + 2
        block = tn.asarray(rs.standard_normal((1 << 14, d)).astype(np.float32))
        shape = (self.b, self.tmax, self.h, d)
        self.sets = [(filled(shape, block), filled(shape, block)) for _ in range(nsets)]
        one = lambda: tn.asarray(rs.standard_normal((self.b, self.h, d)).astype(np.float32))
        self.q, self.k_new, self.v_new = one(), one(), one()
        self.q4 = self.q.reshape(self.b, 1, self.h, d)
        self.turn = 0
        plan = attention.plan_attention((self.b, 1, self.h, d), shape, shape, False, None, "bthd")
        self.fwd_geometry = (self.b, self.h, 1, length + 1, d, d)
        self.fwd_strides = da._i64arr(plan.strides("q", "k", "v", "o"))
        self.scale = plan.scale
        self.nsets = nsets

    def caches(self):
        self.turn += 1
        return self.sets[self.turn % self.nsets]

    def existing(self):
        """The parent's code: two sliced assignments, then tnn_attn_fwd over the live prefix IN PLACE (strides of the cache)."""
        k, v = self.caches()
        k[:, self.length] = self.k_new
        v[:, self.length] = self.v_new
        out = da.DeviceArray._new((self.b, 1, self.h, self.d), np.float32)
        lse = da.DeviceArray._new((self.b, self.h, 1), np.float32)
        _lib.get().attn_fwd(self.q4._ptr, k._ptr, v._ptr, out._ptr, lse._ptr, *self.fwd_geometry, self.fwd_strides, self.scale,
                            0, out._code())
        return out

    def decode(self, splits=None):
        k, v = self.caches()
        return da.attention_decode(self.q, k, v, self.length, self.k_new, self.v_new, layout="bthd", route="native", splits=splits)


def alternate(legs, repeats, inner):
    for fn in legs.values():
        fn()
        fn()
    _lib.synchronize()
    t = {name: [] for name in legs}
    for _ in range(repeats):
        for name, fn in legs.items():
            t[name].append(timed(fn, inner))
    return t


def cell(values):
    return "%.1f (%.1f..%.1f)" % (float(np.median(values)), min(values), max(values))


def generation_rates(lines, prompt, new):
    """(c): the example's model, untrained (the token values do not change the work), batch 8."""
    import importlib.util
    path = os.path.join(ROOT, "tinynn-autograd_amd", "examples", "charlm_run.py")
    spec = importlib.util.spec_from_file_location("charlm_run_example", path)
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    from tinynn_autograd_amd.generation import generate
    args = example.parse(["--seq", str(prompt + new), "--vocab", "64", "--width", "128", "--heads", "4"])
    model, _ = example.build(args)
    ids = np.random.RandomState(0).randint(0, args.vocab, (8, prompt))
    for cache in (True, False):
        generate(model, ids, 8, temperature=0.0, cache=cache)                      # warm-up
        took = []
        for _ in range(3):
            _lib.synchronize()
            t0 = time.perf_counter()
            generate(model, ids, new, temperature=0.0, cache=cache)               # ends in its one read-back
            took.append(time.perf_counter() - t0)
        rate = [8 * new / t for t in took]
        lines.append("charlm     batch 8, prompt %d, %d new tokens, width 128, 2 blocks, cache=%-5s  %s tokens/s (wall clock, 3 runs)"
                     % (prompt, new, cache, cell(rate)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_vs_fwd.txt"))
    ap.add_argument("--quick", action="store_true", help="the smallest shape of every section only (a dry run of the probe)")
    args = ap.parse_args()
    assert tn.backend_name() != "cpu-twin(test only)"
    assert _lib.get().has_decode
    props = _lib.device_props()
    device = props["name"].strip() or "%d CUs" % props["cus"]
    rate = copy_rate()
    rs = np.random.RandomState(0)

    class Lines(list):
        """Every line goes to stdout and to the file as it is measured."""
        def append(self, line):
            list.append(self, line)
            print(line, flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    f.write("\n".join(self) + "\n")
    lines = Lines()
    for line in ["# device: %s; float32; layout bthd, %d heads; %d repeats of %d calls, device events, legs alternating; shapes up to "
             "%d MiB rotate over operand sets that exceed it in all; median (min..max) in us" % (device, HEADS, args.repeats, args.inner,
                                                                                              CACHE_BYTES >> 20),
             "# copy rate of this box, measured in this run (1 GiB device-to-device, read + written): %.2f TB/s; TB/s and the share "
             "of it are those of tnn_decode_attn (bytes: B H len (D + Dv) 4); TARGET = %d" % (rate / 1e12, decoding.TARGET),
             "# (a) existing = sliced append + tnn_attn_fwd with Tq = 1 striding into the cache; slower = decode's median exceeds the "
             "existing route's by more than the two legs' own spread (max - min)",
             "%-5s %-6s %-4s %-6s %28s %28s %9s %7s %8s %s" % ("B H", "len", "D", "splits", "existing us", "decode us", "speedup", "TB/s",
                                                             "of copy", "")]:
        lines.append(line)
    shapes = [(bh, n, d) for bh in BH for n in LENS for d in DIMS]
    if args.quick:
        shapes = shapes[:1]
    worst = []
    for bh, n, d in shapes:
        s = Shape(bh, n, d, rs)
        plan = decoding.plan_decode((s.b, s.h, d), (s.b, s.tmax, s.h, d), (s.b, s.tmax, s.h, d), n)
        if s.b * s.tmax * s.h * d >= 1 << 31:                   # tnn_attn_fwd refuses a tensor of 2^31 elements or more
            t = alternate({"decode": s.decode}, args.repeats, args.inner)
            m = float(np.median(t["decode"]))
            lines.append("%-5d %-6d %-4d %-6d %28s %28s %9s %7.2f %7.1f%% %s" % (
                bh, n, d, plan.splits, "refused: 2^31 elements", cell(t["decode"]), "", s.bytes / (m * 1e-6) / 1e12,
                100.0 * s.bytes / (m * 1e-6) / rate, ""))
            del s
            da.trim_cache()
            continue
        t = alternate({"existing": s.existing, "decode": s.decode}, args.repeats, args.inner)
        med = {k: float(np.median(v)) for k, v in t.items()}
        spread = max(max(v) - min(v) for v in t.values())
        slower = med["decode"] > med["existing"] + spread
        worst.append(slower)
        got = s.bytes / (med["decode"] * 1e-6)
        lines.append("%-5d %-6d %-4d %-6d %28s %28s %8.1fx %7.2f %7.1f%% %s" % (
            bh, n, d, plan.splits, cell(t["existing"]), cell(t["decode"]), med["existing"] / med["decode"], got / 1e12,
            100.0 * got / rate, "SLOWER" if slower else ""))
        del s
        da.trim_cache()
    lines.append("# shapes at which tnn_decode_attn is slower than the existing route beyond the spread: %d of %d" % (sum(worst), len(worst)))
    lines.append("# (b) sweep of `splits` (workgroups = B H x splits); us, median (min..max)")
    for bh, n, d in (SWEEP[:1] if args.quick else SWEEP):
        s = Shape(bh, n, d, rs)
        chunks = -(-(n + 1) // decoding.CHUNK)
        options = [x for x in (1, 2, 4, 8, 16, 32, 64, 128, 256) if x <= min(chunks, decoding.MAX_SPLITS)]
        legs = {x: (lambda x=x: s.decode(x)) for x in options}
        t = alternate(legs, args.repeats, args.inner)
        best = min(float(np.median(v)) for v in t.values())
        for x in options:
            m = float(np.median(t[x]))
            lines.append("sweep B H %-4d len %-6d D %-4d splits %-4d workgroups %-6d %26s  %.2fx the best" % (
                bh, n, d, x, bh * x, cell(t[x]), m / best))
        del s, legs
        da.trim_cache()
    lines.append("# (c) generation")
    generation_rates(lines, 32, 8 if args.quick else 224)


if __name__ == "__main__":
    main()
