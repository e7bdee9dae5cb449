"""The fused linear + cross-entropy (ops.linear_cross_entropy_, csrc/tnn_lce.hip) against ops.dense_ + ops.cross_entropy_ at
the same shapes, in one process, warmed, device-event timed, the legs alternating (the helpers of tools/probes/decode_ab.py):

    (a) time and memory   forward alone and forward + backward (dh, dw, db) of both routes at M x K x V; microseconds per
                          call, the ratio composed / fused, and the pool bytes one forward + backward leaves behind on a
                          trimmed pool (live + cached: what the step held at once, the logits and their gradient included)
    (b) splits            tnn_lce_fwd over the split counts: what lce.choose_splits is to be tuned from
    (c) chunk bytes       forward + backward over lce.CHUNK_BYTES: what that constant is to be tuned from

    python tools/probes/lce_ab.py [--repeats 3] [--inner 2] [--out profiles/lce_vs_composed.txt] [--quick]
"""

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np                                          # noqa: E402

import decode_ab as ab                                      # noqa: E402  (timed, alternate, cell)
import tinynn_autograd_amd as tn                            # noqa: E402
from tinynn_autograd_amd import _lib, lce                   # noqa: E402
from tinynn_autograd_amd import device_array as da          # noqa: E402
from tinynn_autograd_amd.core import ops                    # noqa: E402

ROWS = (2048, 8192)
WIDTHS = (512, 1024, 4096)
VOCABS = (4096, 32768, 131072)


class Head(object):
    def __init__(self, m, k, v, rs):
        self.m, self.k, self.v = m, k, v
        self.h = tn.Tensor(tn.asarray(rs.standard_normal((m, k)).astype(np.float32)), requires_grad=True)
        self.w = tn.Tensor(ab.filled((k, v), tn.asarray((rs.standard_normal((64, v)) * 0.02).astype(np.float32))), requires_grad=True)
        self.b = tn.Tensor(tn.zeros((1, v), np.float32), requires_grad=True)
        self.t = tn.asarray(rs.randint(0, v, m).astype(np.int64))

    def loss(self, route):
        return ops.linear_cross_entropy_(self.h, self.w, self.b, self.t, route=route)

    def step(self, route):
        for p in (self.h, self.w, self.b):
            p.zero_grad()
        self.loss(route).backward()

    def held(self, route):
        """Pool bytes one forward + backward leaves on a trimmed pool, less what was live before it."""
        for p in (self.h, self.w, self.b):
            p.zero_grad()
        da.trim_cache()
        before = _lib.pool_stats()
        self.step(route)
        _lib.synchronize()
        after = _lib.pool_stats()
        return after["live_bytes"] + after["cached_bytes"] - before["live_bytes"] - before["cached_bytes"]


def main_table(lines, repeats, inner, quick):
    lines.append("(a) us per call, median (min..max) of %d x %d calls; held: MiB of pool one forward + backward leaves behind" % (repeats, inner))
    lines.append("%5s %5s %7s %3s %5s | %-26s %-26s %-6s | %-28s %-28s %-6s | %9s %9s" % (
        "M", "K", "V", "spl", "chunk", "fwd fused", "fwd composed", "c / f", "fwd+bwd fused", "fwd+bwd composed", "c / f",
        "held f", "held c"))
    rs = np.random.RandomState(0)
    slower = []
    for m in ROWS:
        for k in WIDTHS:
            for v in VOCABS:
                if quick and m * v > 2048 * 32768:
                    continue
                head = Head(m, k, v, rs)
                f = ab.alternate({r: (lambda r=r: head.loss(r)) for r in ("native", "composed")}, repeats, inner)
                s = ab.alternate({r: (lambda r=r: head.step(r)) for r in ("native", "composed")}, repeats, inner)
                med = lambda t, r: float(np.median(t[r]))
                if med(s, "native") > med(s, "composed"):
                    slower.append((m, k, v))
                lines.append("%5d %5d %7d %3d %5d | %-26s %-26s %-6s | %-28s %-28s %-6s | %9.1f %9.1f" % (
                    m, k, v, lce.choose_splits(m, v), lce.choose_chunk_rows(m, v), ab.cell(f["native"]), ab.cell(f["composed"]),
                    "%.2fx" % (med(f, "composed") / med(f, "native")), ab.cell(s["native"]), ab.cell(s["composed"]),
                    "%.2fx" % (med(s, "composed") / med(s, "native")), head.held("native") / 2.0 ** 20, head.held("composed") / 2.0 ** 20))
                del head
                da.trim_cache()
    lines.append("forward + backward slower than composed (M, K, V): %s" % (slower or "none"))


def sweeps(lines, repeats, inner):
    rs = np.random.RandomState(1)
    lines += ["", "(b) splits: tnn_lce_fwd through ops.linear_cross_entropy_, us per call over the split counts"]
    for m, k, v in ((2048, 1024, 32768), (8192, 1024, 32768), (2048, 1024, 4096)):
        head = Head(m, k, v, rs)
        counts = [s for s in (1, 2, 4, 8, 16, 32, 64) if s <= lce.most_splits(v)]
        run = lambda s: da.linear_cross_entropy(head.h.values, head.w.values, head.b.values, head.t, route="native", splits=s)
        t = ab.alternate({s: (lambda s=s: run(s)) for s in counts}, repeats, inner)
        lines.append("M %d K %d V %d (chosen %d): %s" % (m, k, v, lce.choose_splits(m, v),
                                                         ", ".join("%d: %.1f" % (s, float(np.median(t[s]))) for s in counts)))
        del head
        da.trim_cache()
    lines += ["", "(c) chunk bytes: forward + backward, us per call over the chunk buffer's size (rows per chunk)"]
    for m, k, v in ((8192, 1024, 32768), (8192, 1024, 131072)):
        head = Head(m, k, v, rs)
        sizes = [mb << 20 for mb in (16, 64, 256, 1024)]
        rows = {b: lce.choose_chunk_rows(m, v, b) for b in sizes}

        def step(b):
            for p in (head.h, head.w, head.b):
                p.zero_grad()
            ops.linear_cross_entropy_(head.h, head.w, head.b, head.t, route="native", chunk_rows=rows[b]).backward()
        t = ab.alternate({b: (lambda b=b: step(b)) for b in sizes}, repeats, inner)
        lines.append("M %d K %d V %d: %s" % (m, k, v, ", ".join("%d MiB (%d rows): %.1f" % (b >> 20, rows[b], float(np.median(t[b])))
                                                                  for b in sizes)))
        del head
        da.trim_cache()


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--repeats", default=3, type=int)
    parser.add_argument("--inner", default=2, type=int)
    parser.add_argument("--out", default=None)
    parser.add_argument("--quick", action="store_true", help="shapes up to M V = 2048 x 32768 only")
    args = parser.parse_args()
    assert _lib.get().has_lce and tn.backend_name() == "hip-gfx950", "the probe measures libtnn_hip.so on the GPU"
    lines = ["# tools/probes/lce_ab.py on %s" % _lib.device_props()["name"], ""]
    main_table(lines, args.repeats, args.inner, args.quick)
    sweeps(lines, args.repeats, args.inner)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
