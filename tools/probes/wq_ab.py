"""The int8 weight-only linear layer against the float32 ops.dense_ of the same shape, in one process, warmed, device-event
timed, the legs alternating (the pattern and the helpers of tools/probes/decode_ab.py):

    (a) linear     ops.dense_wq_ (tnn_wq_linear, the planner's splits) against ops.dense_ (the float32 GEMM with the bias
                   epilogue) at M x (K, N); microseconds per call, the fraction of 8 TB/s the K N code bytes reach, the ratio
                   float / int8.  Weights up to the 256 MiB last-level cache rotate over sets that together exceed it.
    (b) splits     tnn_wq_linear at M = 1 over the split counts: what wq.choose_splits is tuned from
    (c) generation tokens/s of examples/charlm_run.py's model, captured, with float32 and with int8 weights, and the largest
                   difference of the first decoding step's logits between the two

    python tools/probes/wq_ab.py [--repeats 5] [--inner 8] [--out profiles/wq_vs_float.txt] [--quick]
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

import decode_ab as ab                                      # noqa: E402  (timed, alternate, cell)
import tinynn_autograd_amd as tn                            # noqa: E402
from tinynn_autograd_amd import _lib, wq                    # noqa: E402
from tinynn_autograd_amd import device_array as da          # noqa: E402
from tinynn_autograd_amd.core import ops                    # noqa: E402

ROWS = (1, 2, 4, 8, 16)
SHAPES = ((512, 512), (4096, 4096), (4096, 16384), (4096, 32000))
PEAK = 8e12                                                 # bytes per second the fractions refer to


class Weight(object):
    """Float32 weights [K, N] and their codes, as many sets as it takes to exceed the last-level cache."""

    def __init__(self, k, n, rs):
        self.k, self.n, self.turn = k, n, 0
        sets = lambda nbytes: 1 if nbytes > ab.CACHE_BYTES else min(ab.CACHE_BYTES // nbytes + 2, 64)
        block = tn.asarray((rs.standard_normal((k, n)) * 0.02).astype(np.float32))
        self.floats = [tn.Tensor(block.copy()) for _ in range(sets(4 * k * n))]
        codes, scales = da.wq_quantize(block)
        self.int8 = [(codes.copy(), scales.copy()) for _ in range(sets(k * n))]
        self.b = tn.Tensor(tn.zeros((1, n), np.float32))

    def run_float(self, x):
        self.turn += 1
        return ops.dense_(x, self.floats[self.turn % len(self.floats)], self.b)

    def run_int8(self, x, splits=None):
        self.turn += 1
        return ops.dense_wq_(x, self.int8[self.turn % len(self.int8)], self.b, route="native", splits=splits)


def linear_table(lines, repeats, inner, quick):
    lines.append("(a) linear: us per call, median (min..max) of %d x %d calls; int8: share of %.0f TB/s the K N code bytes reach"
                 % (repeats, inner, PEAK * 1e-12))
    lines.append("%3s %6s %6s %6s | %-24s | %-24s %-7s | %s" % ("M", "K", "N", "splits", "float32 us", "int8 us", "of peak", "f32/int8"))
    rs = np.random.RandomState(0)
    slower = []
    for k, n in SHAPES:
        if quick and (k, n) not in SHAPES[:2]:
            continue
        w = Weight(k, n, rs)
        for m in ROWS:
            x = tn.Tensor(tn.asarray(rs.standard_normal((m, k)).astype(np.float32)))
            t = ab.alternate({"float": lambda: w.run_float(x), "int8": lambda: w.run_int8(x)}, repeats, inner)
            f, i = float(np.median(t["float"])), float(np.median(t["int8"]))
            if i > f:
                slower.append((m, k, n))
            lines.append("%3d %6d %6d %6d | %-24s | %-24s %-7s | %.2fx%s" % (
                m, k, n, wq.choose_splits(m, k, n), ab.cell(t["float"]), ab.cell(t["int8"]), "%.1f%%" % (100.0 * k * n / (i * 1e-6) / PEAK),
                f / i, "   SLOWER than float32" if i > f else ""))
        del w
        da.trim_cache()
    lines.append("slower than float32 (M, K, N): %s" % (slower or "none"))


def splits_table(lines, repeats, inner):
    lines.append("")
    lines.append("(b) splits: tnn_wq_linear at M = 1, us per call over the workgroups per column panel")
    rs = np.random.RandomState(1)
    for k, n in SHAPES[:3]:
        w = Weight(k, n, rs)
        x = tn.Tensor(tn.asarray(rs.standard_normal((1, k)).astype(np.float32)))
        counts = [s for s in (1, 2, 4, 8, 16, 32, 64) if s <= wq.most_splits(k)]
        t = ab.alternate({s: (lambda s=s: w.run_int8(x, s)) for s in counts}, repeats, inner)
        lines.append("K %d N %d (chosen %d): %s" % (k, n, wq.choose_splits(1, k, n),
                                                    ", ".join("%d: %.1f" % (s, float(np.median(t[s]))) for s in counts)))
        del w
        da.trim_cache()


def generation_rates(lines, prompt, new):
    lines.append("")
    lines.append("(c) generation: examples/charlm_run.py's model (untrained), batch 8, prompt %d, %d new tokens, width 128, 4 heads, "
                 "2 blocks, captured; tokens/s, wall clock, 3 runs" % (prompt, new))
    spec = importlib.util.spec_from_file_location("charlm_run_example", os.path.join(ROOT, "tinynn-autograd_amd", "examples",
                                                                                     "charlm_run.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    from tinynn_autograd_amd import generation as gen
    model, _ = example.build(example.parse(["--seq", str(prompt + new), "--vocab", "64", "--width", "128", "--heads", "4"]))
    ids = np.random.RandomState(0).randint(0, 64, (8, prompt))
    gen.generate(model, ids, 8, temperature=0.0, capture=True)
    qw = gen.quantize_weights(model, "int8")
    lines.append("quantized %d weights, %d of %d bytes; kept float: %s" % ((len(qw.quantized),) + qw.nbytes() + (qw.kept or "none",)))
    for weights in (None, qw):
        gen.generate(model, ids, 8, temperature=0.0, capture=True, weights=weights)
        took = []
        for _ in range(3):
            _lib.synchronize()
            t0 = time.perf_counter()
            gen.generate(model, ids, new, temperature=0.0, capture=True, weights=weights)
            took.append(time.perf_counter() - t0)
        lines.append("weights %-8s %s tokens/s" % ("int8" if weights else "float32", ab.cell([8 * new / t for t in took])))

    def first_step_logits(table):
        cache = gen.KVCache(prompt + 1)
        model.set_phase("TEST")
        ops.WQ_ACTIVE = table
        try:
            gen._forward(model.net.layers, tn.Tensor(ids), 0, cache)
            return np.asarray(gen._forward(model.net.layers, tn.Tensor(ids[:, :1]), prompt, cache).values, dtype=np.float64)
        finally:
            ops.WQ_ACTIVE = None
            model.set_phase("TRAIN")

    f, q = first_step_logits(None), first_step_logits(qw.activate())
    lines.append("first decoding step: max |logit_int8 - logit_f32| %.3e (largest |logit_f32| %.3e)" % (np.abs(q - f).max(), np.abs(f).max()))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--repeats", default=5, type=int)
    parser.add_argument("--inner", default=8, type=int)
    parser.add_argument("--out", default=None)
    parser.add_argument("--quick", action="store_true", help="the two smaller weights only")
    args = parser.parse_args()
    assert _lib.get().has_wq and tn.backend_name() == "hip-gfx950", "the probe measures libtnn_hip.so on the GPU"
    lines = ["# tools/probes/wq_ab.py on %s" % _lib.device_props()["name"], ""]
    linear_table(lines, args.repeats, args.inner, args.quick)
    splits_table(lines, args.repeats, args.inner)
    generation_rates(lines, 32, 224)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
