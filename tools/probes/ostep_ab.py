"""The device-resident optimizer step (csrc/tnn_ostep.hip) against the existing Adam launch, float32, in one process, warmed.

    python tools/probes/ostep_ab.py [--repeats 9] [--inner 8] [--out profiles/ostep_vs_adam.txt]

Per size n it records
  * tnn_adam_ex with advance = 0 (the update launch alone, 28 n bytes) and tnn_ostep_adamw (the update launch alone, the same
    28 n bytes, plus the run lookup) on the SAME arrays, alternating within every repeat, device-event timed over `--inner`
    calls inside one fenced region;
  * the whole clipped step: tnn_ostep_sumsq + tnn_ostep_begin + tnn_ostep_adamw (4 n more bytes for the norm);
  * the composed route (AdamW(fused=False): DeviceArray arithmetic, the norm read back), by the wall clock per synchronised
    call — the read-back IS its cost.
Every call takes the next of several operand sets which together exceed the 256 MiB last-level cache, so a call does not find
its operands where its predecessor left them (at 2^26 elements one set is 1 GiB and needs no rotation).  The run table has 16
runs, what one transformer block gives.  Writes the table to --out and prints it.
"""

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np                                          # noqa: E402

import tinynn_autograd_amd as tn                            # noqa: E402
from tinynn_autograd_amd import _lib, ostep                 # noqa: E402
from tinynn_autograd_amd import device_array as da          # noqa: E402
from tinynn_autograd_amd.core.optimizer import AdamW        # noqa: E402

PEAK = 8.0e12                        # bytes / s, the part's HBM peak
SIZES = (1 << 20, 1 << 24, 1 << 26)
CACHE_BYTES = 256 << 20
LR, B1, B2, EPS, WD = 1e-3, 0.9, 0.999, 1e-8, 0.01
RUNS = 16


def timed(fn, inner):
    e0, e1 = _lib.Event(), _lib.Event()
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    _lib.synchronize()
    return e0.elapsed_ms(e1) * 1e3 / inner


def wall(fn):
    _lib.synchronize()
    t0 = time.perf_counter()
    fn()
    _lib.synchronize()
    return (time.perf_counter() - t0) * 1e6


def cell(values):
    return "%.1f (%.1f..%.1f)" % (float(np.median(values)), min(values), max(values))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=8)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ostep_vs_adam.txt"))
    args = ap.parse_args()
    assert tn.backend_name() != "cpu-twin(test only)"
    lib = _lib.get()
    assert lib.has_ostep
    props = _lib.device_props()
    device = props["name"].strip() or "%d CUs" % props["cus"]
    lines = ["# device: %s; float32; %d repeats of %d calls (adam_ex and adamw alternate within a repeat), rotating operand sets "
             "that exceed %d MiB in all, device events; composed: wall clock per synchronised call; median (min..max) in us"
             % (device, args.repeats, args.inner, CACHE_BYTES >> 20),
             "# bytes of an update launch: 28 n (read p g m v, write p m v); TB/s and the share of the %.0f TB/s HBM peak are "
             "those of tnn_ostep_adamw; %d decay runs" % (PEAK / 1e12, RUNS),
             "%-10s %22s %22s %7s %6s %8s %24s %28s" % ("n", "tnn_adam_ex us", "tnn_ostep_adamw us", "ratio", "TB/s", "of peak",
                                                      "clipped step (a+b+c) us", "composed step us")]
    for n in args.sizes:
        nsets = max(1, -(-CACHE_BYTES // (16 * n)) + 1) if 16 * n <= 2 * CACHE_BYTES else 1
        rs = np.random.RandomState(0)
        host_g = (rs.uniform(0.1, 1.0, n) * np.where(rs.rand(n) < 0.5, -1.0, 1.0)).astype(np.float32)
        host_p = rs.standard_normal(n).astype(np.float32)
        sets = [tuple(tn.asarray(a) for a in (np.roll(host_p, s), np.roll(host_g, s), np.zeros(n, np.float32), np.zeros(n, np.float32)))
                for s in range(nsets)]
        pows = tn.asarray(np.array([B1 ** 3, B2 ** 3, 0.0, 0.0]), dtype=np.float64)
        st = ostep.initial_state(LR)
        st[ostep.T], st[ostep.B1_POW], st[ostep.B2_POW] = 3, B1 ** 3, B2 ** 3
        rec = tn.asarray(st, dtype=np.float64)
        ws = tn.empty((ostep.grid(n),), np.float64)
        cuts = [(i * n) // RUNS for i in range(RUNS)] + [n]
        starts, flags = ostep.decay_runs([(a, b - a) for a, b in zip(cuts[:-1], cuts[1:])], [i % 2 == 0 for i in range(RUNS)])
        table = tn.asarray(ostep.run_table(starts, flags), dtype=np.int64)
        turn = [0]

        def operands():
            turn[0] += 1
            return sets[turn[0] % nsets]

        def adam_ex():
            p, g, m, v = operands()
            lib.adam_ex(p._ptr, g._ptr, m._ptr, v._ptr, n, LR, B1, B2, EPS, pows._ptr, None, _lib.F32, 0, None, None)

        def adamw():
            p, g, m, v = operands()
            lib.ostep_adamw(p._ptr, g._ptr, m._ptr, v._ptr, None, n, rec._ptr, table._ptr, len(starts), B1, B2, EPS, WD, _lib.F32)

        def clipped():
            p, g, m, v = operands()
            lib.ostep_sumsq(g._ptr, n, ws._ptr, ws.nbytes, _lib.F32)
            lib.ostep_begin(rec._ptr, ws._ptr, n, 1.0, 1, B1, B2, ostep.SCHED_COSINE, LR, 0.0, 100, 1000000)
            lib.ostep_adamw(p._ptr, g._ptr, m._ptr, v._ptr, None, n, rec._ptr, table._ptr, len(starts), B1, B2, EPS, WD, _lib.F32)

        for fn in (adam_ex, adamw, clipped):
            for _ in range(2):
                fn()
        t_adam, t_adamw = [], []
        for _ in range(args.repeats):
            t_adam.append(timed(adam_ex, args.inner))
            t_adamw.append(timed(adamw, args.inner))
        t_clip = [timed(clipped, args.inner) for _ in range(args.repeats)]

        opt = AdamW(lr=LR, weight_decay=WD, max_norm=1.0, schedule=ostep.Cosine(100, 1000000), fused=False)
        opt.bind_layout([(a, b - a, i, None, "w" if i % 2 == 0 else "b") for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:]))])

        def composed():
            p, g, _m, _v = sets[0]
            opt.apply_flat(p, g)
        composed()
        t_com = [wall(composed) for _ in range(max(3, args.repeats // 3))]

        med_a, med_w = float(np.median(t_adam)), float(np.median(t_adamw))
        rate = 28.0 * n / (med_w * 1e-6)
        lines.append("%-10d %22s %22s %6.3fx %6.2f %7.1f%% %24s %28s" % (n, cell(t_adam), cell(t_adamw), med_w / med_a, rate / 1e12,
                                                                         100.0 * rate / PEAK, cell(t_clip), cell(t_com)))
        del sets, opt, ws, table
        da.trim_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
