"""Dropout: the native kernels (csrc/tnn_dropout.hip: a one-thread ticket launch and one data launch) vs the composed route (a
host-drawn mask, an upload, the generic multiply / select / add), plain and fused-residual forms, float32, in one process,
warmed.  The native side is device-event timed over `--inner` calls inside one fenced region; every call takes the next of
several operand sets, which together exceed the 256 MiB last-level cache, so a call does not find its operands where its
predecessor left them.  The composed side synchronises by design (it reads the generator's state and draws on the host), so it
is timed by the wall clock per call, host work included — that IS its cost.

    python tools/probes/dropout_ab.py [--repeats 7] [--inner 8] [--out profiles/dropout_vs_composed.txt]

Writes the table to --out (default: profiles/dropout_vs_composed.txt of this checkout) and prints it.  Bytes of the native
route: x and y (2 n) plain and backward, x, residual and y (3 n) fused, 4 bytes each.  The ticket launch is timed twice: alone
(tnn_rng_uniform over zero elements launches nothing else) and as the difference between forward (ticket + data) and backward
(data only), which move the same bytes.
"""

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np                                          # noqa: E402

import tinynn_autograd_amd as tn                            # noqa: E402
from tinynn_autograd_amd import _lib, rng                   # noqa: E402
from tinynn_autograd_amd import device_array as da          # noqa: E402

COPY_RATE = 6.29e12                  # bytes / s of a device copy kernel on this part (measured, micro-architecture notes)
SIZES = (1 << 16, 1 << 20, 1 << 24)
CACHE_BYTES = 256 << 20
P = 0.1


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
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dropout_vs_composed.txt"))
    args = ap.parse_args()
    assert tn.backend_name() != "cpu-twin(test only)"
    lib = _lib.get()
    assert lib.has_dropout
    props = _lib.device_props()
    device = props["name"].strip() or "%d CUs" % props["cus"]
    gen = rng.Generator(1)
    state = gen.device_state()
    ticket = da.DeviceArray._new((2,), np.int64)

    def ticket_only():
        lib.rng_uniform(state._ptr, ticket._ptr, None, 0, 0, _lib.F32)
    for _ in range(4):
        ticket_only()
    alone = [timed(ticket_only, 64) for _ in range(args.repeats)]

    lines = ["# device: %s; float32, p = %.2f; native: %d repeats of %d calls over rotating operand sets that exceed %d MiB in all, "
             "device events; composed: wall clock per synchronised call (host draw and upload included), %d calls; median "
             "(min..max) in us" % (device, P, args.repeats, args.inner, CACHE_BYTES >> 20, args.repeats),
             "# bytes: 2 n plain and backward, 3 n fused residual, 4 bytes each; TB/s and the fraction of the %.2f TB/s copy rate "
             "are those of the native route" % (COPY_RATE / 1e12),
             "# the one-thread ticket launch alone (back to back, 64 per region): %s us" % cell(alone),
             "%-10s %-9s %24s %30s %9s %7s %8s" % ("n", "form", "native us", "composed us", "speedup", "TB/s", "of copy")]
    slower = []
    for n in SIZES:
        nsets = max(2, -(-CACHE_BYTES // (2 * n * 4)) + 1)
        host = np.random.RandomState(0).standard_normal(n).astype(np.float32)
        sets = [(tn.asarray(np.roll(host, s + 1)), tn.asarray(np.roll(host, -s - 1))) for s in range(nsets)]
        out = da.DeviceArray._new((n,), np.float32)
        turn = [0]

        def operands():
            turn[0] += 1
            return sets[turn[0] % nsets]

        def plain(route):
            def run():
                x, _ = operands()
                return da.dropout(x, P, generator=gen, route=route, out=out if route == "native" else None)
            return run

        def fused(route):
            def run():
                x, r = operands()
                return da.dropout(x, P, r, generator=gen, route=route, out=out if route == "native" else None)
            return run

        _, mask = da.dropout(sets[0][0], P, generator=gen, route="native")

        def backward():
            x, _ = operands()
            return da.dropout_bwd(x, mask, dx_out=out)

        med = {}
        for label, make, mult in (("plain", plain, 2), ("residual", fused, 3), ("backward", None, 2)):
            nat = backward if make is None else make("native")
            for _ in range(2):
                nat()
            t_nat = [timed(nat, args.inner) for _ in range(args.repeats)]
            med[label] = float(np.median(t_nat))
            rate = mult * n * 4 / (med[label] * 1e-6)
            if make is None:
                com_cell, speed = "(the same launches as plain)", ""
            else:
                com = make("composed")
                com()
                t_com = [wall(com) for _ in range(args.repeats)]
                ratio = float(np.median(t_com)) / med[label]
                com_cell, speed = cell(t_com), "%.1fx" % ratio
                if ratio < 1.0:
                    slower.append("n = %d %s" % (n, label))
            lines.append("%-10d %-9s %24s %30s %9s %7.2f %7.1f%%" % (n, label, cell(t_nat), com_cell, speed, rate / 1e12,
                                                                  100.0 * rate / COPY_RATE))
        lines.append("#   n = %d: forward (ticket + data) - backward (data only) = %.1f us" % (n, med["plain"] - med["backward"]))
        del sets, out, mask
        da.trim_cache()
    lines.append("# native slower than composed at: %s" % (", ".join(slower) if slower else "no size measured here"))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
