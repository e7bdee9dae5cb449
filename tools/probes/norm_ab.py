"""Layer norm and RMS norm: the native kernels (csrc/tnn_norm.hip: one launch forward, one call backward) vs the composed route
(sums, products and a square root on the generic kernels), forward and forward + backward, in one process, warmed,
device-event timed over the same number of calls per side inside one fenced region, the two sides alternating.  Every call
takes the next of several operand sets (x and dy), which together exceed the 256 MiB last-level cache, so a call does not
find its operands where its predecessor left them.

    python tools/probes/norm_ab.py [--repeats 7] [--inner 8] [--out profiles/norm_vs_composed.txt]

Writes the table to --out (default: profiles/norm_vs_composed.txt of this checkout) and prints it.  The bytes of the native
route are the ones it must move: x and y forward (2 M N), x, dy and dx backward (3 M N); the row statistics, gamma, beta and
the partial rows of the parameter gradients come on top and are not counted.
"""

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np                                          # noqa: E402

import tinynn_autograd_amd as tn                            # noqa: E402
from tinynn_autograd_amd import _lib, norm                  # noqa: E402
from tinynn_autograd_amd import device_array as da          # noqa: E402

COPY_RATE = 6.29e12                  # bytes / s of a device copy kernel on this part (measured, micro-architecture notes)
SHAPES = ((8192, 1024), (8192, 4096), (32768, 768))
CACHE_BYTES = 256 << 20


def timed(fn, inner):
    e0, e1 = _lib.Event(), _lib.Event()
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    _lib.synchronize()
    return e0.elapsed_ms(e1) * 1e3 / inner


def sides(kind, m, n, nsets):
    rs = np.random.RandomState(0)
    host = rs.standard_normal((m, n)).astype(np.float32)
    sets = [[tn.asarray(np.roll(host, s + 1, axis=0)), tn.asarray(np.roll(host, -s - 1, axis=0))] for s in range(nsets)]
    gamma = tn.asarray((1.0 + 0.1 * rs.standard_normal(n)).astype(np.float32))
    beta = tn.asarray((0.1 * rs.standard_normal(n)).astype(np.float32)) if kind == "layer" else None
    turn = {"native": 0, "composed": 0}

    def forward(x, route):
        if kind == "layer":
            return da.layer_norm(x, gamma, beta, route=route)
        y, rstd = da.rms_norm(x, gamma, route=route)
        return y, None, rstd

    def fwd(route):
        def run():
            x, _ = sets[turn[route] % nsets]
            turn[route] += 1
            return forward(x, route)
        return run

    def fwd_bwd(route):
        def run():
            x, dy = sets[turn[route] % nsets]
            turn[route] += 1
            _, mean, rstd = forward(x, route)
            return da.norm_bwd(x, dy, gamma, mean, rstd, kind=kind, route=route)
        return run
    return fwd, fwd_bwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "norm_vs_composed.txt"))
    args = ap.parse_args()
    assert tn.backend_name() != "cpu-twin(test only)"
    assert _lib.get().has_norm
    props = _lib.device_props()
    device = props["name"].strip() or "%d CUs" % props["cus"]
    lines = ["# device: %s; float32, gamma (and beta) present; per side %d repeats of %d calls over rotating operand sets (x, dy) "
             "that exceed %d MiB in all, device events, sides alternating; median (min..max) in us" % (
                 device, args.repeats, args.inner, CACHE_BYTES >> 20),
             "# bytes: 2 M N forward, 5 M N forward + backward, 4 bytes each; TB/s and the fraction of the %.2f TB/s copy rate "
             "are those of the native route" % (COPY_RATE / 1e12),
             "%-6s %-14s %-6s %-8s %24s %26s %8s %7s %8s" % ("kind", "shape", "form", "pass", "native us", "composed us",
                                                            "speedup", "TB/s", "of copy")]
    for kind in norm.KINDS:
        for m, n in SHAPES:
            plan = norm.plan_norm((m, n), (n,), (n,) if kind == "layer" else None, kind=kind, native=True)
            assert plan.route == "native"
            nsets = max(2, -(-CACHE_BYTES // (2 * m * n * 4)) + 1)
            fwd, fwd_bwd = sides(kind, m, n, nsets)
            for label, make, mult in (("fwd", fwd, 2), ("fwd+bwd", fwd_bwd, 5)):
                nat, com = make("native"), make("composed")
                for fn in (nat, com):
                    for _ in range(2):
                        fn()
                _lib.synchronize()
                t = {"native": [], "composed": []}
                for _ in range(args.repeats):
                    t["native"].append(timed(nat, args.inner))
                    t["composed"].append(timed(com, args.inner))
                med = {k: float(np.median(v)) for k, v in t.items()}
                cell = {k: "%.1f (%.1f..%.1f)" % (med[k], min(v), max(v)) for k, v in t.items()}
                rate = mult * m * n * 4 / (med["native"] * 1e-6)
                lines.append("%-6s %-14s %-6s %-8s %24s %26s %7.1fx %7.2f %7.1f%%" % (
                    kind, "[%d, %d]" % (m, n), plan.form, label, cell["native"], cell["composed"],
                    med["composed"] / med["native"], rate / 1e12, 100.0 * rate / COPY_RATE))
            del fwd, fwd_bwd, nat, com
            da.trim_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
