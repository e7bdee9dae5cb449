"""Attention: the native kernels (csrc/tnn_attn.hip: one launch forward, two backward) vs the composed route (batched
products, max-subtract, exp, sum, divide on the generic kernels), forward and forward + backward, causal and not, in one
process, warmed, device-event timed over the same number of calls per side inside one fenced region, the two sides
alternating.  Every call takes the next of several operand sets (q, k, v, do: 4 x 16 MiB each; six sets are 384 MiB, more
than the 256 MiB last-level cache), so a call does not find its operands where its predecessor left them.

    python tools/probes/attn_ab.py [--repeats 7] [--inner 8] [--sets 6] [--out profiles/attn_vs_composed.txt]

Writes the table to --out (default: profiles/attn_vs_composed.txt of this checkout) and prints it.
"""

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np                                          # noqa: E402

import tinynn_autograd_amd as tn                            # noqa: E402
from tinynn_autograd_amd import _lib, attention             # noqa: E402
from tinynn_autograd_amd import device_array as da          # noqa: E402

PEAK_FLOPS = 157.3e12
B, H, T, D = 8, 8, 1024, 64


def timed(fn, inner):
    e0, e1 = _lib.Event(), _lib.Event()
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    _lib.synchronize()
    return e0.elapsed_ms(e1) * 1e3 / inner


def sides(causal, nsets):
    rs = np.random.RandomState(0)
    sets = [[tn.asarray(rs.standard_normal((B, H, T, D)).astype(np.float32)) for _ in range(4)] for _ in range(nsets)]
    turn = {"native": 0, "composed": 0}

    def fwd(route):
        def run():
            q, k, v, _ = sets[turn[route] % nsets]
            turn[route] += 1
            return da.attention(q, k, v, causal=causal, route=route)
        return run

    def fwd_bwd(route):
        def run():
            q, k, v, do = sets[turn[route] % nsets]
            turn[route] += 1
            o, lse = da.attention(q, k, v, causal=causal, route=route)
            _, delta = da.attention_bwd_q(q, k, v, o, do, lse, causal=causal, route=route)
            da.attention_bwd_kv(q, k, v, do, lse, delta, causal=causal, route=route)
        return run
    return fwd, fwd_bwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=8)
    ap.add_argument("--sets", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_vs_composed.txt"))
    args = ap.parse_args()
    assert tn.backend_name() != "cpu-twin(test only)"
    assert _lib.get().has_attn
    default = attention.plan_attention((B, H, T, D), (B, H, T, D), (B, H, T, D), native=True).route
    props = _lib.device_props()
    device = props["name"].strip() or "%d CUs" % props["cus"]
    set_mib = 4 * B * H * T * D * 4 / 2.0 ** 20
    lines = ["# device: %s; B %d, H %d, Tq = Tk = %d, D = Dv = %d, float32; per side %d repeats of %d calls over %d rotating "
             "operand sets (%.0f MiB each, %.0f MiB in all), device events, sides alternating; median (min..max) in us" % (
                 device, B, H, T, D, args.repeats, args.inner, args.sets, set_mib, set_mib * args.sets),
             "# TFLOP/s by the conventional count (4 B H T T D forward, 14 forward + backward: backward 10 with one recomputation "
             "of the scores; the two backward launches each rebuild them and execute 18 in all; half under the causal mask) and "
             "the fraction of the %.1f TFLOP/s fp32 MFMA peak are those of the native route" % (PEAK_FLOPS / 1e12),
             "%-10s %-8s %-9s %26s %26s %8s %9s %7s" % ("mask", "pass", "default", "native us", "composed us", "speedup",
                                                      "TFLOP/s", "of peak")]
    for causal in (False, True):
        fwd, fwd_bwd = sides(causal, args.sets)
        for label, make, mult in (("fwd", fwd, 4.0), ("fwd+bwd", fwd_bwd, 14.0)):
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
            flops = mult * B * H * T * T * D * (0.5 if causal else 1.0)
            tf = flops / (med["native"] * 1e-6) / 1e12
            lines.append("%-10s %-8s %-9s %26s %26s %7.1fx %9.3f %6.2f%%" % (
                "causal" if causal else "full", label, default, cell["native"], cell["composed"],
                med["composed"] / med["native"], tf, 100.0 * tf * 1e12 / PEAK_FLOPS))
            da.trim_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
