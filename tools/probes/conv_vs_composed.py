"""Convolution: the native kernels (csrc/tnn_conv.hip, one launch per product) vs the composed route (a loop over the filter
taps on the generic kernels), per layer shape, forward and backward (dx + dw + db), in one process, warmed, device-event
timed over many calls inside one fenced region, the two sides alternating.  Also the route conv.py takes by itself.

    python tools/probes/conv_vs_composed.py [--repeats 5] [--inner 10] [--out profiles/conv_vs_composed.txt] [--once]

--once: one un-timed native forward + backward per shape (for a kernel trace: three kernels per shape).
"""

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np                                          # noqa: E402

import tinynn_autograd_amd as tn                            # noqa: E402
from tinynn_autograd_amd import _lib, conv                  # noqa: E402
from tinynn_autograd_amd import device_array as da          # noqa: E402

PEAK_FLOPS = 157.3e12

# name, x shape, w shape, stride, padding
SHAPES = [
    ("lenet conv1 batch 128", (128, 1, 28, 28), (6, 1, 5, 5), 1, 2),
    ("lenet conv2 batch 128", (128, 6, 14, 14), (16, 6, 5, 5), 1, 0),
    ("lenet conv1 batch 1024", (1024, 1, 28, 28), (6, 1, 5, 5), 1, 2),
    ("lenet conv2 batch 1024", (1024, 6, 14, 14), (16, 6, 5, 5), 1, 0),
    ("wide 64->128 3x3 56x56 batch 32", (32, 64, 56, 56), (128, 64, 3, 3), 1, 1),
]


def timed(fn, inner):
    e0, e1 = _lib.Event(), _lib.Event()
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    _lib.synchronize()
    return e0.elapsed_ms(e1) * 1e3 / inner


def sides(xs, ws, stride, padding):
    rs = np.random.RandomState(0)
    plan = conv.plan_conv2d(xs, ws, stride=stride, padding=padding, native=True)
    x = tn.asarray(rs.standard_normal(xs).astype(np.float32))
    w = tn.asarray(rs.standard_normal(ws).astype(np.float32))
    b = tn.asarray(rs.standard_normal(ws[0]).astype(np.float32))
    dy = tn.asarray(rs.standard_normal(plan.out_shape).astype(np.float32))

    def fwd(route):
        return lambda: da.conv2d(x, w, b, stride, padding, route=route)

    def bwd(route):
        def run():
            da.conv2d_bwd_data(dy, w, xs, stride, padding, route=route)
            da.conv2d_bwd_filter(x, dy, ws, stride, padding, route=route)
        return run
    flops = 2.0 * plan.N * plan.OH * plan.OW * plan.F * plan.C * plan.KH * plan.KW
    return plan, fwd, bwd, flops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    assert tn.backend_name() != "cpu-twin(test only)"
    assert _lib.get().has_conv
    if args.once:
        for name, xs, ws, stride, padding in SHAPES:
            _, fwd, bwd, _ = sides(xs, ws, stride, padding)
            fwd("native")()
            bwd("native")()
        _lib.synchronize()
        print("one native forward + backward per shape issued (%d shapes)" % len(SHAPES))
        return
    lines = ["# device: %s; %d repeats of %d calls, device events, sides alternating; median (min..max) in us" %
             (_lib.device_props()["name"], args.repeats, args.inner),
             "# TFLOP/s and the fraction of the %.1f TFLOP/s fp32 MFMA peak are those of the native route; backward = dx + dw + db "
             "(twice the forward's multiply-adds)" % (PEAK_FLOPS / 1e12),
             "%-34s %-5s %-9s %24s %24s %8s %9s %7s" % ("shape", "pass", "default", "native us", "composed us", "speedup",
                                                     "TFLOP/s", "of peak")]
    for name, xs, ws, stride, padding in SHAPES:
        plan, fwd, bwd, flops = sides(xs, ws, stride, padding)
        for label, make, fl in (("fwd", fwd, flops), ("bwd", bwd, 2 * flops)):
            nat, com = make("native"), make("composed")
            for fn in (nat, com):
                fn()
            _lib.synchronize()
            t = {"native": [], "composed": []}
            for _ in range(args.repeats):
                t["native"].append(timed(nat, args.inner))
                t["composed"].append(timed(com, max(1, args.inner // 5)))
            med = {k: float(np.median(v)) for k, v in t.items()}
            cell = {k: "%.1f (%.1f..%.1f)" % (med[k], min(v), max(v)) for k, v in t.items()}
            tf = fl / (med["native"] * 1e-6) / 1e12
            lines.append("%-34s %-5s %-9s %24s %24s %7.1fx %9.3f %6.2f%%" % (
                name, label, plan.route, cell["native"], cell["composed"], med["composed"] / med["native"], tf,
                100.0 * tf * 1e12 / PEAK_FLOPS))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
