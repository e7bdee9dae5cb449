"""Batched matmul: one tnn_gemm_batched launch vs a Python loop of the 2-D `@` over the batch elements (the only way to get
the result before the batched kernel existed), per shape, in one process, warmed, device-event timed, the two sides
alternating.  Also the route the dispatcher takes by itself and its time.

    python tools/probes/bmm_vs_loop.py [--repeats 7] [--inner 20] [--out profiles/bmm_vs_loop.txt] [--once]

--once: one un-timed pass over every shape through the batched route (for a kernel trace: one kernel per call).
"""

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np                                          # noqa: E402

import tinynn_autograd_amd as tn                            # noqa: E402
from tinynn_autograd_amd import _lib, batching              # noqa: E402
from tinynn_autograd_amd import device_array as da          # noqa: E402

PEAK_FLOPS, PEAK_BYTES = 157.3e12, 8.0e12

# name, a shape, b shape, swap_a (the dW form)
SHAPES = [
    ("1000x(4x4.4x4)", (1000, 4, 4), (1000, 4, 4), False),
    ("512x(32x32.32x32)", (512, 32, 32), (512, 32, 32), False),
    ("64x(128x64.64x128)", (64, 128, 64), (64, 64, 128), False),
    ("64x(128x128.128x64)", (64, 128, 128), (64, 128, 64), False),
    ("8x(512x512.512x512)", (8, 512, 512), (8, 512, 512), False),
    ("4x(1024x1024.1024x1024)", (4, 1024, 1024), (4, 1024, 1024), False),
    ("2x(2048x2048.2048x2048)", (2, 2048, 2048), (2, 2048, 2048), False),
    ("32x(128x256).(256x256)", (32, 128, 256), (256, 256), False),
    ("dW of 32x(128x256).(256x256)", (32, 128, 256), (32, 128, 256), True),
]


def timed(fn, inner):
    e0, e1 = _lib.Event(), _lib.Event()
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    _lib.synchronize()
    return e0.elapsed_ms(e1) * 1e3 / inner


def sides(name, sa, sb, swap_a):
    rs = np.random.RandomState(0)
    a = tn.asarray(rs.standard_normal(sa).astype(np.float32))
    b = tn.asarray(rs.standard_normal(sb).astype(np.float32))
    if swap_a:
        # dW of X[..., M, K] @ W: what core/ops.py does (one long-K TN GEMM) vs the per-element X[i].T @ G[i] summed
        K, N = sa[-1], sb[-1]

        def chosen():
            return a.reshape(-1, K).T @ b.reshape(-1, N)

        def batched():
            da.BMM_ROUTE = "batched"
            try:
                return da.matmul(a, b, swap_a=True).sum(axis=0)
            finally:
                da.BMM_ROUTE = None

        def loop():
            acc = a[0].T @ b[0]
            for i in range(1, sa[0]):
                acc = acc + a[i].T @ b[i]
            return acc

        route = "gemm2d (TN, K = %d)" % (sa[0] * sa[1])
        flops = 2.0 * sa[0] * sa[1] * K * N
        nbytes = 4.0 * (a.size + b.size + K * N)
        return chosen, batched, loop, route, flops, nbytes
    plan = batching.plan_matmul(sa, sb, native=True)

    def chosen():
        return a @ b

    def batched():
        da.BMM_ROUTE = "batched"
        try:
            return a @ b
        finally:
            da.BMM_ROUTE = None

    def loop():
        if len(sb) == 2:
            return [a[i] @ b for i in range(sa[0])]
        return [a[i] @ b[i] for i in range(sa[0])]

    M, K, N = sa[-2], sa[-1], sb[-1]
    flops = 2.0 * sa[0] * M * K * N
    nbytes = 4.0 * (a.size + b.size + sa[0] * M * N)
    return chosen, batched, loop, plan.route, flops, nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    assert tn.backend_name() != "cpu-twin(test only)"
    _lib.get()
    lines = []
    if args.once:
        for name, sa, sb, swap_a in SHAPES[:-2]:
            _, batched, _, _, _, _ = sides(name, sa, sb, swap_a)
            batched()
        _lib.synchronize()
        print("one batched call per shape issued (%d calls)" % len(SHAPES[:-2]))
        return
    head = "%-30s %-22s %12s %12s %12s %9s %9s  %s" % ("shape", "route", "chosen us", "batched us", "loop us",
                                                       "TFLOP/s", "GB/s", "bound")
    lines.append("# device: %s; %d repeats of %d calls, device events, sides alternating; min..max over the repeats" %
                 (_lib.device_props()["name"], args.repeats, args.inner))
    lines.append(head)
    for name, sa, sb, swap_a in SHAPES:
        chosen, batched, loop, route, flops, nbytes = sides(name, sa, sb, swap_a)
        inner = max(2, args.inner // 4) if sa[0] >= 512 else args.inner
        for fn in (chosen, batched, loop):
            fn()
            fn()
        _lib.synchronize()
        t = {"chosen": [], "batched": [], "loop": []}
        for _ in range(args.repeats):
            t["chosen"].append(timed(chosen, inner))
            t["batched"].append(timed(batched, inner))
            t["loop"].append(timed(loop, inner))
        med = {k: float(np.median(v)) for k, v in t.items()}
        spread = {k: "%.1f..%.1f" % (min(v), max(v)) for k, v in t.items()}
        sec = med["chosen"] * 1e-6
        tf, gb = flops / sec / 1e12, nbytes / sec / 1e9
        t_mfma, t_hbm = flops / PEAK_FLOPS, nbytes / PEAK_BYTES
        bound = "launch latency" if sec > 20 * max(t_mfma, t_hbm) else ("MFMA" if t_mfma > t_hbm else "HBM")
        lines.append("%-30s %-22s %12.1f %12.1f %12.1f %9.3f %9.1f  %s" % (name, route, med["chosen"], med["batched"],
                                                                        med["loop"], tf, gb, bound))
        lines.append("%-30s %-22s %12s %12s %12s" % ("", "  (min..max)", spread["chosen"], spread["batched"], spread["loop"]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
