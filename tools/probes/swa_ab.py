"""Sliding-window causal attention (window=, csrc/tnn_swa.hip) against full causal attention on the same operands, in one
process, warmed, device-event timed, the legs alternating (the helpers of tools/probes/decode_ab.py):

    (a) band against triangle   forward alone and forward + backward (dq, dk, dv) at B x T x H x D, microseconds per call,
                                the ratio causal / window and the ratio of visited 64 x 64 blocks (swa.visited_blocks): the
                                time is expected to follow the blocks

(The staging table of profiles/swa_vs_full.txt was taken once with a build of the register-prefetch variant of the forward
loop next to the library; that variant lost and is not kept, so the table is not reproduced here.)

    python tools/probes/swa_ab.py [--repeats 5] [--inner 20] [--out profiles/swa_vs_full.txt]
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
from tinynn_autograd_amd import _lib, swa                   # noqa: E402
from tinynn_autograd_amd import device_array as da          # noqa: E402

B, H, D = 2, 16, 128
LENGTHS = (2048, 8192)
WINDOWS = (256, 1024)
GROUPS = (1, 4)


def operands(T, group, rs):
    make = lambda h: tn.asarray(rs.standard_normal((B, T, h, D)).astype(np.float32))
    return make(H), make(H // group), make(H // group), make(H)


def legs(q, k, v, do_, group, window):
    """(forward, forward + backward) of one setting; window None: the causal kernels."""
    if group == 1:
        opts = dict(causal=True, layout="bthd", route="native", window=window)
        fwd, bwd_q, bwd_kv = da.attention, da.attention_bwd_q, da.attention_bwd_kv
    else:
        opts = dict(causal=True, route="native", window=window)
        fwd, bwd_q, bwd_kv = da.gqa_attention, da.gqa_attention_bwd_q, da.gqa_attention_bwd_kv

    def both():
        o, lse = fwd(q, k, v, **opts)
        dq, delta = bwd_q(q, k, v, o, do_, lse, **opts)
        bwd_kv(q, k, v, do_, lse, delta, **opts)
    return (lambda: fwd(q, k, v, **opts)), both


def band_table(lines, repeats, inner, rs):
    lines += ["(a) window against causal, B %d H %d D %d, us per call: median (min..max) of %d repeats of %d calls" % (B, H, D, repeats, inner),
              "T      W     group  blocks band/causal  fwd causal           fwd window           ratio  fwd+bwd causal       fwd+bwd window       ratio"]
    slower = []
    for T in LENGTHS:
        for group in GROUPS:
            q, k, v, do_ = operands(T, group, rs)
            for W in WINDOWS:
                cf, cb = legs(q, k, v, do_, group, None)
                wf, wb = legs(q, k, v, do_, group, W)
                t = ab.alternate({"cf": cf, "wf": wf, "cb": cb, "wb": wb}, repeats, inner)
                band, tri = swa.visited_blocks(T, W)
                rf, rb = np.median(t["cf"]) / np.median(t["wf"]), np.median(t["cb"]) / np.median(t["wb"])
                lines.append("%-6d %-5d %-6d %5d / %-5d      %-20s %-20s %-6.2f %-20s %-20s %.2f" % (
                    T, W, group, band, tri, ab.cell(t["cf"]), ab.cell(t["wf"]), rf, ab.cell(t["cb"]), ab.cell(t["wb"]), rb))
                if rf < 1.0 or rb < 1.0:
                    slower.append((T, W, group))
            del q, k, v, do_
            da.trim_cache()
    lines += ["", "shapes at which the window is slower than causal: %s" % (slower or "none"), ""]


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--repeats", default=5, type=int)
    parser.add_argument("--inner", default=20, type=int)
    parser.add_argument("--out", default=None)
    args = parser.parse_args()
    assert _lib.get().has_swa and tn.backend_name() == "hip-gfx950", "the probe measures libtnn_hip.so on the GPU"
    rs = np.random.RandomState(0)
    lines = ["# tools/probes/swa_ab.py on %s" % _lib.device_props()["name"], ""]
    band_table(lines, args.repeats, args.inner, rs)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
