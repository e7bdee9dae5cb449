"""Training attention with per-sequence lengths: the three tnn_varlen_* launches (csrc/tnn_varlen.hip; forward, dq + delta,
dk + dv) against the three tnn_attn_* launches on the same padded operands, in one process, warmed, device-event timed, the
legs alternating (the helpers of decode_ab.py), float32, causal, layout "bthd", batch 8 x 8 heads.

    (a) full lengths     every lens[b] = T: what reading the lengths costs where they skip nothing.  The margin is the
                         baseline's own max - min over its medians of this run; "loses" marks a median beyond it.
    (b) random lengths   lens uniform with a mean fill of 25 / 50 / 75 % of T (drawn once per shape, seed 0), against the padded
                         causal launch, which computes the right live rows and wastes the rest.  Next to the ratio: the share
                         of live 64 x 64 score blocks (varlen.live_blocks), which is what the ratio can at best follow.
    (c) the model        examples/charlm_run.py's model (width 128, 4 heads, 2 blocks, untrained), batch 8 x 1024 tokens,
                         --ragged-train batches: live tokens/s of a training step with and without lens.

    python tools/probes/varlen_ab.py [--repeats 5] [--inner 3] [--out profiles/varlen_vs_padded.txt] [--quick]
"""

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np                                          # noqa: E402

import decode_ab as ab                                      # noqa: E402  (alternate, cell, filled)
import tinynn_autograd_amd as tn                            # noqa: E402
from tinynn_autograd_amd import _lib                        # noqa: E402
from tinynn_autograd_amd import device_array as da          # noqa: E402
from tinynn_autograd_amd import varlen as vl                # noqa: E402

B, H = 8, 8
DIMS = (64, 128)
ROWS = (256, 1024, 4096)
FILLS = ((25, 0.0, 0.5), (50, 0.0, 1.0), (75, 0.5, 1.0))    # mean fill %, lens uniform in (lo T, hi T]


class Shape(object):
    """The operands of one (T, D) and the two legs: forward + both backward launches, with and without lengths."""

    def __init__(self, t, d, rs):
        block = tn.asarray(rs.standard_normal((1 << 12, d)).astype(np.float32))
        self.q, self.k, self.v, self.do = (ab.filled((B, t, H, d), block) for _ in range(4))
        self.t = t

    def leg(self, lens):
        opts = dict(causal=True, layout="bthd", route="native")
        if lens is not None:
            opts["lens"] = lens

        def run():
            o, lse = da.attention(self.q, self.k, self.v, **opts)
            dq, delta = da.attention_bwd_q(self.q, self.k, self.v, o, self.do, lse, **opts)
            return da.attention_bwd_kv(self.q, self.k, self.v, self.do, lse, delta, **opts)
        return run


def alternate(legs, repeats, inner):
    """{leg: `repeats` medians}, every median over `inner` single timed calls, the legs taking turns inside every repeat."""
    for fn in legs.values():
        fn()
        fn()
    _lib.synchronize()
    t = {name: [] for name in legs}
    for _ in range(repeats):
        for name, fn in legs.items():
            t[name].append(float(np.median([ab.timed(fn, 1) for _ in range(inner)])))
    return t


def model_rates(lines, seq, steps):
    """(c): live tokens per second of the example's training step on --ragged-train batches (wall clock around the one
    read-back of the last loss), the same batches with and without lens."""
    import importlib.util
    path = os.path.join(ROOT, "tinynn-autograd_amd", "examples", "charlm_run.py")
    spec = importlib.util.spec_from_file_location("charlm_run_example", path)
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    from tinynn_autograd_amd.core.tensor import Tensor
    args = example.parse(["--seq", str(seq), "--vocab", "64", "--width", "128", "--heads", "4", "--ragged-train"])
    rs = np.random.RandomState(0)
    x, y = example.make_data(rs, 8, seq, args.vocab, args.period)
    host, targets = example.ragged_batch(rs, x, y, seq)
    ids, targets, lens = Tensor(x), targets.reshape(-1), da.lengths(host)
    legs = {}
    for name, given in (("with lens", lens), ("without", None)):
        np.random.seed(0)
        model, loss_layer = example.build(args)

        def step(model=model, loss_layer=loss_layer, given=given):
            model.zero_grad()
            loss = loss_layer.loss(model.forward(ids, lens=given), targets)
            loss.backward()
            model.step()
            return loss
        legs[name] = step
    for _ in range(3):                                             # warm-up of both legs before either is timed
        for step in legs.values():
            float(step().values)
    rates = {name: [] for name in legs}
    for _ in range(5):                                             # the legs take turns: a drift of the clocks hits both
        for name, step in legs.items():
            _lib.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                loss = step()
            float(loss.values)
            rates[name].append(host.sum() * steps / (time.perf_counter() - t0))
    for name in legs:
        lines.append("charlm     batch 8 x %d tokens (%d live), width 128, 2 blocks, training step %-10s %s live tokens/s (wall "
                     "clock, 5 runs of %d steps, the legs alternating)" % (seq, host.sum(), name, ab.cell(rates[name]), steps))
    lines.append("charlm     with lens / without: %.2fx" % (np.median(rates["with lens"]) / np.median(rates["without"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "varlen_vs_padded.txt"))
    ap.add_argument("--quick", action="store_true", help="the smallest shape of every section only (a dry run of the probe)")
    args = ap.parse_args()
    assert tn.backend_name() != "cpu-twin(test only)"
    assert _lib.get().has_varlen
    props = _lib.device_props()
    device = props["name"].strip() or "%d CUs" % props["cus"]
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
    lines.append("# device: %s; float32, causal, layout bthd, batch %d x %d heads, D = Dv; forward + dq + dk/dv launches; %d medians "
                 "of %d timed calls each, device events, legs alternating; median (min..max) of the medians in us" % (device, B, H, args.repeats, args.inner))
    lines.append("# (a) every lens[b] = T: tnn_varlen_* against tnn_attn_* on the same operands; margin = the baseline's max - min over its medians")
    lines.append("%-5s %-5s %30s %30s %9s %10s %s" % ("D", "T", "tnn_attn us", "tnn_varlen us", "ratio", "margin us", ""))
    shapes = [(d, t) for d in DIMS for t in ROWS]
    if args.quick:
        shapes = [(64, 256)]
    made = {}
    for d, t in shapes:
        s = made[(d, t)] = Shape(t, d, rs)
        got = alternate({"attn": s.leg(None), "varlen": s.leg(da.lengths(np.full(B, t)))}, args.repeats, args.inner)
        med = {k: float(np.median(v)) for k, v in got.items()}
        margin = max(got["attn"]) - min(got["attn"])
        lines.append("%-5d %-5d %30s %30s %8.3fx %10.1f %s" % (d, t, ab.cell(got["attn"]), ab.cell(got["varlen"]),
                                                              med["varlen"] / med["attn"], margin,
                                                              "loses" if med["varlen"] > med["attn"] + margin else ""))
    lines.append("# (b) lens uniform with the given mean fill, against the padded causal launch; live blocks: the share of 64 x 64 "
                 "score blocks under the lengths and the diagonal, of those under the diagonal alone")
    lines.append("%-5s %-5s %-6s %30s %30s %12s %12s" % ("D", "T", "fill %", "padded us", "tnn_varlen us", "varlen/padded", "live blocks"))
    for d, t in shapes:
        s = made[(d, t)]
        for fill, lo, hi in (FILLS[1:2] if args.quick else FILLS):
            host = np.random.RandomState(0).randint(int(lo * t) + 1, int(hi * t) + 1, B)
            live, total = vl.live_blocks(host, t, True)
            got = alternate({"padded": s.leg(None), "varlen": s.leg(da.lengths(host))}, args.repeats, args.inner)
            lines.append("%-5d %-5d %-6d %30s %30s %11.3fx %11.3f" % (
                d, t, fill, ab.cell(got["padded"]), ab.cell(got["varlen"]),
                float(np.median(got["varlen"])) / float(np.median(got["padded"])), live / total))
    made.clear()
    da.trim_cache()
    lines.append("# (c) the model: one training step on a --ragged-train batch")
    model_rates(lines, 128 if args.quick else 1024, 2 if args.quick else 4)


if __name__ == "__main__":
    main()
