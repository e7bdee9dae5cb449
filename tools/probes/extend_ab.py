"""Cache-extending attention: ONE tnn_extend_attn call (csrc/tnn_extend.hip) against the only routes the code had before it for
the same job — T new rows per sequence on top of `len` cached ones — in one process, warmed, device-event timed, the legs
alternating (the helpers of decode_ab.py), float32, cache layout "bthd", batch 4 x 8 heads, D = Dv = 128:

    (a) len x T        extend   ONE da.attention_extend call: attention of the T rows over len + T keys and the append
                       decode   T calls of da.attention_decode, one row each with its append (the planner's key split): what
                                continuing a cached sequence cost — the three one-row projections per step are NOT in it
                       refill   tnn_attn_fwd (causal) over the WHOLE prefix of len + T rows and the slice-assigned fill of the
                                cache: what throwing the cache away cost — the projections of the len old rows are NOT in it
                       Reported: microseconds, median (min..max), and the two ratios; "loses" marks a shape at which the
                       extension's median exceeds a leg's by more than the legs' own spread.
    (b) the model      examples/charlm_run.py's model (width 128, 4 heads, 2 blocks, untrained), batch 8: prompt tokens/s of
                       generate(..., 1 new token) with the prompt in one piece and with prefill_chunk = 256 and 64.

    python tools/probes/extend_ab.py [--repeats 5] [--inner 2] [--out profiles/extend_vs_fwd.txt] [--quick]
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

B, H, D = 4, 8, 128
LENS = (0, 256, 1024, 4096)
ROWS = (1, 16, 64, 256)


class Shape(object):
    """The operands of one (len, T): caches of len + T rows, the T new rows, the whole prefix for the refill leg."""

    def __init__(self, length, t, rs):
        self.length, self.t, n = length, t, length + t
        block = tn.asarray(rs.standard_normal((1 << 12, D)).astype(np.float32))
        self.k, self.v = ab.filled((B, n, H, D), block), ab.filled((B, n, H, D), block)
        new = lambda rows: tn.asarray(rs.standard_normal((B, rows, H, D)).astype(np.float32))
        self.q, self.k_new, self.v_new = new(t), new(t), new(t)
        host = [np.asarray(a) for a in (self.q, self.k_new, self.v_new)]
        self.steps = [tuple(tn.asarray(np.ascontiguousarray(a[:, i])) for a in host) for i in range(t)]      # [B, H, D] per step
        self.q_all, self.k_all, self.v_all = ab.filled((B, n, H, D), block), ab.filled((B, n, H, D), block), ab.filled((B, n, H, D), block)

    def extend(self):
        return da.attention_extend(self.q, self.k, self.v, self.length, self.k_new, self.v_new, layout="bthd", route="native")

    def decode(self):
        out = None
        for i, (q, kn, vn) in enumerate(self.steps):
            out = da.attention_decode(q, self.k, self.v, self.length + i, kn, vn, layout="bthd", route="native")
        return out

    def refill(self):
        out, _ = da.attention(self.q_all, self.k_all, self.v_all, True, None, "bthd", "native")
        self.k[:, :self.length + self.t] = self.k_all
        self.v[:, :self.length + self.t] = self.v_all
        return out


def prompt_rates(lines, prompt, chunks):
    """(b): prompt tokens per second of the example's model, batch 8, one new token (wall clock around the one read-back)."""
    import importlib.util
    path = os.path.join(ROOT, "tinynn-autograd_amd", "examples", "charlm_run.py")
    spec = importlib.util.spec_from_file_location("charlm_run_example", path)
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    from tinynn_autograd_amd.generation import generate
    args = example.parse(["--seq", str(prompt + 1), "--vocab", "64", "--width", "128", "--heads", "4"])
    model, _ = example.build(args)
    ids = np.random.RandomState(0).randint(0, args.vocab, (8, prompt))
    want = None
    for chunk in chunks:
        out = generate(model, ids, 1, temperature=0.0, prefill_chunk=chunk)       # warm-up
        want = out if want is None else want
        took = []
        for _ in range(5):
            _lib.synchronize()
            t0 = time.perf_counter()
            generate(model, ids, 1, temperature=0.0, prefill_chunk=chunk)
            took.append(time.perf_counter() - t0)
        lines.append("charlm     batch 8, prompt %d, width 128, 2 blocks, prefill_chunk=%-5s %s prompt tokens/s (wall clock, 5 runs); "
                     "token equal to the one-piece run's: %s" % (prompt, chunk, ab.cell([8 * prompt / t for t in took]),
                                                                 bool(np.array_equal(out, want))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "extend_vs_fwd.txt"))
    ap.add_argument("--quick", action="store_true", help="the smallest shape of every section only (a dry run of the probe)")
    args = ap.parse_args()
    assert tn.backend_name() != "cpu-twin(test only)"
    assert _lib.get().has_extend
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
    for line in ["# device: %s; float32; layout bthd, batch %d x %d heads, D = Dv = %d; %d repeats of %d calls, device events, legs "
                 "alternating; median (min..max) in us" % (device, B, H, D, args.repeats, args.inner),
                 "# (a) extend = ONE tnn_extend_attn (grid B H ceil(T / 64) = %d ceil(T / 64) workgroups, keys not split); decode = T "
                 "tnn_decode_attn steps; refill = tnn_attn_fwd over len + T rows + the cache fill" % (B * H),
                 "%-6s %-5s %26s %28s %28s %10s %10s %s" % ("len", "T", "extend us", "decode us", "refill us", "decode/ext", "refill/ext", "")]:
        lines.append(line)
    shapes = [(n, t) for n in LENS for t in ROWS]
    if args.quick:
        shapes = [(256, 16)]
    for n, t in shapes:
        s = Shape(n, t, rs)
        got = ab.alternate({"extend": s.extend, "decode": s.decode, "refill": s.refill}, args.repeats, args.inner)
        med = {k: float(np.median(v)) for k, v in got.items()}
        spread = max(max(v) - min(v) for v in got.values())
        loses = [k for k in ("decode", "refill") if med["extend"] > med[k] + spread]
        lines.append("%-6d %-5d %26s %28s %28s %9.2fx %9.2fx %s" % (
            n, t, ab.cell(got["extend"]), ab.cell(got["decode"]), ab.cell(got["refill"]), med["decode"] / med["extend"],
            med["refill"] / med["extend"], "loses to " + ", ".join(loses) if loses else ""))
        del s
        da.trim_cache()
    lines.append("# (b) the model: the prompt in one piece (None) and in pieces")
    prompt_rates(lines, 64 if args.quick else 1024, (None, 16) if args.quick else (None, 256, 64))


if __name__ == "__main__":
    main()
