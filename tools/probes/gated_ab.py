"""The gated-activation launches against the composed route and against a device copy of the same bytes, in one process,
warmed, device-event timed, the legs alternating (the pattern of tools/probes/rope_ab.py, whose helpers it shares through
decode_ab.py), float32, act = silu (SwiGLU), the PACKED layout TransformerBlock(mlp=) uses: z [M, 2 F] read in place, y [M, F],
dz [M, 2 F]:

    (a) the launches   M = 8192, F in {4096, 11008} — every operand set is beyond the 256 MiB last-level cache:
                         copy      x.copy() of 1.5 M F elements (forward: 3 M F read + written) or 2.5 M F (backward: 5 M F):
                                   the same bytes, no arithmetic — the roof
                         wide      ONE tnn_gated_fwd / tnn_gated_bwd launch on 16-byte accesses
                         element   the same launch on a z moved by one element (the element path)
                         composed  sigmoid, products and sums on the generic operations, slices of z, slice assignments into dz
                       Reported: microseconds, TB/s of bytes read + written, and the share of the copy's rate.
    (b) the model      examples/charlm_run.py's model at width 128, 4 heads, 2 blocks, --mlp gelu against --mlp swiglu: training
                       steps/s (batch 16 x 256 tokens) and generated tokens/s (batch 8, prompt 32, 224 new tokens), eager and
                       captured.

    python tools/probes/gated_ab.py [--repeats 5] [--inner 4] [--out profiles/gated_vs_composed.txt] [--quick]
"""

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np                                          # noqa: E402

import decode_ab as ab                                      # noqa: E402  (timed, alternate, cell, filled, copy_rate)
import rope_ab                                              # noqa: E402  (load_example)
import tinynn_autograd_amd as tn                            # noqa: E402
from tinynn_autograd_amd import _lib, gated                 # noqa: E402
from tinynn_autograd_amd import device_array as da          # noqa: E402

M = 8192
WIDTHS = (4096, 11008)
ACT = "silu"


def moved(a):
    """The same values at an address one element past a 16-byte boundary."""
    buf = tn.zeros((a.size + 1,), np.float32)
    view = buf[1:].reshape(a.shape)
    view[...] = a
    return view


class Operands(object):
    def __init__(self, m, f, rs):
        self.z = ab.filled((m, 2 * f), tn.asarray(rs.standard_normal((1 << 10, 2 * f)).astype(np.float32)))
        self.dy = ab.filled((m, f), tn.asarray(rs.standard_normal((1 << 10, f)).astype(np.float32)))
        self.dz = tn.zeros((m, 2 * f), np.float32)
        self.z_moved = moved(self.z)
        self.fwd_bytes, self.bwd_bytes = 3 * m * f * 4, 5 * m * f * 4
        self.fwd_copy = tn.zeros((3 * m * f // 2,), np.float32)
        self.bwd_copy = tn.zeros((5 * m * f // 2,), np.float32)


def legs(ops, backward):
    if backward:
        return {"copy": ops.bwd_copy.copy,
                "wide": lambda: da.gated_bwd(ops.z, None, ops.dy, act=ACT, packed=True, route="native", dz_out=ops.dz),
                "element": lambda: da.gated_bwd(ops.z_moved, None, ops.dy, act=ACT, packed=True, route="native", dz_out=ops.dz),
                "composed": lambda: da.gated_bwd(ops.z, None, ops.dy, act=ACT, packed=True, route="composed", dz_out=ops.dz)}
    return {"copy": ops.fwd_copy.copy,
            "wide": lambda: da.gated(ops.z, act=ACT, packed=True, route="native"),
            "element": lambda: da.gated(ops.z_moved, act=ACT, packed=True, route="native"),
            "composed": lambda: da.gated(ops.z, act=ACT, packed=True, route="composed")}


def model_rates(lines, prompt, new, steps):
    from tinynn_autograd_amd.core.tensor import Tensor
    from tinynn_autograd_amd.generation import generate
    example = rope_ab.load_example()
    seq = prompt + new
    for mlp in ("gelu", "swiglu"):
        args = example.parse(["--seq", str(seq), "--vocab", "64", "--width", "128", "--heads", "4", "--mlp", mlp])
        np.random.seed(0)
        model, loss_layer = example.build(args)
        rs = np.random.RandomState(0)
        x, y = example.make_data(rs, 16, seq, args.vocab, args.period)

        def train_step():
            model.zero_grad()
            loss = loss_layer.loss(model.forward(Tensor(x)), y.reshape(-1))
            loss.backward()
            model.step()
        for _ in range(3):
            train_step()
        took = []
        for _ in range(3):
            _lib.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                train_step()
            _lib.synchronize()
            took.append((time.perf_counter() - t0) / steps)
        hidden = model.net.layers[1].hidden
        lines.append("charlm --mlp %-7s (hidden %d) training, batch 16 x %d tokens, width 128, 4 heads, 2 blocks: %s steps/s (wall "
                     "clock, 3 runs of %d steps)" % (mlp, hidden, seq, ab.cell([1.0 / t for t in took]), steps))
        ids = rs.randint(0, args.vocab, (8, prompt))
        lens = np.full((8,), prompt, dtype=np.int64)
        for name, kw in (("eager", dict()), ("captured", dict(prompt_lens=lens, capture=True))):
            generate(model, ids, 8, temperature=0.0, **kw)                          # warm-up
            took = []
            for _ in range(3):
                _lib.synchronize()
                t0 = time.perf_counter()
                generate(model, ids, new, temperature=0.0, **kw)
                took.append(time.perf_counter() - t0)
            lines.append("charlm --mlp %-7s generation %-9s batch 8, prompt %d, %d new tokens: %s tokens/s (wall clock, 3 runs)"
                         % (mlp, name, prompt, new, ab.cell([8 * new / t for t in took])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gated_vs_composed.txt"))
    ap.add_argument("--quick", action="store_true", help="an eighth of the rows and a short model run (a dry run of the probe)")
    args = ap.parse_args()
    assert tn.backend_name() != "cpu-twin(test only)"
    assert _lib.get().has_gated
    props = _lib.device_props()
    device = props["name"].strip() or "%d CUs" % props["cus"]
    rate = ab.copy_rate()
    rs = np.random.RandomState(0)

    class Lines(list):
        def append(self, line):
            list.append(self, line)
            print(line, flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    f.write("\n".join(self) + "\n")
    lines = Lines()
    m = M // 8 if args.quick else M
    lines.append("# device: %s; float32; act %s; packed z [M, 2 F] -> y [M, F], dz [M, 2 F]; %d repeats of %d calls, device events, "
                 "legs alternating; median (min..max) in us" % (device, ACT, args.repeats, args.inner))
    lines.append("# copy rate of this box, measured in this run (1 GiB device-to-device, read + written): %.2f TB/s" % (rate / 1e12))
    lines.append("# (a) M = %d; TB/s of bytes read + written (forward 3 M F, backward 5 M F elements); share: of the copy leg's rate "
                 "at the same bytes" % m)
    for f in WIDTHS:
        ops = Operands(m, f, rs)
        for backward in (False, True):
            lds = dict(gate=2 * f, up=2 * f)
            if backward:
                lds.update(dgate=2 * f, dup=2 * f)
            plan = gated.plan_gated(m, f, ACT, backward, lds=lds)
            times = ab.alternate(legs(ops, backward), args.repeats, args.inner)
            med = {k: float(np.median(v)) for k, v in times.items()}
            nbytes = ops.bwd_bytes if backward else ops.fwd_bytes
            for name in times:
                lines.append("F %-6d %-8s %-9s %28s us  %6.2f TB/s  %5.1f %% of the copy%s" % (
                    f, "backward" if backward else "forward", name, ab.cell(times[name]), nbytes / (med[name] * 1e-6) / 1e12,
                    100.0 * med["copy"] / med[name],
                    "  (%d workgroups of %d threads)" % (plan.grid, gated.THREADS) if name == "wide" else ""))
            if med["wide"] > med["composed"]:
                lines.append("# WARNING: the native launch is slower than the composed route (F %d)" % f)
        del ops
        da.trim_cache()
    lines.append("# (b) the model")
    model_rates(lines, 32, 8 if args.quick else 224, 3 if args.quick else 20)


if __name__ == "__main__":
    main()
