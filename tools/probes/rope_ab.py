"""The rotary position embedding launch against the composed route and against a device copy of the same bytes, in one
process, warmed, device-event timed, the legs alternating (the pattern of tools/probes/decode_ab.py, whose helpers it uses),
float32, layout "bthd":

    (a) the launch   q [8, 1024, 16, 128] plus k [8, 1024, 4, 128], full rotary width, both pairings:
                         copy      q.copy() and k.copy(): the same bytes read and written, no arithmetic — the roof
                         wide      ONE tnn_rope_apply launch on 16-byte accesses
                         element   the same launch on operands moved by one element (the element path)
                         composed  slice reads, products and slice assignments on the array operations
                     The operand sets rotate and together exceed the 256 MiB last-level cache.  Reported: microseconds, TB/s
                     of bytes read + written, and the share of the copy's rate.
    (b) the model    examples/charlm_run.py's model at width 128, 4 heads over 2 key / value heads, 2 blocks, with and without
                     --rope: training steps/s (batch 16 x 256 tokens) and generated tokens/s (batch 8, prompt 32, 224 new
                     tokens), eager and captured — profiles/ragged_generation.txt holds the learned-position figures of the
                     commit before.

    python tools/probes/rope_ab.py [--repeats 5] [--inner 4] [--out profiles/rope_vs_composed.txt] [--quick]
"""

import argparse
import importlib.util
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np                                          # noqa: E402

import decode_ab as ab                                      # noqa: E402  (timed, alternate, cell, filled, copy_rate)
import tinynn_autograd_amd as tn                            # noqa: E402
from tinynn_autograd_amd import _lib, rope                  # noqa: E402
from tinynn_autograd_amd import device_array as da          # noqa: E402

SHAPE = (8, 1024, 16, 4, 128)                               # B, T, H, Hkv, D


class Operands(object):
    """Rotating sets of (q, k, q_out, k_out), aligned, and the same moved by one element."""

    def __init__(self, b, t, h, hkv, d, rs):
        self.bytes = 2 * b * t * (h + hkv) * d * 4          # read + written
        nsets = ab.CACHE_BYTES // self.bytes + 2
        block = tn.asarray(rs.standard_normal((1 << 14, d)).astype(np.float32))
        qs, ks = (b, t, h, d), (b, t, hkv, d)
        self.sets = [(ab.filled(qs, block), ab.filled(ks, block), tn.zeros(qs, np.float32), tn.zeros(ks, np.float32))
                     for _ in range(nsets)]

        def moved(a):
            buf = tn.zeros((a.size + 1,), np.float32)
            view = buf[1:].reshape(a.shape)
            view[...] = a
            return view
        self.moved = [tuple(moved(a) for a in s) for s in self.sets]
        self.turn = 0

    def next(self, moved=False):
        self.turn += 1
        return (self.moved if moved else self.sets)[self.turn % len(self.sets)]


def launch_legs(ops, rot, with_composed=True):
    def copy():
        q, k, _, _ = ops.next()
        return q.copy(), k.copy()

    def wide():
        q, k, qo, ko = ops.next()
        return da.rope(q, k, rotary=rot, route="native", out=(qo, ko))

    def element():
        q, k, qo, ko = ops.next(moved=True)
        return da.rope(q, k, rotary=rot, route="native", out=(qo, ko))

    def composed():
        q, k, qo, ko = ops.next()
        return da.rope(q, k, rotary=rot, route="composed", out=(qo, ko))
    legs = {"copy": copy, "wide": wide, "element": element}
    if with_composed:
        legs["composed"] = composed
    return legs


def load_example():
    path = os.path.join(ROOT, "tinynn-autograd_amd", "examples", "charlm_run.py")
    spec = importlib.util.spec_from_file_location("charlm_run_example", path)
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    return example


def model_rates(lines, prompt, new, steps):
    from tinynn_autograd_amd.core.tensor import Tensor
    from tinynn_autograd_amd.generation import generate
    example = load_example()
    seq = prompt + new
    for flag in ([], ["--rope"]):
        args = example.parse(["--seq", str(seq), "--vocab", "64", "--width", "128", "--heads", "4", "--kv-heads", "2"] + flag)
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
        label = "rope" if flag else "learned positions"
        lines.append("charlm %-18s training, batch 16 x %d tokens, width 128, 4 heads over 2, 2 blocks: %s steps/s (wall clock, "
                     "3 runs of %d steps)" % (label, seq, ab.cell([1.0 / t for t in took]), steps))
        ids = rs.randint(0, args.vocab, (8, prompt))
        lens = np.full((8,), prompt, dtype=np.int64)
        for name, kw in (("eager", dict()), ("eager ragged", dict(prompt_lens=lens)), ("captured", dict(prompt_lens=lens, capture=True))):
            generate(model, ids, 8, temperature=0.0, **kw)                          # warm-up
            took = []
            for _ in range(3):
                _lib.synchronize()
                t0 = time.perf_counter()
                generate(model, ids, new, temperature=0.0, **kw)
                took.append(time.perf_counter() - t0)
            lines.append("charlm %-18s generation %-12s batch 8, prompt %d, %d new tokens: %s tokens/s (wall clock, 3 runs)"
                         % (label, name, prompt, new, ab.cell([8 * new / t for t in took])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rope_vs_composed.txt"))
    ap.add_argument("--quick", action="store_true", help="a quarter of the launch shape and a short model run (a dry run of the probe)")
    args = ap.parse_args()
    assert tn.backend_name() != "cpu-twin(test only)"
    assert _lib.get().has_rope
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
    b, t, h, hkv, d = SHAPE
    if args.quick:
        t //= 4
    lines.append("# device: %s; float32; layout bthd; %d repeats of %d calls, device events, legs alternating; median (min..max) in us"
                 % (device, args.repeats, args.inner))
    lines.append("# copy rate of this box, measured in this run (1 GiB device-to-device, read + written): %.2f TB/s" % (rate / 1e12))
    lines.append("# (a) q [%d, %d, %d, %d] + k [%d, %d, %d, %d], R = D, table length %d; TB/s of bytes read + written; share: of the "
                 "copy leg's rate at the same bytes" % (b, t, h, d, b, t, hkv, d, t))
    ops = Operands(b, t, h, hkv, d, rs)
    for pairing in rope.PAIRINGS:
        rot = rope.Rotary(t, d, pairing=pairing)
        plan = rope.plan_rope((b, t, h, d), (b, t, hkv, d), d, t)
        times = ab.alternate(launch_legs(ops, rot), args.repeats, args.inner)
        med = {k: float(np.median(v)) for k, v in times.items()}
        for name in times:
            lines.append("%-12s %-9s %28s us  %6.2f TB/s  %5.1f %% of the copy%s" % (
                pairing, name, ab.cell(times[name]), ops.bytes / (med[name] * 1e-6) / 1e12, 100.0 * med["copy"] / med[name],
                "  (%d workgroups of %d threads)" % (plan.grid, rope.THREADS) if name == "wide" else ""))
        if med["wide"] > med["composed"]:
            lines.append("# WARNING: the native launch is slower than the composed route (%s)" % pairing)
    del ops
    da.trim_cache()
    lines.append("# (b) the model")
    model_rates(lines, 32, 8 if args.quick else 224, 3 if args.quick else 20)


if __name__ == "__main__":
    main()
