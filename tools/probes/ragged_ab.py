"""The ragged decoding step (csrc/tnn_ragged.hip) against the uniform one (csrc/tnn_decode.hip) of the SAME build, in one
process per section, warmed, device-event timed, the legs alternating, float32, cache layout "bthd" with 8 heads; the operand
sets rotate as in tools/probes/decode_ab.py (whose Shape this probe reuses).

    (a) tnn_ragged_decode_attn against tnn_decode_attn at uniform lengths, three shapes of profiles/decode_vs_fwd.txt.  The
        uniform kernel runs as TWO legs, so that its spread against itself is on the table next to the ragged kernel's ratio
    (b) the first shape as B H sequences of ONE head, with ragged lengths uniform in [len / 4, len]: bytes of the live
        prefixes per second — what the workgroups without keys and the uneven runs cost
    (c) DESIGN section 4d's generation model (width 128, 2 blocks, batch 8, prompt 32, 224 new tokens): tokens/s of today's
        generate, the ragged path eager, the ragged path captured, and captured with prompts of 8 .. 32 tokens

Every section is a child process under its own time limit; the first that fails ends the probe.

    python tools/probes/ragged_ab.py [--repeats 20] [--inner 4] [--out profiles/ragged_generation.txt] [--quick]
"""

import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SHAPES = ((8, 4096, 128), (64, 4096, 64), (8, 32768, 128))
LIMITS = {"a": 240, "b": 120, "c": 300}        # seconds per section


def emit(out, line):
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def section_a(args, shapes):
    import numpy as np
    import decode_ab as ab
    from tinynn_autograd_amd import decoding, device_array as da, ragged
    rs = np.random.RandomState(0)
    emit(args.out, "# (a) uniform lengths: tnn_decode_attn twice (its spread against itself) and tnn_ragged_decode_attn; us, median "
                   "(min..max) of %d repeats of %d calls; again and ragged: the ratio of that leg's median to the first uniform leg's; "
                   "inside = the ragged median lies within the 10th .. 90th percentile of the two uniform legs' times" %
         (args.repeats, args.inner))
    emit(args.out, "%-5s %-6s %-4s %-6s %26s %26s %26s %8s %8s %s" % ("B H", "len", "D", "splits", "uniform us", "uniform again us",
                                                                      "ragged us", "again", "ragged", ""))
    for bh, n, d in shapes:
        s = ab.Shape(bh, n, d, rs)
        lens = da.lengths(np.full(s.b, n, dtype=np.int64))
        plan = ragged.plan_ragged_decode((s.b, s.h, d), (s.b, s.tmax, s.h, d), (s.b, s.tmax, s.h, d), (s.b,))
        uniform = decoding.plan_decode((s.b, s.h, d), (s.b, s.tmax, s.h, d), (s.b, s.tmax, s.h, d), n)
        assert plan.splits == uniform.splits

        def rag():
            k, v = s.caches()
            return da.attention_decode_ragged(s.q, k, v, lens, s.k_new, s.v_new, layout="bthd", route="native")
        t = ab.alternate({"uniform": s.decode, "again": s.decode, "ragged": rag}, args.repeats, args.inner)
        med = {k: float(np.median(v)) for k, v in t.items()}
        lo, hi = np.percentile(t["uniform"] + t["again"], [10, 90])
        emit(args.out, "%-5d %-6d %-4d %-6d %26s %26s %26s %7.3fx %7.3fx %s" % (
            bh, n, d, plan.splits, ab.cell(t["uniform"]), ab.cell(t["again"]), ab.cell(t["ragged"]), med["again"] / med["uniform"],
            med["ragged"] / med["uniform"], "inside" if lo <= med["ragged"] <= hi else "OUTSIDE the uniform kernel's own spread"))
        del s
        da.trim_cache()
    emit(args.out, "# what the ragged form adds per workgroup: lens[b] is a scalar load that can only be issued once the kernel arguments "
                   "(the pointer, H) have arrived, and the run of chunks — hence every K and V address — waits for it: one more dependent "
                   "round trip to memory at the top of every workgroup, which weighs most where a workgroup's run is one chunk (DESIGN 4d)")


def section_b(args, shapes):
    import numpy as np
    import decode_ab as ab
    from tinynn_autograd_amd import device_array as da
    rs = np.random.RandomState(1)
    bh, n, d = shapes[0]
    ab.HEADS = 1                                               # B H sequences of one head each: every one its own length
    s = ab.Shape(bh, n, d, rs)
    rate = ab.copy_rate()
    ragged_lens = rs.randint(n // 4, n + 1, s.b).astype(np.int64)
    emit(args.out, "# (b) B %d, H 1, Tmax %d, D %d: lengths uniform in [len / 4, len] against all at len; bytes = sum_b H lens[b] (D + Dv) 4, "
                   "the live prefixes alone; copy rate of this box in this run: %.2f TB/s" % (bh, s.tmax, d, rate / 1e12))
    legs, live = {}, {}
    for name, host in (("all at len", np.full(s.b, n, dtype=np.int64)), ("ragged", ragged_lens)):
        lens = da.lengths(host)
        live[name] = int(host.sum()) * s.h * 2 * d * 4

        def leg(lens=lens):
            k, v = s.caches()
            return da.attention_decode_ragged(s.q, k, v, lens, s.k_new, s.v_new, layout="bthd", route="native")
        legs[name] = leg
    t = ab.alternate(legs, args.repeats, args.inner)
    for name in legs:
        m = float(np.median(t[name]))
        emit(args.out, "%-12s lens %-40s %26s us  %6.2f TB/s of live bytes, %5.1f%% of the copy rate" % (
            name, "all %d" % n if name != "ragged" else str(ragged_lens.tolist()), ab.cell(t[name]), live[name] / (m * 1e-6) / 1e12,
            100.0 * live[name] / (m * 1e-6) / rate))


def section_c(args, new):
    import importlib.util
    import numpy as np
    import decode_ab as ab
    from tinynn_autograd_amd import _lib
    from tinynn_autograd_amd.generation import generate
    path = os.path.join(ROOT, "tinynn-autograd_amd", "examples", "charlm_run.py")
    spec = importlib.util.spec_from_file_location("charlm_run_example", path)
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    prompt = 32
    cfg = example.parse(["--seq", str(prompt + new), "--vocab", "64", "--width", "128", "--heads", "4"])
    model, _ = example.build(cfg)
    rs = np.random.RandomState(0)
    ids = rs.randint(0, cfg.vocab, (8, prompt))
    short = rs.randint(8, prompt + 1, 8)
    full = np.full(8, prompt)
    variants = (("today's generate", dict()), ("ragged eager", dict(prompt_lens=full)),
                ("ragged captured", dict(prompt_lens=full, capture=True)),
                ("ragged captured, prompts of %d..%d tokens" % (short.min(), short.max()), dict(prompt_lens=short, capture=True)))
    emit(args.out, "# (c) generation: batch 8, prompt %d, %d new tokens, width 128, 2 blocks, greedy, cache=True; tokens/s = 8 x new "
                   "tokens / wall clock of one generate() call (it ends in its one read-back), median (min..max) of 5 runs, the "
                   "variants alternating; a captured run records its graph inside the timed call" % (prompt, new))
    rates = {name: [] for name, _ in variants}
    outs = {}
    for name, kw in variants:
        outs[name] = generate(model, ids, new, temperature=0.0, **kw)              # warm-up, and the ids for the check below
    same = all(np.array_equal(outs[name], outs["today's generate"]) for name, _ in variants[:3])
    for _ in range(5):
        for name, kw in variants:
            _lib.synchronize()
            t0 = time.perf_counter()
            generate(model, ids, new, temperature=0.0, **kw)
            rates[name].append(8 * new / (time.perf_counter() - t0))
    base = float(np.median(rates["today's generate"]))
    for name, _ in variants:
        emit(args.out, "%-48s %34s tokens/s  %.2fx today's" % (name, ab.cell(rates[name]), float(np.median(rates[name])) / base))
    emit(args.out, "# the three uniform-length variants gave %s ids" % ("IDENTICAL" if same else "DIFFERENT"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_generation.txt"))
    ap.add_argument("--quick", action="store_true", help="the smallest shape of every section only (a dry run of the probe)")
    ap.add_argument("--section", choices=sorted(LIMITS), help="run ONE section in this process (what the driver starts)")
    args = ap.parse_args()
    if args.section is None:                                   # the driver: one child per section, each under its own limit
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            open(args.out, "w").close()
        for name in sorted(LIMITS):
            cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--section", name,
                   "--repeats", str(args.repeats), "--inner", str(args.inner), "--out", args.out or ""]
            rc = subprocess.call(cmd + (["--quick"] if args.quick else []))
            if rc != 0:
                emit(args.out, "# section (%s) ended with status %d: the probe stops here" % (name, rc))
                return rc
        return 0
    import tinynn_autograd_amd as tn
    from tinynn_autograd_amd import _lib
    assert tn.backend_name() != "cpu-twin(test only)"
    assert _lib.get().has_ragged and _lib.get().has_decode
    shapes = SHAPES[:1] if args.quick else SHAPES
    if args.section == "a":
        props = _lib.device_props()
        emit(args.out, "# device: %s; float32; layout bthd, 8 heads; device events, legs alternating in one process; shapes up to 256 MiB "
                       "rotate over operand sets that exceed it in all" % (props["name"].strip() or "%d CUs" % props["cus"]))
        section_a(args, shapes)
    elif args.section == "b":
        section_b(args, shapes)
    else:
        section_c(args, 16 if args.quick else 224)
    return 0


if __name__ == "__main__":
    sys.exit(main())
