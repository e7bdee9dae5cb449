"""The int8 key / value cache against float32 caches of the same logical shape, in one process, warmed, device-event timed,
the legs alternating (the pattern and the helpers of tools/probes/decode_ab.py), layout "bthd":

    (a) decode     tnn_kvq_decode_attn against tnn_decode_attn (group 1) / tnn_gqa_decode_attn (group 8) at B H x len x D of
                   profiles/decode_vs_fwd.txt; microseconds, live bytes per second against this run's copy rate (int8: B Hkv
                   len (D + Dv + 8), float: B Hkv len (D + Dv) 4), the ratio float / int8, and the float leg against itself.
                   Shapes up to the 256 MiB last-level cache rotate over operand sets that together exceed it.
    (b) fill       tnn_kvq_quantize_rows against a device copy of the same float bytes
    (c) accuracy   max and RMS difference of the attention output between an int8 and a float32 cache holding the same
                   standard-normal k and v, len 4096 (recorded, not asserted)
    (d) generation tokens/s of examples/charlm_run.py's model, captured, with and without --kv-quant int8

    python tools/probes/kvq_ab.py [--repeats 5] [--inner 4] [--out profiles/kvq_vs_float.txt] [--quick]
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
from tinynn_autograd_amd import _lib, kvq                   # noqa: E402
from tinynn_autograd_amd import device_array as da          # noqa: E402

HEADS = ab.HEADS
GROUPS = (1, 8)
DIMS = (64, 128)


class Shape(object):
    """The operands of one (B H, len, D, group): float caches and int8 caches of Hkv = H / group heads filled from the same
    random block, one q, one new row."""

    def __init__(self, bh, length, d, group, rs):
        self.b, self.h, self.hkv, self.length, self.d, self.group = bh // HEADS, HEADS, HEADS // group, length, d, group
        tmax = length + 1
        rows = self.b * self.hkv * length
        self.bytes_float, self.bytes_int8 = rows * 2 * d * 4, rows * (2 * d + 8)
        sets = lambda nbytes: 1 if nbytes > ab.CACHE_BYTES else ab.CACHE_BYTES // nbytes + 2
        block = rs.standard_normal((1 << 14, d)).astype(np.float32)
        codes, scales = kvq.quantize_host(block)
        fblock, cblock = tn.asarray(block), da.asarray(codes, dtype=np.uint8)
        sblock = da.asarray(np.ascontiguousarray(scales[:, None]), dtype=np.float32)
        shape, sshape = (self.b, tmax, self.hkv, d), (self.b, tmax, self.hkv, 1)
        self.floats = [(ab.filled(shape, fblock), ab.filled(shape, fblock)) for _ in range(sets(self.bytes_float))]
        self.int8 = [(self.filled(shape, cblock, np.uint8), self.filled(shape, cblock, np.uint8),
                      self.filled(sshape, sblock, np.float32).reshape(self.b, tmax, self.hkv),
                      self.filled(sshape, sblock, np.float32).reshape(self.b, tmax, self.hkv))
                     for _ in range(sets(self.bytes_int8))]
        one = lambda heads: tn.asarray(rs.standard_normal((self.b, heads, d)).astype(np.float32))
        self.q, self.k_new, self.v_new = one(self.h), one(self.hkv), one(self.hkv)
        self.turn = 0

    @staticmethod
    def filled(shape, block, dtype):
        out = da.zeros(shape, dtype)
        flat = out.reshape(-1, shape[-1])
        n = block.shape[0]
        for start in range(0, flat.shape[0], n):
            stop = min(start + n, flat.shape[0])
            flat[start:stop] = block[:stop - start]
        return out

    def run_float(self):
        self.turn += 1
        k, v = self.floats[self.turn % len(self.floats)]
        if self.group == 1:
            return da.attention_decode(self.q, k, v, self.length, self.k_new, self.v_new, layout="bthd", route="native")
        return da.gqa_decode(self.q, k, v, self.length, self.k_new, self.v_new, layout="bthd", route="native")

    def run_int8(self):
        self.turn += 1
        kc, vc, ks, vs = self.int8[self.turn % len(self.int8)]
        return da.attention_decode_kvq(self.q, kc, vc, ks, vs, self.length, self.k_new, self.v_new, layout="bthd", route="native")


def decode_table(lines, rate, repeats, inner, quick):
    lines.append("(a) decode: us per call, median (min..max) of %d x %d calls; TB/s of live bytes (share of the copy rate, read + written)" % (repeats, inner))
    lines.append("%5s %6s %4s %3s | %-24s %-14s | %-24s %-14s | %-9s %s" % ("B H", "len", "D", "grp", "float32 us", "TB/s", "int8 us",
                                                                            "TB/s", "f32/int8", "f32 second leg / first"))
    rs = np.random.RandomState(0)
    for group in GROUPS:
        for d in DIMS:
            for bh in ab.BH:
                for length in ab.LENS:
                    if quick and (bh, length) not in ((8, 4096), (512, 4096)):
                        continue
                    s = Shape(bh, length, d, group, rs)
                    t = ab.alternate({"float": s.run_float, "int8": s.run_int8, "float2": s.run_float}, repeats, inner)
                    f, i, f2 = (float(np.median(t[n])) for n in ("float", "int8", "float2"))
                    tb = lambda nbytes, us: "%.2f (%.0f%%)" % (nbytes / us * 1e-6, 100.0 * nbytes / (us * 1e-6) / rate)
                    lines.append("%5d %6d %4d %3d | %-24s %-14s | %-24s %-14s | %-9s %.3f%s" % (
                        bh, length, d, group, ab.cell(t["float"]), tb(s.bytes_float, f), ab.cell(t["int8"]), tb(s.bytes_int8, i),
                        "%.2fx" % (f / i), f2 / f, "   SLOWER than float32" if i > f else ""))
                    del s
                    da.trim_cache()


def fill_table(lines, repeats, inner):
    lines.append("")
    lines.append("(b) fill: tnn_kvq_quantize_rows (k and v, one launch) against two device copies of the same float bytes, us")
    rs = np.random.RandomState(1)
    for b, t, hkv, d in ((8, 512, 8, 128), (8, 4096, 8, 128), (8, 4096, 8, 64)):
        k, v = (tn.asarray(rs.standard_normal((b, t, hkv, d)).astype(np.float32)) for _ in range(2))
        kc, vc = (da.zeros((b, t, hkv, d), np.uint8) for _ in range(2))
        ks, vs = (da.zeros((b, t, hkv), np.float32) for _ in range(2))
        legs = {"quantize": lambda: da.kvq_quantize_rows(k, v, kc, vc, ks, vs, 0, "bthd", route="native"),
                "copy": lambda: (k.copy(), v.copy())}
        tm = ab.alternate(legs, repeats, inner)
        lines.append("B %d T %d Hkv %d D %d (%.1f MiB of floats): quantize %s, copy %s" % (
            b, t, hkv, d, 2 * k.nbytes / 2 ** 20, ab.cell(tm["quantize"]), ab.cell(tm["copy"])))


def accuracy(lines):
    lines.append("")
    lines.append("(c) accuracy: int8 against float32 caches holding the same standard-normal k and v, q standard normal, len 4096")
    rs = np.random.RandomState(2)
    for d, group in ((64, 1), (128, 1), (128, 8)):
        b, hkv, n = 2, HEADS // group, 4096
        k, v = (rs.standard_normal((b, n, hkv, d)).astype(np.float32) for _ in range(2))
        q = rs.standard_normal((b, HEADS, d)).astype(np.float32)
        kn, vn = (rs.standard_normal((b, hkv, d)).astype(np.float32) for _ in range(2))
        kf, vf = (da.zeros((b, n + 1, hkv, d), np.float32) for _ in range(2))
        kf[:, :n], vf[:, :n] = tn.asarray(k), tn.asarray(v)
        kc, vc = (da.zeros((b, n + 1, hkv, d), np.uint8) for _ in range(2))
        ks, vs = (da.zeros((b, n + 1, hkv), np.float32) for _ in range(2))
        da.kvq_quantize_rows(k, v, kc, vc, ks, vs, 0, "bthd", route="native")
        of = np.asarray(da.gqa_decode(q, kf, vf, n, kn, vn, layout="bthd", route="native"), dtype=np.float64)
        oq = np.asarray(da.attention_decode_kvq(q, kc, vc, ks, vs, n, kn, vn, layout="bthd", route="native"), dtype=np.float64)
        lines.append("D %d group %d: max |o_int8 - o_f32| %.3e, rms %.3e (rms of o_f32 %.3e)" % (
            d, group, np.abs(oq - of).max(), np.sqrt(((oq - of) ** 2).mean()), np.sqrt((of ** 2).mean())))


def generation_rates(lines, prompt, new):
    lines.append("")
    lines.append("(d) generation: examples/charlm_run.py's model (untrained), batch 8, prompt %d, %d new tokens, width 128, 4 heads "
                 "(D 32), 2 blocks, captured; tokens/s, wall clock, 3 runs" % (prompt, new))
    spec = importlib.util.spec_from_file_location("charlm_run_example", os.path.join(ROOT, "tinynn-autograd_amd", "examples",
                                                                                     "charlm_run.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    from tinynn_autograd_amd.generation import KVCache, generate
    model, _ = example.build(example.parse(["--seq", str(prompt + new), "--vocab", "64", "--width", "128", "--heads", "4"]))
    ids = np.random.RandomState(0).randint(0, 64, (8, prompt))
    for quant in (None, "int8"):
        cache = lambda: KVCache(prompt + new, quant=quant) if quant else True
        generate(model, ids, 8, temperature=0.0, cache=KVCache(prompt + 8, quant=quant) if quant else True, capture=True)
        took = []
        for _ in range(3):
            _lib.synchronize()
            t0 = time.perf_counter()
            generate(model, ids, new, temperature=0.0, cache=cache(), capture=True)
            took.append(time.perf_counter() - t0)
        lines.append("kv cache %-8s %s tokens/s" % (quant or "float32", ab.cell([8 * new / t for t in took])))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--repeats", default=5, type=int)
    parser.add_argument("--inner", default=4, type=int)
    parser.add_argument("--out", default=None)
    parser.add_argument("--quick", action="store_true", help="two (B H, len) cells per D and group")
    args = parser.parse_args()
    assert _lib.get().has_kvq and tn.backend_name() == "hip-gfx950", "the probe measures libtnn_hip.so on the GPU"
    rate = ab.copy_rate()
    lines = ["# tools/probes/kvq_ab.py on %s; device copy rate of this run %.2f TB/s read + written (%.2f TB/s one way)"
             % (_lib.device_props()["name"], rate * 1e-12, rate * 0.5e-12), ""]
    decode_table(lines, rate, args.repeats, args.inner, args.quick)
    fill_table(lines, args.repeats, args.inner)
    accuracy(lines)
    generation_rates(lines, 32, 224)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
