"""Token embedding and per-row cross-entropy: the native kernels (csrc/tnn_token.hip) vs the composed route (row gather, one-hot
product, max / exp / sum / log on the generic kernels), in one process, warmed, device-event timed inside one fenced region,
the two sides alternating.  Every call takes the next of several operand sets, which together exceed the 256 MiB last-level
cache, so a call does not find its operands where its predecessor left them.  The box's copy rate is measured in the same
run (a device-to-device copy of 1 GiB, read + written bytes per second) and the native routes are put against it.

    python tools/probes/token_ab.py [--repeats 7] [--inner 4] [--out profiles/token_vs_composed.txt]

Bytes counted for the native route, 4 each: cross-entropy forward M V (every logit once), forward + backward 3 M V (the
logits again, dlogits written); embedding forward + backward 3 M E + V E (table rows read and out written, dy read, EVERY
row of dtable written).  ids, targets, row statistics and the sort's workspace come on top and are not counted.  The
composed side builds its one-hot matrices on the host inside the call (that is the route), so it is timed over fewer calls.
"""

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np                                          # noqa: E402

import tinynn_autograd_amd as tn                            # noqa: E402
from tinynn_autograd_amd import _lib, tokens                # noqa: E402
from tinynn_autograd_amd import device_array as da          # noqa: E402

XENT_SHAPES = ((8192, 1024), (8192, 32768))
EMBED = (16384, 32768, 1024)         # M, V, E
CACHE_BYTES = 256 << 20


def timed(fn, inner):
    e0, e1 = _lib.Event(), _lib.Event()
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    _lib.synchronize()
    return e0.elapsed_ms(e1) * 1e3 / inner


def copy_rate():
    """Bytes read + written per second by a device-to-device copy of 1 GiB (median of 5 after a warm-up)."""
    src = tn.zeros((1 << 28,), np.float32)
    src.copy()
    _lib.synchronize()
    times = [timed(src.copy, 2) for _ in range(5)]
    return 2.0 * src.nbytes / (float(np.median(times)) * 1e-6)


def measure(make, repeats, inner, composed_repeats, composed_inner):
    nat, com = make("native"), make("composed")
    nat()
    nat()
    com()
    _lib.synchronize()
    t = {"native": [], "composed": []}
    for r in range(repeats):
        t["native"].append(timed(nat, inner))
        if r < composed_repeats:
            t["composed"].append(timed(com, composed_inner))
    return t


def xent_sides(m, v, nsets):
    rs = np.random.RandomState(0)
    host = (2.0 * rs.standard_normal((m, v))).astype(np.float32)
    sets = [tn.asarray(np.roll(host, s + 1, axis=0)) for s in range(nsets)]
    targets = tn.asarray(rs.randint(0, v, m).astype(np.int64))
    turn = {"native": 0, "composed": 0}

    def fwd(route):
        def run():
            turn[route] += 1
            return da.cross_entropy(sets[turn[route] % nsets], targets, route=route)
        return run

    def fwd_bwd(route):
        def run():
            turn[route] += 1
            x = sets[turn[route] % nsets]
            loss, _, lse, count = da.cross_entropy(x, targets, route=route)
            return da.cross_entropy_bwd(x, targets, lse, count, 1.0, route=route)
        return run
    return fwd, fwd_bwd


def embed_side(m, v, e, hot, nsets):
    rs = np.random.RandomState(1)
    table = tn.asarray((0.02 * rs.standard_normal((v, e))).astype(np.float32))
    host = rs.standard_normal((m, e)).astype(np.float32)
    sets = [tn.asarray(np.roll(host, s + 1, axis=0)) for s in range(nsets)]
    ids = rs.randint(0, v, m).astype(np.int64)
    if hot:
        ids[rs.permutation(m)[: m // 2]] = 7                    # half of all positions hold ONE token
    ids = tn.asarray(ids)
    turn = {"native": 0, "composed": 0}

    def fwd_bwd(route):
        def run():
            turn[route] += 1
            da.embedding(table, ids, route=route)
            return da.embedding_bwd(sets[turn[route] % nsets], ids, (v, e), route=route)
        return run
    return fwd_bwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "token_vs_composed.txt"))
    args = ap.parse_args()
    assert tn.backend_name() != "cpu-twin(test only)"
    assert _lib.get().has_token
    props = _lib.device_props()
    device = props["name"].strip() or "%d CUs" % props["cus"]
    rate = copy_rate()
    lines = ["# device: %s; float32; native: %d repeats of %d calls, composed: fewer (its one-hot matrices are built on the host "
             "inside the call), over rotating operand sets that exceed %d MiB in all, device events, sides alternating; median "
             "(min..max) in us" % (device, args.repeats, args.inner, CACHE_BYTES >> 20),
             "# copy rate of this box, measured in this run (1 GiB device-to-device, read + written): %.2f TB/s; TB/s and the "
             "share of it are those of the native route (bytes: the module docstring)" % (rate / 1e12),
             "%-10s %-24s %-6s %-8s %26s %32s %9s %7s %8s" % ("op", "shape", "form", "pass", "native us", "composed us",
                                                             "speedup", "TB/s", "of copy")]

    def row(op, shape, form, label, t, nbytes):
        med = {k: float(np.median(v)) for k, v in t.items()}
        cell = {k: "%.1f (%.1f..%.1f)" % (med[k], min(v), max(v)) for k, v in t.items()}
        got = nbytes / (med["native"] * 1e-6)
        lines.append("%-10s %-24s %-6s %-8s %26s %32s %8.1fx %7.2f %7.1f%%" % (
            op, shape, form, label, cell["native"], cell["composed"], med["composed"] / med["native"], got / 1e12,
            100.0 * got / rate))
        return med["native"]

    for m, v in XENT_SHAPES:
        plan = tokens.plan_cross_entropy((m, v), (m,))
        big = m * v * 4 > CACHE_BYTES
        nsets = 2 if big else -(-CACHE_BYTES // (m * v * 4)) + 1
        fwd, fwd_bwd = xent_sides(m, v, nsets)
        for label, make, mult in (("fwd", fwd, 1), ("fwd+bwd", fwd_bwd, 3)):
            t = measure(make, args.repeats, args.inner, 2 if big else args.repeats, 1 if big else args.inner)
            row("xent", "[%d, %d]" % (m, v), plan.form, label, t, mult * m * v * 4)
        del fwd, fwd_bwd
        da.trim_cache()
    m, v, e = EMBED
    took = {}
    for hot in (False, True):
        make = embed_side(m, v, e, hot, 5)
        t = measure(make, args.repeats, args.inner, 2, 1)
        took[hot] = row("embedding", "M %d V %d E %d" % EMBED, "hot" if hot else "unif", "fwd+bwd", t, (3 * m * e + v * e) * 4)
        del make
        da.trim_cache()
    lines.append("# embedding with half of all positions on one token takes %.2fx the uniform case" % (took[True] / took[False]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
