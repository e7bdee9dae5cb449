"""Writes tests/golden/rope_cases.npz: the results of rope_oracle's named cases (inputs are regenerated from seeds, not stored)
and a few 50-digit spot values of the cos / sin tables, produced by this project's oracle and mpmath alone.

    <pairing>.<name>.a / .b    the rotated tensors of rope_oracle.CASES at offset GOLDEN_OFFSET, float32 inputs and tables, as
                               float64 (the long-double oracle's values, rounded)
    table.spots                [n, 2] the (p, i) of rope_oracle.TABLE_SPOTS (P = 4096, R = TABLE_R, base 10000)
    table.cos / table.sin      [n, 2] double-double pairs (hi, lo) of the 50-digit cosine and sine of p base^(-2 i / R)
    lm.*                       the two-block rotary language model's fixture (lm_fixture below)

Checked here, on the CPU, for float32 AND float64:
  * the planner's tables meet the table bound at every spot, and a table built from a FLOAT64 angle misses it at P = 4096
    (so the long-double angle is part of the contract and the test notices a regression);
  * on every case the oracle alone is within its bound, a same-precision numpy evaluation (rope.rope_host) is within it too,
    and the bound is below 1e-3 of the median output magnitude;
  * position shift: the attention scores of rotated q and k do not change when every position is shifted by the same amount
    (float64, to 1e-12).

    python tests/gen_rope_golden.py
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conftest                                                             # noqa: E402,F401  (puts the repository on sys.path)
import rope_oracle as ro                                                    # noqa: E402
from tinynn_autograd_amd import rope as rp                                  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rope_cases.npz")


def table_spots():
    import mpmath as mp
    mp.mp.dps = 50
    cos_dd, sin_dd = [], []
    for p, i in ro.TABLE_SPOTS:
        angle = mp.mpf(p) * mp.power(mp.mpf(ro.BASE), -mp.mpf(2 * i) / ro.TABLE_R)
        cos_dd.append(ro.dd_split(mp.cos(angle)))
        sin_dd.append(ro.dd_split(mp.sin(angle)))
    data = {"table.spots": np.array(ro.TABLE_SPOTS, dtype=np.int64), "table.cos": np.array(cos_dd), "table.sin": np.array(sin_dd)}
    exact_c, exact_s = ro.dd_join(*data["table.cos"].T), ro.dd_join(*data["table.sin"].T)
    for dtype in (np.float32, np.float64):
        cos_t, sin_t = rp.tables(ro.P, ro.TABLE_R, ro.BASE, dtype)
        worst = 0.0
        for n, (p, i) in enumerate(ro.TABLE_SPOTS):
            bound = ro.table_bound(p, i, ro.TABLE_R, dtype)
            for got, exact in ((cos_t[p, i], exact_c[n]), (sin_t[p, i], exact_s[n])):
                err = float(abs(np.longdouble(got) - exact))
                assert err <= bound, "table (%d, %d) %s: %.3e > %.3e" % (p, i, np.dtype(dtype).name, err, bound)
                worst = max(worst, err / bound)
        print("tables %s: worst error / bound %.3f" % (np.dtype(dtype).name, worst))
    # a float64 angle is not good enough
    i = np.arange(ro.TABLE_R // 2)
    angle64 = np.arange(ro.P, dtype=np.float64)[:, None] * (ro.BASE ** (-2.0 * i / ro.TABLE_R))[None, :]
    missed = 0.0
    for n, (p, i) in enumerate(ro.TABLE_SPOTS):
        err = float(abs(np.longdouble(np.cos(angle64[p, i])) - exact_c[n]))
        missed = max(missed, err / ro.table_bound(p, i, ro.TABLE_R, np.float64))
    assert missed > 2.0, "a float64 angle stays within the float64 table bound (%.2f): the test could not tell" % missed
    print("a float64 angle misses the float64 table bound by a factor %.1f" % missed)
    return data


def cases():
    data = {}
    for pairing in ro.PAIRINGS:
        for name, (B, T, Ha, Hb, D, R) in ro.CASES.items():
            for dtype in (np.float32, np.float64):
                cos_t, sin_t = rp.tables(ro.P, R, ro.BASE, dtype)
                xs = ro.case_input(name, dtype)
                for which, x in zip("ab", xs):
                    if x is None:
                        continue
                    for inverse in (False, True):
                        res = ro.reference(x, cos_t, sin_t, ro.GOLDEN_OFFSET, None, "bthd", pairing, inverse, dtype)
                        what = "%s %s %s %s inverse %d" % (pairing, name, which, np.dtype(dtype).name, inverse)
                        ro.assert_within(res.values, res, what + " (oracle alone)")
                        ro.assert_within(rp.rope_host(x, cos_t, sin_t, ro.GOLDEN_OFFSET, None, "bthd", pairing, inverse), res,
                                         what + " (same precision)")
                        rot = np.abs(res.values[..., :R]).astype(np.float64)
                        assert np.median(res.bounds[..., :R]) < 1e-3 * np.median(rot), what
                    if dtype == np.float32:
                        res = ro.reference(x, cos_t, sin_t, ro.GOLDEN_OFFSET, None, "bthd", pairing, False, dtype)
                        data["%s.%s.%s" % (pairing, name, which)] = res.values.astype(np.float64)
    return data


def position_shift():
    rs = np.random.RandomState(ro.case_seed("shift"))
    q, k = rs.randn(1, 9, 2, 16), rs.randn(1, 9, 2, 16)
    for pairing in ro.PAIRINGS:
        for R in (16, 10):
            cos_t, sin_t = rp.tables(64, R, ro.BASE, np.float64)
            scores = []
            for shift in (0, 5, 55):
                qr, kr = (ro.reference(a, cos_t, sin_t, shift, None, "bthd", pairing, False, np.float64).values.astype(np.float64)
                          for a in (q, k))
                scores.append(np.einsum("bihd,bjhd->bhij", qr, kr))
            for s in scores[1:]:
                assert np.abs(s - scores[0]).max() <= 1e-12, "position shift, %s R %d: %.3e" % (pairing, R, np.abs(s - scores[0]).max())


def lm_fixture():
    """The seed and the head scale of rope_oracle's two-block rotary model, chosen as tests/gen_gqa_golden.py chooses its own: the
    first seed, and the smallest power of two, at which EVERY greedy step's float64 top-2 logit margin exceeds
    2 x LM_MARGIN x lm.logit_bound, the bound being max |float32 - float64| over the last-position logits of every step with
    the float32 evaluation this package's composed route on the CPU twin."""
    from tinynn_autograd_amd import _lib
    import rope_support as rsup
    _lib.install_test_twin(conftest.build_twin())
    c = ro.LM
    for seed in range(20):
        scale = 1.0
        for _ in range(6):
            params, prompt = ro.lm_params(seed, scale), ro.lm_prompt(seed)
            ids, steps = ro.lm_generate(params, prompt, c["new"])
            net = rsup.lm_net(params, np.float32, fused=False)
            net.set_phase("TEST")
            bound = max(np.abs(rsup.lm_last_logits(net, ids[:, :c["prompt"] + n]) - steps[n]).max() for n in range(c["new"]))
            srt = np.sort(steps, axis=-1)
            margin = float((srt[..., -1] - srt[..., -2]).min())
            if margin > 2 * ro.LM_MARGIN * bound:
                print("lm: seed %d, head scale %g, top-2 margin %.3e, logit bound %.3e" % (seed, scale, margin, bound))
                return {"lm.seed": np.int64(seed), "lm.head_scale": np.float64(scale), "lm.logit_bound": np.float64(bound),
                        "lm.ids": ids}
            scale *= 2.0
    raise AssertionError("no seed gives the margin")


def main():
    data = table_spots()
    data.update(cases())
    position_shift()
    data.update(lm_fixture())
    np.savez_compressed(OUT, **data)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(data), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
