"""Writes tests/golden/gated_cases.npz: the results of gated_oracle's named cases (inputs are regenerated from seeds, not
stored), produced by this project's oracle alone.

    <name>.y / .dgate / .dup     the oracle's values for float32 inputs, as float64 (.dup only for the cases with up)

Checked here, on the CPU, for float32 AND float64: on every case a same-precision numpy evaluation (gated.gated_host /
gated_bwd_host; the erf form through math.erf) is within the derived bound, and the bound passes the median gate.

    python tests/gen_gated_golden.py
"""

import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conftest                                                             # noqa: E402,F401  (puts the repository on sys.path)
import gated_oracle as go                                                   # noqa: E402
from tinynn_autograd_amd import gated as gt                                 # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gated_cases.npz")


def same_precision(gate, up, dy, act):
    """(y, dgate, dup) with one rounding per operation in gate's dtype."""
    if act != "gelu":
        dgate, dup = gt.gated_bwd_host(gate, up, dy, act)
        return gt.gated_host(gate, up, act), dgate, dup
    t = gate.dtype.type
    erf = np.vectorize(math.erf, otypes=[np.float64])
    cdf = t(0.5) * (t(1) + erf(gate * t(math.sqrt(0.5))).astype(gate.dtype))
    pdf = t(1.0 / math.sqrt(2.0 * math.pi)) * np.exp(t(-0.5) * gate * gate)
    a, slope = gate * cdf, cdf + gate * pdf
    return a * up, (dy * up) * slope, dy * a


def main():
    data = {}
    for name, (act, M, F, with_up) in go.GOLDEN_CASES.items():
        for dtype in (np.float32, np.float64):
            gate, up, dy = go.make_inputs(M, F, go.case_seed(name), dtype)
            up = up if with_up else None
            res = go.reference(gate, up, dy, act, dtype)
            y, dgate, dup = same_precision(gate, up, dy, act)
            go.check(dict(y=y, dgate=dgate, dup=dup), res, "%s %s (same precision)" % (name, np.dtype(dtype).name), verbose=True)
            if dtype == np.float32:
                for field in ("y", "dgate", "dup"):
                    if res.values[field] is not None:
                        data["%s.%s" % (name, field)] = res.values[field].astype(np.float64)
    np.savez_compressed(OUT, **data)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(data), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
