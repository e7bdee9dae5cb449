"""Writes tests/golden/dropout_cases.npz from this repository's own generator (tinynn-autograd_amd/dropout.py): per case of
CASES the input, the stream words, the keep mask and the outputs of the plain and the residual form.  The fixture pins the
generator: a later edit of it cannot silently change every seeded run (tests/test_dropout_golden.py).

    python tests/gen_dropout_golden.py
"""

import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "golden", "dropout_cases.npz")

# name -> (seed, calls, first, n, p, dtype)
CASES = {
    "zero_state": (0, 0, 0, 16, 0.5, np.float32),
    "offset_and_calls": (1234, 7, 3, 21, 0.1, np.float32),
    "wide_seed_and_calls": (2 ** 40 + 7, 2 ** 33 + 5, 0, 12, 0.9, np.float64),
    "across_the_block_carry": (7, 3, 2 ** 34 - 8, 16, 0.25, np.float64),
}


def planner():
    """dropout.py loaded from its file: numpy only, no package import and no device."""
    path = os.path.join(os.path.dirname(HERE), "tinynn-autograd_amd", "dropout.py")
    spec = importlib.util.spec_from_file_location("dropout_planner", path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def case_input(name):
    """(x, residual): small numbers exact in float16, so the fixture stores them in 2 bytes each."""
    seed, calls, first, n, p, dtype = CASES[name]
    rs = np.random.RandomState(sorted(CASES).index(name))
    x = (rs.randint(-40, 41, n) / 8.0).astype(dtype)
    x[x == 0] = dtype(0.125)
    return x, (rs.randint(-40, 41, n) / 4.0).astype(dtype)


def build(dp):
    out = {}
    for name, (seed, calls, first, n, p, dtype) in CASES.items():
        x, res = case_input(name)
        out[name + ".x"] = x.astype(np.float16)
        out[name + ".residual"] = res.astype(np.float16)
        out[name + ".words"] = dp.stream_words(seed, calls, first, n)
        out[name + ".keep"] = dp.keep_mask(seed, calls, first, n, dp.threshold_of(p))
        out[name + ".uniform"] = dp.uniform(seed, calls, first, n, dtype)
        out[name + ".y"] = dp.reference(x, seed, calls, p, first=first)
        out[name + ".y_residual"] = dp.reference(x, seed, calls, p, residual=res, first=first)
    return out


if __name__ == "__main__":
    arrays = build(planner())
    np.savez_compressed(OUT, **arrays)
    print("%s: %d arrays, %d bytes" % (OUT, len(arrays), os.path.getsize(OUT)))
