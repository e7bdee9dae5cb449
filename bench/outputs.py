"""`--dump-outputs DIR`: what the timed path handed its caller after its last timed step — that step's loss and every layer's
weight and bias — written as DIR/<name>.npy in float32, at most 64 MB in all, so that two builds run with the same arguments can
be compared output for output.  An array larger than its share of the limit is written as `<name>_sample.npy`: the same fixed,
seeded choice of its flat elements in every run."""

import os

import numpy as np

LIMIT_BYTES = 64 << 20
HEADER_BYTES = 4096                      # room left per file for the .npy header
SAMPLE_SEED = 1234


def shares(sizes, limit=LIMIT_BYTES):
    """Elements written of each array (float32): the smaller arrays whole, what is left split evenly over the larger ones."""
    left = (limit - HEADER_BYTES * len(sizes)) // 4
    keep = [0] * len(sizes)
    order = sorted(range(len(sizes)), key=lambda i: sizes[i])
    for j, i in enumerate(order):
        keep[i] = min(sizes[i], left // (len(order) - j))
        left -= keep[i]
    return keep


def sample(a, k, seed=SAMPLE_SEED):
    """k flat elements of `a`, one at a seeded position inside each of k equal stretches of it, in index order."""
    edges = np.arange(k + 1, dtype=np.int64) * a.size // k
    idx = edges[:-1] + (np.random.RandomState(seed).random_sample(k) * (edges[1:] - edges[:-1])).astype(np.int64)
    return a.reshape(-1)[idx]


def write_outputs(out_dir, named, limit=LIMIT_BYTES):
    """named: [(name, host array)] -> out_dir/<name>.npy (float32); returns the paths written."""
    os.makedirs(out_dir, exist_ok=True)
    arrays = [(name, np.asarray(a, dtype=np.float32)) for name, a in named]
    paths = []
    for (name, a), k in zip(arrays, shares([a.size for _, a in arrays], limit)):
        if k < a.size:
            name, a = name + "_sample", sample(a, k)
        path = os.path.join(out_dir, name + ".npy")
        np.save(path, np.ascontiguousarray(a))
        paths.append(path)
    return paths
