"""Autoregressive generation from a token model: a key / value cache per attention layer and the token loop.

    cache = KVCache(max_len)                      one (k, v, length) per layer that takes `cache`, allocated from the first batch
    ids = generate(model, prompt_ids, 32)         numpy int64 [B, P + 32]

With the cache a step costs one row through every layer: the prompt runs once through the ordinary causal path (the PREFILL,
whose k and v are slice-assigned into the cache), then every new token runs three projections of ONE row per attention
layer and ops.attention_decode_ over the cached prefix — O(P + N) per layer instead of O((P + N)^2).

The loop stays on the device.  The uniform numbers u [N, B] are drawn on the host and uploaded ONCE — or, with
`generator=` (rng.Generator), filled on the device by ONE Generator.uniform call, with no host draw and no upload; every
sampled id is written into a device [B, P + N] buffer by ops.sample_rows_ and feeds the next step's Embedding as device ids; there is ONE read-back, at the end.  On the native route nothing synchronises with the host
between the first and the last new token.  (On the composed route — the CPU test twin — sample_rows reads the logits back.)

Out of scope: ragged batches (every sequence of the batch has the same length), grouped-query heads, chunked prefill (it
needs a bottom-right causal rule), top-p, bf16, graph capture of the token loop.
"""

import inspect

import numpy as np

from . import device_array as da
from .core import ops
from .core.tensor import Tensor


class LayerCache(object):
    """The keys and values of ONE attention layer: k [B, max_len, H, D], v [B, max_len, H, D] (layout "bthd": what a
    [B T, H D] projection reshapes to), allocated from the first batch, and the number of live rows."""

    def __init__(self, max_len):
        self.max_len, self.length, self.k, self.v = int(max_len), 0, None, None

    def check(self, b, t, h, d):
        """What MultiHeadAttention.forward asks BEFORE any launch."""
        if self.length == 0:
            if t > self.max_len:
                raise ValueError("KVCache: a prompt of %d tokens exceeds the cache's %d rows" % (t, self.max_len))
            return
        if t != 1:
            raise ValueError("KVCache: the cache holds %d tokens — a step takes ONE new token per sequence, got T = %d "
                             "(chunked prefill is out of scope)" % (self.length, t))
        if self.length >= self.max_len:
            raise ValueError("KVCache: the cache is full (%d of %d rows)" % (self.length, self.max_len))
        if tuple(self.k.shape) != (b, self.max_len, h, d):
            raise ValueError("KVCache: the cache was allocated for [B, H, D] = %s, got %s"
                             % ((self.k.shape[0],) + tuple(self.k.shape[2:]), (b, h, d)))

    def fill(self, k, v):
        """The prefill's k and v [B, T, H, D] (device arrays) become rows [0, T)."""
        b, t, h, d = (int(s) for s in k.shape)
        self.k = da.zeros((b, self.max_len, h, d), k.dtype)
        self.v = da.zeros((b, self.max_len, h, int(v.shape[3])), v.dtype)
        self.k[:, :t] = k
        self.v[:, :t] = v
        self.length = t


class KVCache(object):
    """One LayerCache per layer that takes `cache`, made on demand: `cache.layer(i)` is layer i's."""

    def __init__(self, max_len):
        max_len = int(max_len)
        if max_len < 1:
            raise ValueError("KVCache: max_len must be >= 1, got %d" % max_len)
        self.max_len, self.layers = max_len, {}

    def layer(self, index):
        if index not in self.layers:
            self.layers[index] = LayerCache(self.max_len)
        return self.layers[index]

    @property
    def length(self):
        return max([c.length for c in self.layers.values()] or [0])

    def reset(self):
        self.layers = {}


_TAKES = {}      # (layer class, argument name) -> bool: inspect.signature costs more than a decoding step's launches


def _takes(layer, name):
    key = (type(layer), name)
    known = _TAKES.get(key)
    if known is None:
        try:
            known = name in inspect.signature(type(layer).forward).parameters
        except (TypeError, ValueError):
            known = False
        _TAKES[key] = known
    return known


def _forward(layers, ids, offset, cache):
    """The layers one after the other with plain layer.forward (NOT Net.forward, whose TRAIN-mode head fusion must not
    engage), `offset` / `cache` handed to those that declare them."""
    x = ids
    for i, layer in enumerate(layers):
        kwargs = {}
        if offset and _takes(layer, "offset"):
            kwargs["offset"] = offset
        if cache is not None and _takes(layer, "cache"):
            kwargs["cache"] = cache.layer(i)
        x = layer.forward(x, **kwargs)
    return x


def generate(model_or_net, prompt_ids, max_new_tokens, temperature=1.0, top_k=None, u=None, seed=None, cache=True,
             generator=None):
    """Continue `prompt_ids` [B, P] (integers) by `max_new_tokens` tokens -> numpy int64 [B, P + N].

    temperature 0: greedy; otherwise token n of sequence b is the inverse CDF of softmax(logits / temperature) over the top_k
    largest (None: all) at u[n, b].  u: [N, B] numbers in [0, 1), given, or drawn from np.random.RandomState(seed).
    generator: an rng.Generator — u is then its uniform((N, B)) in the dtype of the logits, ONE device fill that consumes one
    call of the generator (stream element n B + b is u[n, b]); it excludes `u` and `seed`, and temperature 0 draws nothing.
    cache=True: a KVCache — the prompt runs once, every new token costs one row per layer.  cache=False: the whole growing
    prefix runs through the net every step — the independent route, and what the CPU test twin compares with.
    The net runs in phase TEST; the previous phase is restored.  P + N beyond an Embedding's max_len raises before any launch."""
    net = getattr(model_or_net, "net", model_or_net)
    layers = net.layers
    host = np.asarray(getattr(prompt_ids, "values", prompt_ids))
    if host.ndim != 2 or host.dtype.kind not in "iu" or host.shape[1] < 1:
        raise ValueError("generate: prompt_ids must be integers [B, P] with P >= 1, got shape %s, dtype %s" % (host.shape, host.dtype))
    B, P = (int(s) for s in host.shape)
    N = int(max_new_tokens)
    if N < 0:
        raise ValueError("generate: max_new_tokens must be >= 0, got %d" % N)
    for layer in layers:
        limit = getattr(layer, "max_len", None)
        if limit is not None and _takes(layer, "offset") and P + N > int(limit):
            raise ValueError("generate: %d prompt + %d new tokens exceed the embedding's max_len %d" % (P, N, int(limit)))
    temperature = float(temperature)
    if generator is not None and (u is not None or seed is not None):
        raise ValueError("generate: `generator` draws u on the device — it excludes `u` and `seed`")
    if temperature != 0.0 and generator is None:
        if u is None:
            u = np.random.RandomState(seed).random_sample((N, B))
        u = np.asarray(u, dtype=np.float64)
        if u.shape != (N, B) or (u.size and not (u.min() >= 0.0 and u.max() < 1.0)):
            raise ValueError("generate: u must be [N, B] = %s numbers in [0, 1), got shape %s" % ((N, B), u.shape))
    host = np.ascontiguousarray(host, dtype=np.int64)
    if N == 0 or B == 0:
        return host.copy()

    phase = model_or_net.get_phase()
    model_or_net.set_phase("TEST")
    try:
        out = da.zeros((B, P + N), np.int64)                   # every id of the run, on the device
        out[:, :P] = da.asarray(host)
        u_dev = None                                           # uploaded ONCE, in the dtype of the logits
        kv = KVCache(P + N) if cache else None
        for n in range(N):
            if cache and n > 0:
                ids, offset = out[:, P + n - 1:P + n], P + n - 1
            else:
                ids, offset = out[:, :P + n], 0
            t = int(ids.shape[1])
            logits = _forward(layers, Tensor(ids), offset, kv)
            vocab = int(logits.shape[-1])
            last = ops.getitem_(ops.reshape(logits, (B, t, vocab)), (slice(None), t - 1))
            if temperature != 0.0 and u_dev is None and generator is not None:
                u_dev = generator.uniform((N, B), last.values.dtype)       # (r 2^-24: exact in either dtype, below 1)
            elif temperature != 0.0 and u_dev is None:
                dt = last.values.dtype                         # (rounding to float32 must not produce 1.0)
                u_dev = da.asarray(np.minimum(u.astype(dt), np.nextafter(dt.type(1), dt.type(0))))
            picked = ops.sample_rows_(last, None if u_dev is None else u_dev[n], temperature=temperature, top_k=top_k)
            out[:, P + n] = picked.values
        return np.asarray(out)                                 # the ONE read-back
    finally:
        model_or_net.set_phase(phase)
