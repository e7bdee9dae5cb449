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

Ragged batches, end of sequence, graph capture.  With `prompt_lens`, `eos_id`, `capture`, `stop_every` or `return_lengths`
the per-step state moves to the device (include/tnn_ragged.h): lens[B], the current ids, the end-of-sequence flags and the
step's uniform numbers sit at fixed addresses, ops.attention_decode_ragged_ and ops.embedding_at_ read the lengths there, and
ONE small launch (device_array.ragged_advance) advances all of it.  No argument of a token step changes from step to step,
so `capture=True` records the step once (graph.capture) and replays it: one graph launch per token instead of one Python
dispatch per kernel.  Without these arguments the path above runs, bit for bit.

Grouped-query heads need no concept here: a layer built with kv_heads= calls LayerCache.check and fill with its key / value
head count and runs the grouped decode ops, whose ragged form has fixed arguments and is captured like the multi-head one.

Rotary position embeddings need none either: a layer built with rope= (a rope.Rotary) rotates q and k at offset 0 in the
prefill, at cache.length in a uniform step and at cache.lens — read on the device, at a fixed address — in a ragged step, so
the captured step stays a replay.  generate refuses P + N (ragged: Pmax + N) beyond a layer's rope.max_len before any launch.

Chunked prefill and continuation (include/tnn_extend.h).  A cache made with extend=True also takes T > 1 new tokens when
it is filled: the layer rotates them at offset cache.length and runs ops.attention_extend_, which attends over the cached
rows and the new ones (the bottom-right causal rule) and appends them in ONE launch.  generate(prefill_chunk=C) runs the
prompt as ceil(P / C) pieces — the first through the ordinary prefill, the rest through the extension — and
generate(cache=a KVCache(extend=True)) continues the sequence an earlier call left in that cache.  The default cache
refuses T > 1 on a filled cache as before.

Out of scope: ragged chunks (lengths read on the device with T > 1), top-p, bf16, and skipping the work
of sequences that have ended (they go on emitting the pad token; `stop_every` ends the loop once ALL have ended).
"""

import inspect

import numpy as np

from . import _lib
from . import device_array as da
from . import ragged as rg
from .core import ops
from .core.tensor import Tensor


class LayerCache(object):
    """The keys and values of ONE attention layer: k [B, max_len, H, D], v [B, max_len, H, D] (layout "bthd": what a
    [B T, H D] projection reshapes to), allocated from the first batch, and the number of live rows."""

    def __init__(self, max_len, lens=None, extend=False):
        self.max_len, self.length, self.k, self.v = int(max_len), 0, None, None
        self.extend = bool(extend)     # a filled cache also takes T > 1 new rows (ops.attention_extend_); False: ONE per step
        self.lens = lens     # a ragged.Lengths: every sequence's own live rows, read on the device; `length` is then the
                             # host's upper bound (what check() uses)

    def check(self, b, t, h, d):
        """What MultiHeadAttention.forward asks BEFORE any launch."""
        if self.extend and self.lens is not None:
            raise ValueError("KVCache: extend=True with per-sequence lengths (ragged extension is out of scope)")
        if self.length == 0:
            if t > self.max_len:
                raise ValueError("KVCache: a prompt of %d tokens exceeds the cache's %d rows" % (t, self.max_len))
            return
        if self.extend:
            if t < 1 or self.length + t > self.max_len:
                raise ValueError("KVCache: %d cached + %d new tokens overflow the cache's %d rows" % (self.length, t, self.max_len))
        elif t != 1:
            raise ValueError("KVCache: the cache holds %d tokens — a step takes ONE new token per sequence, got T = %d "
                             "(chunked prefill is out of scope)" % (self.length, t))
        elif self.length >= self.max_len:
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

    def __init__(self, max_len, lens=None, extend=False):
        max_len = int(max_len)
        if max_len < 1:
            raise ValueError("KVCache: max_len must be >= 1, got %d" % max_len)
        self.max_len, self.layers, self.lens, self.extend = max_len, {}, lens, bool(extend)

    def layer(self, index):
        if index not in self.layers:
            self.layers[index] = LayerCache(self.max_len, self.lens, self.extend)
        return self.layers[index]

    def set_lens(self, lens):
        """A ragged batch: every layer's decode step reads the sequences' lengths from `lens` (a ragged.Lengths) on the device."""
        self.lens = lens
        for c in self.layers.values():
            c.lens = lens

    def set_length(self, length):
        """The host's upper bound of the live rows of every layer that has been filled (generate's captured steps: a replay
        runs no Python that would count)."""
        for c in self.layers.values():
            if c.length:
                c.length = int(length)

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


def _forward(layers, ids, offset, cache, positions=None):
    """The layers one after the other with plain layer.forward (NOT Net.forward, whose TRAIN-mode head fusion must not
    engage), `offset` / `cache` / `positions` handed to those that declare them."""
    x = ids
    for i, layer in enumerate(layers):
        kwargs = {}
        if offset and _takes(layer, "offset"):
            kwargs["offset"] = offset
        if positions is not None and _takes(layer, "positions"):
            kwargs["positions"] = positions
        if cache is not None and _takes(layer, "cache"):
            kwargs["cache"] = cache.layer(i)
        x = layer.forward(x, **kwargs)
    return x


def generate(model_or_net, prompt_ids, max_new_tokens, temperature=1.0, top_k=None, u=None, seed=None, cache=True,
             generator=None, prompt_lens=None, eos_id=None, pad_id=0, capture=False, stop_every=None, return_lengths=False,
             prefill_chunk=None):
    """Continue `prompt_ids` [B, P] (integers) by `max_new_tokens` tokens -> numpy int64 [B, P + N].

    prompt_lens, eos_id, pad_id, capture, stop_every, return_lengths: the RAGGED path (_generate_ragged states them); with
    all of them at their defaults the path described here runs.

    temperature 0: greedy; otherwise token n of sequence b is the inverse CDF of softmax(logits / temperature) over the top_k
    largest (None: all) at u[n, b].  u: [N, B] numbers in [0, 1), given, or drawn from np.random.RandomState(seed).
    generator: an rng.Generator — u is then its uniform((N, B)) in the dtype of the logits, ONE device fill that consumes one
    call of the generator (stream element n B + b is u[n, b]); it excludes `u` and `seed`, and temperature 0 draws nothing.
    cache=True: a KVCache — the prompt runs once, every new token costs one row per layer.  cache=False: the whole growing
    prefix runs through the net every step — the independent route, and what the CPU test twin compares with.
    cache=a KVCache(extend=True): the caller's cache is used and kept.  Empty, it behaves as cache=True; holding L > 0 rows
    from an earlier call, prompt_ids are the NEW tokens at positions L .. L + P - 1 — they run through the extension
    (ops.attention_extend_) — the result is still [B, P + N], and nothing new is allocated for the cache.  Either way it is
    left at L + P + N - 1 rows, and L + P + N must fit its max_len, the embedding's and the rotary tables'.
    prefill_chunk=C (an integer >= 1; this path only, with a cache): the prompt runs as ceil(P / C) pieces — the first through
    the ordinary prefill (the extension when L > 0), the rest through the extension at the offset of the rows already cached;
    the pieces before the last stop behind the last layer that takes the cache, so only the last piece reaches the head.
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
    ragged = prompt_lens is not None or eos_id is not None or capture or stop_every is not None or return_lengths
    kept = cache if isinstance(cache, KVCache) else None       # the caller's cache: continued, and left to the caller
    if kept is not None:
        if ragged:
            raise ValueError("generate: a kept KVCache continues the uniform path — it excludes prompt_lens, eos_id, capture, "
                             "stop_every and return_lengths")
        if not kept.extend or kept.lens is not None:
            raise ValueError("generate: cache= takes True, False or a KVCache(extend=True) without per-sequence lengths")
        if any(c.k is not None and int(c.k.shape[0]) != B for c in kept.layers.values()):
            raise ValueError("generate: the kept KVCache was filled by a batch of another size than B = %d" % B)
    L = kept.length if kept is not None else 0                 # the rows an earlier call left in the cache
    if prefill_chunk is not None:
        if isinstance(prefill_chunk, bool) or not isinstance(prefill_chunk, (int, np.integer)) or prefill_chunk < 1:
            raise ValueError("generate: prefill_chunk must be an integer >= 1, got %r" % (prefill_chunk,))
        if ragged or not cache:
            raise ValueError("generate: prefill_chunk cuts the prompt of the uniform cached path — it excludes cache=False, "
                             "prompt_lens, eos_id, capture, stop_every and return_lengths")
    past = "" if L == 0 else "%d cached + " % L
    for layer in layers:
        limit = getattr(layer, "max_len", None)
        if limit is not None and _takes(layer, "offset") and L + P + N > int(limit):
            raise ValueError("generate: %s%d prompt + %d new tokens exceed the embedding's max_len %d" % (past, P, N, int(limit)))
        rotary = getattr(layer, "rope", None)                  # (a MultiHeadAttention's or a TransformerBlock's Rotary)
        if rotary is not None and L + P + N > int(rotary.max_len):
            raise ValueError("generate: %s%d prompt + %d new tokens exceed the rotary tables' max_len %d"
                             % (past, P, N, int(rotary.max_len)))
    if kept is not None and L + P + N > kept.max_len:
        raise ValueError("generate: %s%d prompt + %d new tokens exceed the cache's max_len %d" % (past, P, N, kept.max_len))
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
    if ragged:
        return _generate_ragged(model_or_net, layers, host, N, temperature, top_k, u, cache, generator, prompt_lens, eos_id,
                                pad_id, capture, stop_every, return_lengths)
    if N == 0 or B == 0:
        return host.copy()

    phase = model_or_net.get_phase()
    model_or_net.set_phase("TEST")
    try:
        out = da.zeros((B, P + N), np.int64)                   # every id of the run, on the device
        out[:, :P] = da.asarray(host)
        u_dev = None                                           # uploaded ONCE, in the dtype of the logits
        kv = kept if kept is not None else KVCache(P + N, extend=prefill_chunk is not None) if cache else None
        for n in range(N):
            if cache and n > 0:
                ids, offset = out[:, P + n - 1:P + n], L + P + n - 1
            else:
                ids, offset = out[:, :P + n], L
            if cache and n == 0 and prefill_chunk is not None and prefill_chunk < P:
                # the pieces before the last fill the cache and stop behind the last layer that takes it
                body = 1 + max([i for i, layer in enumerate(layers) if _takes(layer, "cache")] or [-1])
                first = (P - 1) // prefill_chunk * prefill_chunk           # where the last piece starts
                for s0 in range(0, first, prefill_chunk):
                    _forward(layers[:body], Tensor(out[:, s0:s0 + prefill_chunk]), L + s0, kv)
                ids, offset = out[:, first:P], L + first
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


def _generate_ragged(model_or_net, layers, host, N, temperature, top_k, u, cache, generator, prompt_lens, eos_id, pad_id,
                     capture, stop_every, return_lengths):
    """generate() for a ragged batch, with an end-of-sequence token and (optionally) a captured token step.

    prompt_ids [B, Pmax] is right-padded; prompt_lens [B] with 1 <= P_b <= Pmax (None: every sequence has Pmax tokens); what
    the prompt holds at and beyond P_b does not matter (it is never uploaded).  The result is [B, Pmax + N], initialised with
    pad_id: row b holds its prompt, its N new tokens — pad_id after an eos_id — and Pmax - P_b trailing pads.
    return_lengths: also [B] lengths, the prompt plus the new tokens up to and including eos_id (from the ids, on the host).

    The padded prompt runs ONCE through the ordinary causal path (position i sees keys <= i alone, so no mask is needed; cache
    rows at and beyond P_b hold garbage that decode never reads and overwrites one by one as lens[b] grows); the logits of
    position P_b - 1 are gathered per sequence.  A step is embedding_at_(cur, lens), the blocks, the head, sample_rows_(logits,
    u_cur) and ragged_advance — every operand at a fixed address.  u [N, B] is uploaded (or filled by `generator`) once, so
    equal u gives the tokens of the uniform path at uniform lengths.  cache=False: the whole growing prefix runs each step,
    with the same gather.

    capture=True (native route, cache=True): after the prefill and one eager step the step is recorded by
    graph.capture(step, warmup=1) and replayed for the remaining tokens; the host follows the lengths itself.  Fewer steps
    left than that takes: they run eagerly.  Measured on one MI355X (profiles/ragged_generation.txt, DESIGN section 4d:
    width 128, 2 blocks, batch 8, prompt 32, 224 new tokens): 80.4 k tokens/s captured against 26.3 k eager and 25.6 k for
    the uniform path — 3.1x; the recording is inside that time.  The default stays False.
    stop_every=k: `done` is read back every k steps — the loop's only synchronisation — and the loop ends once every sequence
    has ended; it works between replays too."""
    B, Pmax = (int(s) for s in host.shape)
    if prompt_lens is None:
        start = np.full(B, Pmax, dtype=np.int64)
    else:
        start = np.asarray(prompt_lens)
        if start.shape != (B,) or start.dtype.kind not in "iu" or (B and not (start.min() >= 1 and start.max() <= Pmax)):
            raise ValueError("generate: prompt_lens must be integers [B] = (%d,) in [1, %d], got %r" % (B, Pmax, prompt_lens))
        start = start.astype(np.int64)
    eos = -1 if eos_id is None else int(eos_id)
    pad = int(pad_id)
    if eos_id is not None and eos < 0:
        raise ValueError("generate: eos_id must be >= 0, got %d" % eos)
    if stop_every is not None and int(stop_every) < 1:
        raise ValueError("generate: stop_every must be >= 1, got %r" % (stop_every,))
    if capture and not cache:
        raise ValueError("generate: capture=True records the cached token step — it needs cache=True")
    Tout = Pmax + N
    ids = np.full((B, Tout), pad, dtype=np.int64)
    for b in range(B):
        ids[b, :start[b]] = host[b, :start[b]]

    def result(arr):
        return (arr, rg.generated_lengths(arr, start, N, eos)) if return_lengths else arr

    if N == 0 or B == 0:
        return result(ids)
    if capture and (not _lib.get().has_ragged or da.RAGGED_ROUTE == "composed" or da.DECODE_ROUTE == "composed"
                    or any(getattr(layer, "fused", True) is False for layer in layers)):
        raise ValueError("generate: capture=True needs the native route (libtnn_hip.so and fused layers): the composed route "
                         "reads values back to the host, which a graph capture cannot do")

    phase = model_or_net.get_phase()
    model_or_net.set_phase("TEST")
    try:
        out = da.asarray(ids)                                  # every id of the run, on the device
        lens = da.lengths(start - 1)                           # the position of every sequence's LAST token
        start_d, done, cur = da.asarray(start), da.zeros((B,), np.int64), da.zeros((B,), np.int64)
        kv = KVCache(Tout, lens) if cache else None
        arange = np.arange(B, dtype=np.int64)

        def last_rows(logits, t):
            """logits [B t, V] -> the row of every sequence's last token, [B, V]: a device-indexed gather."""
            vocab = int(logits.shape[-1])
            return ops.getitem_(ops.reshape(logits, (B * t, vocab)), da.asarray(arange * t + lens.host))

        # ---- the prefill (cache=False: the first of N whole-prefix forwards)
        last = last_rows(_forward(layers, Tensor(out[:, :Pmax]), 0, kv), Pmax)
        dt = last.values.dtype
        u_all = u_cur = None
        if temperature != 0.0:
            if generator is not None:
                u_all = generator.uniform((N, B), dt)          # (r 2^-24: exact in either dtype, below 1)
            else:                                              # (rounding to float32 must not produce 1.0)
                u_all = da.asarray(np.minimum(u.astype(dt), np.nextafter(dt.type(1), dt.type(0))))
            u_cur = da.zeros((B,), dt)
            u_cur[...] = u_all[0]

        def advance(picked):
            da.ragged_advance(picked.values, lens, start_d, done, out, cur, u_all, u_cur, eos=eos_id, pad=pad)

        advance(ops.sample_rows_(last, u_cur, temperature=temperature, top_k=top_k))
        cur_ids = Tensor(cur.reshape(B, 1))

        def step():
            logits = _forward(layers, cur_ids, 0, kv, positions=lens)
            advance(ops.sample_rows_(ops.reshape(logits, (B, int(logits.shape[-1]))), u_cur, temperature=temperature,
                                     top_k=top_k))

        def step_uncached(n):
            t = Pmax + n
            advance(ops.sample_rows_(last_rows(_forward(layers, Tensor(out[:, :t]), 0, None), t), u_cur,
                                     temperature=temperature, top_k=top_k))

        def follow(n):
            """After new token n (0-based) exists: the host's view of the state (a replay runs no Python that would count)."""
            lens.host[:] = start + n
            if kv is not None:
                kv.set_length(Pmax + n)

        every = None if stop_every is None else int(stop_every)

        def all_done(n):
            return every is not None and (n + 1) % every == 0 and bool(np.asarray(done).all())

        n, replay = 1, None                                    # n: the new tokens that exist
        stopped = all_done(0)
        while n < N and not stopped:
            if not cache:
                step_uncached(n)
            elif capture and replay is None and N - n >= 3:    # one eager step, one warm-up step, at least one replay
                from . import graph
                step()
                follow(n)
                n += 1
                replay = graph.capture(step, warmup=1)         # (the warm-up is a real step; the recording runs nothing)
            elif replay is not None:
                replay()
            else:
                step()
            follow(n)
            stopped = all_done(n)
            n += 1
        return result(np.asarray(out))                         # the ONE read-back (besides stop_every's)
    finally:
        model_or_net.set_phase(phase)
