"""Layers with the reference's API (reference: core/layers.py:10-98): `Dense` with lazy fan-in inference and the
`ReLU` / `Sigmoid` / `Tanh` activations.

Device-side differences: `Dense.forward` issues ONE GEMM with a bias epilogue (ops.dense_) instead of a matmul
node plus a broadcast-add node (`fused=False` restores the literal `inputs @ w + b`, core/layers.py:49);
`Sigmoid` is a single fused kernel (the reference's raises on a Tensor).  The parameter dict order is
"w" then "b" (core/layers.py:35): the optimizer's flatten order and the trainer's arena layout depend on it.

Not in the reference: `Conv2D`, `MaxPool2D` and `Flatten` (NCHW; ops.conv2d_ / ops.max_pool2d_), enough for a LeNet, and
`MultiHeadAttention` (ops.attention_), whose parameter dict order is MHA_PARAM_ORDER; `LayerNorm` / `RMSNorm`
(ops.layer_norm_ / ops.rms_norm_; "gamma" then "beta"), `GELU`, and `TransformerBlock`, a pre-norm block built from them whose
ONE flat parameter dict has the order BLOCK_PARAM_ORDER; `Embedding` (ops.embedding_; "tok" then "pos", EMBED_PARAM_ORDER);
`Dropout` (ops.dropout_), the one layer that reads the TRAIN / TEST flag, and the `dropout` argument of `TransformerBlock` and
`Embedding`; `SiLU` (ops.silu_) and the gated feed-forward `TransformerBlock(mlp="swiglu" | "geglu")` (ops.gated_).
"""

from . import ops
from .initializer import ConstantInit
from .initializer import NormalInit
from .initializer import XavierUniformInit
from .initializer import ZerosInit

PARAM_ORDER = ("w", "b")
MHA_PARAM_ORDER = ("wq", "bq", "wk", "bk", "wv", "bv", "wo", "bo")
NORM_PARAM_ORDER = ("gamma", "beta")
EMBED_PARAM_ORDER = ("tok", "pos")
BLOCK_PARAM_ORDER = (("ln1.gamma", "ln1.beta") + tuple("attn." + name for name in MHA_PARAM_ORDER)
                     + ("ln2.gamma", "ln2.beta", "fc1.w", "fc1.b", "fc2.w", "fc2.b"))


class Layer(object):
    """Base class: a name, a parameter dict (empty for activations) and the TRAIN/TEST flag (core/layers.py:21-22, SURVEY F8;
    nobody reads it in the reference — here dropout does)."""

    def __init__(self, name):
        self.name = name
        self.params = {}
        self.grads = {}
        self.is_training = True

    def forward(self, inputs):
        raise NotImplementedError

    def set_phase(self, phase):
        self.is_training = (phase == "TRAIN")


class Dense(Layer):
    """y = x w + b with w: [num_in, num_out], b: [1, num_out].  num_in may be omitted and is then read off the
    first batch (core/layers.py:43-57)."""

    def __init__(self, num_out, num_in=None, w_init=XavierUniformInit(), b_init=ZerosInit(), fused=True):
        super().__init__("Linear")
        self.fused = fused
        self.initializers = dict(zip(PARAM_ORDER, (w_init, b_init)))
        self.shapes = {"w": [num_in, num_out], "b": [1, num_out]}
        self.params = dict.fromkeys(PARAM_ORDER)
        self.inputs = None
        self.is_init = False
        if num_in is not None:
            self._init_parameters(num_in)

    def _init_parameters(self, input_size):
        """Draw the parameters (host RNG, w before b — only w consumes random numbers) and upload them."""
        self.shapes["w"][0] = input_size
        for name in PARAM_ORDER:
            tensor = self.initializers[name](shape=self.shapes[name])
            tensor.zero_grad()
            self.params[name] = tensor
        self.is_init = True

    def forward(self, inputs, relu=False, head_w=None, lazy=False, head_b=None):
        """relu=True is passed by Net.forward when the next layer is a ReLU: one launch for both (ops.dense_); head_w / lazy:
        the classifier-head arrangements of Net.forward (ops.dense_)."""
        if not self.is_init:
            self._init_parameters(inputs.shape[1])
        self.inputs = inputs                     # kept like the reference does (core/layers.py:48)
        w, b = (self.params[name] for name in PARAM_ORDER)
        if not self.fused:
            out = inputs @ w + b
            return ops.clip(out, 0.0) if relu else out
        return ops.dense_(inputs, w, b, relu=relu, head_w=head_w, lazy=lazy, head_b=head_b)


class Activation(Layer):
    """Parameter-free layer applying `func` (core/layers.py:60-72)."""

    def __init__(self, name):
        super().__init__(name)
        self.inputs = None

    def func(self, x):
        raise NotImplementedError

    def forward(self, inputs):
        self.inputs = inputs
        return self.func(inputs)


class ReLU(Activation):
    """clip(x, 0.0): the vjp mask is x >= 0, i.e. gradient 1 AT zero (core/layers.py:97-98, core/ops.py:338)."""

    def __init__(self):
        super().__init__("ReLU")

    def func(self, x):
        return ops.clip(x, 0.0)


class Sigmoid(Activation):
    """1 / (1 + exp(-x)) as one kernel; vjp = s (1 - s)."""

    def __init__(self):
        super().__init__("Sigmoid")

    def func(self, x):
        return ops.sigmoid_(x)


class Tanh(Activation):
    """The reference's formula verbatim in meaning: (1 - e^-x) / (1 + e^-x), which is tanh(x / 2), not tanh(x)
    (core/layers.py:88-89) — reproduced, not corrected."""

    def __init__(self):
        super().__init__("Tanh")

    def func(self, x):
        decay = ops.exp(-x)
        return (1.0 - decay) / (1.0 + decay)


class Conv2D(Layer):
    """2-D convolution over NCHW batches.  `kernel = (KH, KW, C_in, F)` in the upstream framework's order; the weight is
    STORED as [F, C_in, KH, KW] (what the kernels read, and the order for which initializer.get_fans gives fan-in =
    C_in KH KW and fan-out = F), the bias as [F].  C_in may be None and is then read off the first batch.  `fused=False`
    runs the composed route (a loop over the filter taps on the generic array operations) and a separate ReLU."""

    def __init__(self, kernel, stride=1, padding=0, w_init=XavierUniformInit(), b_init=ZerosInit(), fused=True):
        super().__init__("Conv2D")
        if len(kernel) != 4:
            raise ValueError("Conv2D: kernel must be (KH, KW, C_in, F), got %r" % (kernel,))
        kh, kw, c_in, f = kernel
        self.fused = fused
        self.stride, self.padding = stride, padding
        self.initializers = dict(zip(PARAM_ORDER, (w_init, b_init)))
        self.shapes = {"w": [int(f), c_in, int(kh), int(kw)], "b": [int(f)]}
        self.params = dict.fromkeys(PARAM_ORDER)
        self.inputs = None
        self.is_init = False
        if c_in is not None:
            self._init_parameters(int(c_in))

    def _init_parameters(self, channels):
        self.shapes["w"][1] = channels
        for name in PARAM_ORDER:
            tensor = self.initializers[name](shape=self.shapes[name])
            tensor.zero_grad()
            self.params[name] = tensor
        self.is_init = True

    def forward(self, inputs, relu=False):
        """relu=True is passed by Net.forward when the next layer is a ReLU: one launch for both (ops.conv2d_)."""
        if len(inputs.shape) != 4:
            raise ValueError("Conv2D: the input must be [N, C, H, W], got shape %s" % (tuple(inputs.shape),))
        if not self.is_init:
            self._init_parameters(int(inputs.shape[1]))
        self.inputs = inputs
        w, b = (self.params[name] for name in PARAM_ORDER)
        if self.fused:
            return ops.conv2d_(inputs, w, b, self.stride, self.padding, relu=relu)
        out = ops.conv2d_(inputs, w, b, self.stride, self.padding, route="composed")
        return ops.clip(out, 0.0) if relu else out


class MaxPool2D(Layer):
    """Max pooling over `pool_size` windows (integer or pair); stride None = the window; padding is -inf (ops.max_pool2d_:
    the first maximum of a window in row-major order receives its gradient)."""

    def __init__(self, pool_size, stride=None, padding=0):
        super().__init__("MaxPool2D")
        self.pool_size, self.stride, self.padding = pool_size, stride, padding
        self.inputs = None

    def forward(self, inputs):
        self.inputs = inputs
        return ops.max_pool2d_(inputs, self.pool_size, self.stride, self.padding)


class Flatten(Layer):
    """[N, ...] -> [N, prod(...)]: the batch axis is kept (ops.flatten_ ravels it away too)."""

    def __init__(self):
        super().__init__("Flatten")
        self.inputs = None

    def forward(self, inputs):
        self.inputs = inputs
        return ops.reshape(inputs, (int(inputs.shape[0]), -1))


class MultiHeadAttention(Layer):
    """Multi-head self-attention over [B, T, E] inputs: three projections to queries, keys and values, `num_heads` heads of
    E / num_heads dimensions each, softmax(q k^T / sqrt(E / num_heads)) v per head (causal=True: position i attends to
    positions <= i), and an output projection back to E.

    Parameters: "wq", "bq", "wk", "bk", "wv", "bv", "wo", "bo" (w: [E, E], b: [1, E]), created and stored in THAT order —
    the optimizer's flatten order depends on it, as it depends on "w" then "b" for Dense.  E (`num_in`) may be omitted and
    is then read off the first batch.

    Forward: [B T, E] rows -> three ops.dense_ -> [B, T, H, E / H] by reshape alone -> ops.attention_(layout="bthd"), whose
    kernels take strides, so nothing is transposed -> [B T, E] -> the output projection -> [B, T, E].  `fused=False` runs
    the attention on the composed route (batched products, exp and sums on the generic array operations).

    kv_heads (grouped-query attention): a divisor Hkv of num_heads — the keys and values have Hkv heads, query head h attends
    over key / value head h // (num_heads / Hkv); Hkv == 1 is multi-query attention.  "wk" and "wv" are then
    [E, Hkv E / num_heads] and "bk", "bv" [1, Hkv E / num_heads]; the parameter order and the order of host RNG draws are
    unchanged.  Training runs ops.attention_gqa_, the cached path keeps Hkv heads in its LayerCache — num_heads / Hkv times
    fewer bytes per token step — and runs ops.attention_decode_gqa_ / ops.attention_decode_ragged_gqa_.  None (the default)
    is the multi-head path as it was, launch for launch; kv_heads == num_heads computes the same through the grouped ops.

    rope (a rope.Rotary; one may be shared by every layer of a model): q and k are rotated by ONE ops.rope_ launch after the
    projections and before the attention op; v is never rotated and the key stored in a cache is the rotated one.  Positions:
    0 .. T - 1 without a cache and in the prefill, cache.length in a uniform decoding step, cache.lens — read on the device —
    in a ragged one.  Positions beyond rope.max_len raise before any launch.  None (the default): no rotation, the layer as it
    was, launch for launch."""

    def __init__(self, num_heads, num_in=None, causal=False, w_init=XavierUniformInit(), b_init=ZerosInit(), fused=True,
                 kv_heads=None, rope=None):
        super().__init__("MultiHeadAttention")
        self.rope = rope
        num_heads = int(num_heads)
        if num_heads < 1:
            raise ValueError("MultiHeadAttention: num_heads must be >= 1, got %r" % (num_heads,))
        if kv_heads is not None:
            kv_heads = int(kv_heads)
            if kv_heads < 1 or num_heads % kv_heads != 0:
                raise ValueError("MultiHeadAttention: kv_heads must be a divisor of num_heads = %d, got %r" % (num_heads, kv_heads))
        self.kv_heads = kv_heads
        self.num_heads, self.causal, self.fused = num_heads, bool(causal), fused
        self.initializers = {name: (w_init if name[0] == "w" else b_init) for name in MHA_PARAM_ORDER}
        self.shapes = {name: ([num_in, num_in] if name[0] == "w" else [1, num_in]) for name in MHA_PARAM_ORDER}
        self.params = dict.fromkeys(MHA_PARAM_ORDER)
        self.inputs = None
        self.is_init = False
        if num_in is not None:
            self._init_parameters(int(num_in))

    def _init_parameters(self, width):
        if width % self.num_heads != 0:
            raise ValueError("MultiHeadAttention: the input width %d is not a multiple of num_heads = %d"
                             % (width, self.num_heads))
        kv_width = width if self.kv_heads is None else width // self.num_heads * self.kv_heads
        for name in MHA_PARAM_ORDER:                 # host RNG in parameter order: wq, wk, wv, wo draw, the biases do not
            cols = kv_width if name[1] in "kv" else width
            self.shapes[name] = [width, cols] if name[0] == "w" else [1, cols]
            tensor = self.initializers[name](shape=self.shapes[name])
            tensor.zero_grad()
            self.params[name] = tensor
        self.is_init = True

    def forward(self, inputs, cache=None, lens=None):
        """lens (training over a right-padded batch): a ragged.Lengths or a dense int64 device array [B] — sequence b has
        lens[b] live tokens; the attention op gets it (ops.attention_: live rows attend over live keys only, dead rows come
        out as +0 before the output projection, padding is never read on the native route).  Not with a cache.  None: today's
        path, launch for launch.
        cache: a generation.LayerCache (inference).  Empty: the PREFILL — the ordinary causal path runs and its k and v
        [B, T, H, E / H] are slice-assigned into the cache; afterwards T must be 1: three projections of the one row,
        ops.attention_decode_ with the append, the output projection.  A cache with `lens` set (a ragged batch) takes
        ops.attention_decode_ragged_, which reads every sequence's length on the device; cache.length stays the host's upper
        bound.  None: today's path, bit for bit.  With kv_heads the cache holds the key / value heads and the grouped ops run
        in the same places.  A cache made with extend=True also takes T > 1 when it is filled (chunked prefill, a continued
        sequence): q and k are rotated at offset cache.length and ONE ops.attention_extend_ attends over the cached rows and
        the new ones and appends them; T == 1 keeps taking the decode ops."""
        if len(inputs.shape) != 3:
            raise ValueError("MultiHeadAttention: the input must be [B, T, E], got shape %s" % (tuple(inputs.shape),))
        if lens is not None and cache is not None:
            raise ValueError("MultiHeadAttention: lens= (training over a padded batch) and cache= (generation) do not go "
                             "together; a ragged generation batch keeps its lengths in the cache")
        b, t, e = (int(s) for s in inputs.shape)
        if not self.is_init:
            self._init_parameters(e)
        if e != self.shapes["wq"][0]:
            raise ValueError("MultiHeadAttention: the input width %d differs from the layer's %d" % (e, self.shapes["wq"][0]))
        p, h = self.params, self.num_heads
        hk = h if self.kv_heads is None else self.kv_heads       # the heads of k, v and the cache
        route = None if self.fused else "composed"
        if cache is not None:
            if not self.causal:
                raise ValueError("MultiHeadAttention: a key / value cache needs causal=True (a non-causal layer's earlier "
                                 "positions would depend on later tokens)")
            cache.check(b, t, hk, e // h)                # raises before any launch: a full cache, T > 1 after the prefill
        if self.rope is not None:
            self._check_rope(t, cache)                   # likewise: positions beyond the rotary tables
        self.inputs = inputs
        rows = ops.reshape(inputs, (b * t, e))
        grouped = self.kv_heads is not None
        if cache is not None and cache.length > 0 and t > 1:     # (cache.check let it pass: a cache made with extend=True)
            q, k, v = (ops.reshape(ops.dense_(rows, p["w" + n], p["b" + n]), (b, t, h if n == "q" else hk, e // h))
                       for n in "qkv")
            if self.rope is not None:                            # the new rows sit at the cache rows they are appended to
                q, k = ops.rope_(q, k, rotary=self.rope, offset=cache.length, route=route)
            att = ops.attention_extend_(q, cache.k, cache.v, cache.length, k, v, layout="bthd", route=route)
            cache.length += t
        elif cache is not None and cache.length > 0:
            q, k, v = (ops.reshape(ops.dense_(rows, p["w" + n], p["b" + n]), (b, h if n == "q" else hk, e // h)) for n in "qkv")
            if self.rope is not None:                            # the step's row sits at the cache row it is appended to
                where = (dict(positions=cache.lens) if getattr(cache, "lens", None) is not None
                         else dict(offset=cache.length))
                q, k = ops.rope_(ops.reshape(q, (b, 1, h, e // h)), ops.reshape(k, (b, 1, hk, e // h)), rotary=self.rope,
                                 route=route, **where)
                q, k = ops.reshape(q, (b, h, e // h)), ops.reshape(k, (b, hk, e // h))
            if getattr(cache, "lens", None) is not None:         # a ragged batch: the lengths are read on the device
                decode = ops.attention_decode_ragged_gqa_ if grouped else ops.attention_decode_ragged_
                att = decode(q, cache.k, cache.v, cache.lens, k, v, layout="bthd", route=route)
            else:
                decode = ops.attention_decode_gqa_ if grouped else ops.attention_decode_
                att = decode(q, cache.k, cache.v, cache.length, k, v, layout="bthd", route=route)
            cache.length += 1
        else:
            q, k, v = (ops.reshape(ops.dense_(rows, p["w" + n], p["b" + n]), (b, t, h if n == "q" else hk, e // h))
                       for n in "qkv")
            if self.rope is not None:
                q, k = ops.rope_(q, k, rotary=self.rope, route=route)
            if grouped:
                att = ops.attention_gqa_(q, k, v, causal=self.causal, route=route, lens=lens)
            else:
                att = ops.attention_(q, k, v, causal=self.causal, layout="bthd", route=route, lens=lens)
            if cache is not None:
                cache.fill(k.values, v.values)
        out = ops.dense_(ops.reshape(att, (b * t, e)), p["wo"], p["bo"])
        return ops.reshape(out, (b, t, e))

    def _check_rope(self, t, cache):
        """The positions of this call against rope.max_len, on the host, before any launch."""
        limit = self.rope.max_len
        if cache is None or cache.length == 0:
            first, last = 0, t - 1
        elif getattr(cache, "lens", None) is not None:
            host = cache.lens.host
            first, last = (int(host.min()), int(host.max())) if host.size else (0, 0)
        else:
            first, last = cache.length, cache.length + t - 1
        if first < 0 or last >= limit:
            raise ValueError("MultiHeadAttention: positions %d .. %d lie outside the rotary tables' max_len %d"
                             % (first, last, limit))


class LayerNorm(Layer):
    """Layer normalisation over the LAST axis of inputs of any rank >= 1: (x - mean) / sqrt(var + eps) * gamma + beta with
    the biased variance.  Parameters: "gamma" (ones) then "beta" (zeros), shape [1, N], created and stored in THAT order.  N
    (`num_in`) may be omitted and is then read off the first batch's last axis.  `fused=False` runs the composed route (sums,
    products and a square root on the generic array operations)."""
    KIND, NAMES = "layer", NORM_PARAM_ORDER

    def __init__(self, num_in=None, eps=1e-5, fused=True):
        super().__init__(type(self).__name__)
        self.eps, self.fused = float(eps), fused
        self.initializers = {"gamma": ConstantInit(1.0), "beta": ZerosInit()}
        self.shapes = {name: [1, num_in] for name in self.NAMES}
        self.params = dict.fromkeys(self.NAMES)
        self.inputs = None
        self.is_init = False
        if num_in is not None:
            self._init_parameters(int(num_in))

    def _init_parameters(self, width):
        if width < 1:
            raise ValueError("%s: the normalised axis must hold at least one element, got %d" % (self.name, width))
        for name in self.NAMES:                      # (constants: no draw from the host RNG)
            self.shapes[name] = [1, width]
            tensor = self.initializers[name](shape=self.shapes[name])
            tensor.zero_grad()
            self.params[name] = tensor
        self.is_init = True

    def forward(self, inputs):
        if len(inputs.shape) < 1:
            raise ValueError("%s: the input needs at least one axis, got a scalar" % self.name)
        width = int(inputs.shape[-1])
        if not self.is_init:
            self._init_parameters(width)
        if width != self.shapes["gamma"][1]:
            raise ValueError("%s: the input width %d differs from the layer's %d" % (self.name, width, self.shapes["gamma"][1]))
        self.inputs = inputs
        route = None if self.fused else "composed"
        if self.KIND == "layer":
            return ops.layer_norm_(inputs, self.params["gamma"], self.params["beta"], eps=self.eps, route=route)
        return ops.rms_norm_(inputs, self.params["gamma"], eps=self.eps, route=route)


class RMSNorm(LayerNorm):
    """RMS normalisation over the LAST axis: x / sqrt(mean(x^2) + eps) * gamma.  One parameter, "gamma" (ones, [1, N]);
    otherwise as LayerNorm."""
    KIND, NAMES = "rms", ("gamma",)


class GELU(Activation):
    """GELU.  approximate="none": 0.5 x (1 + erf(x / sqrt(2))) — needs the native library; "tanh": the tanh form, which also
    has a composed route."""

    def __init__(self, approximate="none"):
        super().__init__("GELU")
        from ..norm import gelu_form
        self.approximate = gelu_form(approximate)

    def func(self, x):
        return ops.gelu_(x, approximate=self.approximate)


class SiLU(Activation):
    """SiLU (swish): x sigmoid(x), one launch forward and one backward (ops.silu_; `fused=False`: the composed route)."""

    def __init__(self, fused=True):
        super().__init__("SiLU")
        self.fused = fused

    def func(self, x):
        return ops.silu_(x, route=None if self.fused else "composed")


MLP_FORMS = {"gelu": None, "swiglu": "silu", "geglu": "gelu_tanh"}     # TransformerBlock(mlp=) -> the act of ops.gated_


def _check_rate(p):
    from ..dropout import threshold_of
    threshold_of(p)                          # ValueError outside [0, 1)
    return float(p)


class Dropout(Layer):
    """Dropout with rate `p`: in the TRAIN phase every element is zeroed with probability p and the kept ones are scaled by
    1 / (1 - p); in the TEST phase (`is_training` False) and for p == 0 the layer is the identity and launches nothing.  The
    mask comes from `generator` (rng.Generator; None: rng.default_generator — seed it with rng.manual_seed) and is never
    stored: the backward launch regenerates it.  `fused=False` runs the composed route (a host-drawn mask, the existing
    multiply and masked select), which cannot be captured into a graph."""

    def __init__(self, p=0.5, generator=None, fused=True):
        super().__init__("Dropout")
        self.p, self.generator, self.fused = _check_rate(p), generator, fused
        self.inputs = None

    def active(self):
        return self.is_training and self.p > 0.0

    def forward(self, inputs, residual=None):
        """residual: a tensor of the input's shape that is added to the result by the same launch (the identity cases add it
        through the ordinary add)."""
        self.inputs = inputs
        if not self.active():
            return inputs if residual is None else residual + inputs
        return ops.dropout_(inputs, self.p, residual, generator=self.generator, route=None if self.fused else "composed")


class TransformerBlock(Layer):
    """Pre-norm transformer block over [B, T, E] inputs:

        h   = x + MHA(LN1(x))                                  `num_heads` heads, causal=True: position i attends to <= i
        out = h + GELU(LN2(h) W1 + b1) W2 + b2                 W1: [E, hidden], W2: [hidden, E]; hidden defaults to 4 E

    GELU is the tanh form (the one with a composed route, so the block also runs without the native library).  The block owns
    its parts (`ln1`, `attn`, `ln2`, `fc1`, `fc2`) and exposes ONE flat parameter dict in the order BLOCK_PARAM_ORDER:
    ln1.gamma ln1.beta, attn.wq attn.bq attn.wk attn.bk attn.wv attn.bv attn.wo attn.bo, ln2.gamma ln2.beta, fc1.w fc1.b,
    fc2.w fc2.b.  The parameters are created — and the host RNG is drawn from — in that order, so Net.get_parameters, the
    optimizer's flatten order and Model.step see the block as one layer.  The dict is what counts: every forward hands its
    tensors to the parts, so Net.set_parameters works unchanged.  E (`num_in`) may be omitted and is then read off the first
    batch.  `fused=False` puts every part on its composed route.

    dropout > 0: h = x + drop(MHA(LN1(x))) and out = h + drop(MLP(LN2(h))) in the TRAIN phase, both through the fused residual
    form of ops.dropout_ — its launch REPLACES the block's residual add — drawing from `generator` (None: the default
    generator of rng.py).  With dropout == 0 (the default) and in the TEST phase the block runs exactly its launches without
    the argument.  kv_heads: handed to the attention part (grouped-query attention; None: multi-head, as it was).  rope: a
    rope.Rotary handed to the attention part (rotary position embedding of q and k; None: no rotation, as it was).

    mlp: "gelu" (the default) is the feed-forward above, launch for launch as it was.  "swiglu" / "geglu" is the GATED form

        out = h + (act(LN2(h) Wg + bg) * (LN2(h) Wu + bu)) W2 + b2         act: silu ("swiglu") or the tanh GELU ("geglu")

    with Wg and Wu held as ONE fc1.w [E, 2 hidden] — the gate columns, then the up columns — and fc1.b [1, 2 hidden]: one
    GEMM for both projections, then the packed ops.gated_ (one launch forward; one backward that writes the packed dz, so fc1's
    backward is one GEMM too), then fc2 [hidden, E].  BLOCK_PARAM_ORDER, the parameter names and the order of host-RNG draws
    are unchanged; only fc1's shapes differ.  hidden defaults to 4 E for "gelu" and to 8 E / 3 rounded up to a multiple of 8
    for the gated forms (gated.gated_hidden), which keeps the parameter count about the same."""

    def __init__(self, num_heads, hidden=None, num_in=None, causal=False, eps=1e-5, fused=True, dropout=0.0, generator=None,
                 kv_heads=None, rope=None, mlp="gelu"):
        super().__init__("TransformerBlock")
        if mlp not in MLP_FORMS:
            raise ValueError("TransformerBlock: mlp must be one of %s, got %r" % (sorted(MLP_FORMS), mlp))
        self.mlp = mlp
        self.kv_heads = kv_heads
        self.rope = rope
        self.drop = Dropout(dropout, generator=generator, fused=fused)
        self.num_heads, self.hidden, self.causal, self.eps, self.fused = int(num_heads), hidden, bool(causal), float(eps), fused
        if self.num_heads < 1:
            raise ValueError("TransformerBlock: num_heads must be >= 1, got %r" % (num_heads,))
        if hidden is not None and int(hidden) < 1:
            raise ValueError("TransformerBlock: hidden must be >= 1, got %r" % (hidden,))
        self.parts = None
        self.params = dict.fromkeys(BLOCK_PARAM_ORDER)
        self.inputs = None
        self.is_init = False
        if num_in is not None:
            self._init_parameters(int(num_in))

    def _init_parameters(self, width):
        gate = MLP_FORMS[self.mlp] is not None
        if self.hidden is not None:
            hidden = int(self.hidden)
        elif gate:
            from ..gated import gated_hidden
            hidden = gated_hidden(width)
        else:
            hidden = 4 * width
        # created in BLOCK_PARAM_ORDER: each part draws from the host RNG as it is built
        parts = {}
        parts["ln1"] = LayerNorm(width, eps=self.eps, fused=self.fused)
        parts["attn"] = MultiHeadAttention(self.num_heads, num_in=width, causal=self.causal, fused=self.fused,
                                           kv_heads=self.kv_heads, rope=self.rope)
        parts["ln2"] = LayerNorm(width, eps=self.eps, fused=self.fused)
        parts["fc1"] = Dense(2 * hidden if gate else hidden, num_in=width, fused=self.fused)
        parts["fc2"] = Dense(width, num_in=hidden, fused=self.fused)
        self.parts, self.hidden, self.width = parts, hidden, width
        for key in BLOCK_PARAM_ORDER:
            part, name = key.split(".")
            self.params[key] = parts[part].params[name]
        self.is_init = True

    def forward(self, inputs, cache=None, lens=None):
        """cache, lens: handed to the attention part (MultiHeadAttention.forward); None: today's path.  lens together with a
        cache raises before any launch."""
        if len(inputs.shape) != 3:
            raise ValueError("TransformerBlock: the input must be [B, T, E], got shape %s" % (tuple(inputs.shape),))
        if lens is not None and cache is not None:
            raise ValueError("TransformerBlock: lens= (training over a padded batch) and cache= (generation) do not go together")
        b, t, e = (int(s) for s in inputs.shape)
        if not self.is_init:
            self._init_parameters(e)
        if e != self.width:
            raise ValueError("TransformerBlock: the input width %d differs from the block's %d" % (e, self.width))
        self.inputs = inputs
        parts = self.parts
        for key in BLOCK_PARAM_ORDER:                # the flat dict is the truth (Net.set_parameters replaces its tensors)
            part, name = key.split(".")
            parts[part].params[name] = self.params[key]
        if self.rope is not None:
            parts["attn"]._check_rope(t, cache)          # positions beyond the rotary tables raise before ANY launch
        normed = parts["ln1"].forward(inputs)
        h = self.drop.forward(parts["attn"].forward(normed, cache=cache, lens=lens), residual=inputs)   # (inactive: inputs + attn)
        z = parts["fc1"].forward(ops.reshape(parts["ln2"].forward(h), (b * t, e)))
        act = MLP_FORMS[self.mlp]
        if act is None:
            z = ops.gelu_(z, approximate="tanh", route=None if self.fused else "composed")
        else:
            z = ops.gated_(z, act=act, packed=True, route=None if self.fused else "composed")
        return self.drop.forward(ops.reshape(parts["fc2"].forward(z), (b, t, e)), residual=h)

    def set_phase(self, phase):
        super().set_phase(phase)
        self.drop.set_phase(phase)
        for part in (self.parts or {}).values():
            part.set_phase(phase)


class Embedding(Layer):
    """Token embedding over integer ids [B, T] -> [B, T, width]: the rows "tok"[ids] of a [vocab, width] table, plus the
    learned positions "pos"[t] of a [max_len, width] table when `max_len` is given (T > max_len raises).  Parameters: "tok"
    then "pos" (EMBED_PARAM_ORDER; "pos" exists only with max_len), created — and drawn from the host RNG — in THAT order, both
    with `w_init`.  The gradient of "tok" ACCUMULATES over repeated ids; the row `padding_idx` receives none.  The ids never
    get a gradient.  `fused=False` runs the composed route (a row gather; a one-hot product backward that reads the ids on the
    host).  dropout > 0: dropout on the output in the TRAIN phase (ops.dropout_, from `generator`; None: the default generator
    of rng.py); 0, the default, adds no launch."""

    def __init__(self, vocab, width, max_len=None, padding_idx=None, w_init=NormalInit(0.0, 0.02), fused=True, dropout=0.0,
                 generator=None):
        super().__init__("Embedding")
        self.drop = Dropout(dropout, generator=generator, fused=fused)
        self.vocab, self.width, self.max_len, self.fused = int(vocab), int(width), max_len, fused
        if self.vocab < 1 or self.width < 1 or (max_len is not None and int(max_len) < 1):
            raise ValueError("Embedding: vocab, width and max_len must be >= 1, got %r, %r, %r" % (vocab, width, max_len))
        if padding_idx is not None and not 0 <= int(padding_idx) < self.vocab:
            raise ValueError("Embedding: padding_idx %r outside [0, %d)" % (padding_idx, self.vocab))
        self.padding_idx = None if padding_idx is None else int(padding_idx)
        self.names = EMBED_PARAM_ORDER if max_len is not None else EMBED_PARAM_ORDER[:1]
        self.shapes = {"tok": [self.vocab, self.width]}
        if max_len is not None:
            self.shapes["pos"] = [int(max_len), self.width]
        self.params = {}
        for name in self.names:                      # created in EMBED_PARAM_ORDER: each draws from the host RNG
            tensor = w_init(shape=self.shapes[name])
            tensor.zero_grad()
            self.params[name] = tensor
        self.inputs = None
        self.is_init = True

    def forward(self, inputs, offset=0, positions=None):
        """offset: the position of the first id (a decoding step embeds token `offset` alone): positions offset .. offset +
        T - 1 are used, as the row slice of "pos".
        positions: a ragged.Lengths [B] (inference only; it excludes `offset`) — ids [B, 1], sequence b's id sits at position
        positions[b], read on the device (ops.embedding_at_); max_len is checked against the host mirror before any launch."""
        if len(inputs.shape) != 2:
            raise ValueError("Embedding: the input must be integer ids [B, T], got shape %s" % (tuple(inputs.shape),))
        if positions is not None:
            if int(offset) != 0:
                raise ValueError("Embedding: `positions` excludes `offset`")
            if int(inputs.shape[1]) != 1 or tuple(positions.shape) != (int(inputs.shape[0]),):
                raise ValueError("Embedding: `positions` takes ids [B, 1] and one position per sequence, got ids %s and "
                                 "positions %s" % (tuple(inputs.shape), tuple(positions.shape)))
            if self.max_len is not None and positions.host.size and not (0 <= int(positions.host.min())
                                                                         and int(positions.host.max()) < int(self.max_len)):
                raise ValueError("Embedding: positions %d .. %d lie outside max_len %d"
                                 % (int(positions.host.min()), int(positions.host.max()), int(self.max_len)))
            self.inputs = inputs
            return ops.embedding_at_(self.params["tok"], inputs, positions, self.params.get("pos"),
                                     route=None if self.fused else "composed")
        offset = int(offset)
        if offset < 0:
            raise ValueError("Embedding: offset must be >= 0, got %d" % offset)
        if self.max_len is not None and offset + int(inputs.shape[1]) > int(self.max_len):
            raise ValueError("Embedding: sequences of %d ids%s exceed max_len %d"
                             % (int(inputs.shape[1]), " at offset %d" % offset if offset else "", int(self.max_len)))
        self.inputs = inputs
        pos = self.params.get("pos")
        if pos is not None and offset:
            pos = ops.getitem_(pos, slice(offset, offset + int(inputs.shape[1])))
        out = ops.embedding_(self.params["tok"], inputs, pos, padding_idx=self.padding_idx,
                             route=None if self.fused else "composed")
        return self.drop.forward(out) if self.drop.active() else out

    def set_phase(self, phase):
        super().set_phase(phase)
        self.drop.set_phase(phase)
