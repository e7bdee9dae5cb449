"""ctypes binding of include/tnn_hip.h (libtnn_hip.so, gfx950).

This is the only place that talks to the native library.  It fails loudly: a missing shared object,
a missing symbol or a machine without a GPU raise at first use — there is no CPU fallback in the
product.  (tests/ may inject the CPU twin from oracle/ explicitly through install_test_twin(); nothing
in this package ever looks for it.)
"""

import ctypes
import os
from ctypes import c_char_p, c_double, c_int, c_int64, c_size_t, c_void_p, POINTER

import sys

# the package directory — taken from the package, not from __file__: this module may run from its compiled copy under
# _compiled/ (_host_build.py)
_HERE = os.path.dirname(os.path.abspath(sys.modules[__name__.rpartition(".")[0]].__file__))
# TNN_LIB_PATH: another build of the same library (same-box A/B timing of kernel variants, tools/probes/)
LIB_PATH = os.environ.get("TNN_LIB_PATH") or os.path.join(_HERE, "lib", "libtnn_hip.so")

# dtype / op codes (must mirror include/tnn_hip.h)
F32, F64, I64, U8, BF16 = 0, 1, 2, 3, 4
OPT_MOMENTUM, OPT_RMSPROP, OPT_ADAGRAD, OPT_ADADELTA = 0, 1, 2, 3
ADD, SUB, MUL, DIV, POW, MAX, MIN = range(7)
GT, GE, LT, LE, EQ, NE = range(6)
NEG, EXP, LOG, SQRT, SQUARE, ABS, RECIP, SIGMOID, TANH, COPY = range(10)
RSUM, RMAX, RMIN = range(3)
ACT_NONE, ACT_RELU = 0, 1

from ._signatures import _SIGNATURES, _i64p, _p        # noqa: E402  (name -> argtypes; every entry point returns int except tnn_last_error)

EXPORTED_SYMBOLS = sorted(list(_SIGNATURES) + ["tnn_last_error"])

from ._index_signatures import _INDEX_SIGNATURES, IndexDesc   # noqa: E402,F401  (include/tnn_index.h: libtnn_hip.so only)

INDEX_SYMBOLS = sorted(_INDEX_SIGNATURES)

from ._bmm_signatures import _BMM_SIGNATURES                  # noqa: E402  (include/tnn_bmm.h: libtnn_hip.so only)

BMM_SYMBOLS = sorted(_BMM_SIGNATURES)

from ._conv_signatures import _CONV_SIGNATURES                # noqa: E402  (include/tnn_conv.h: libtnn_hip.so only)

CONV_SYMBOLS = sorted(_CONV_SIGNATURES)

from ._attn_signatures import _ATTN_SIGNATURES                # noqa: E402  (include/tnn_attn.h: libtnn_hip.so only)

ATTN_SYMBOLS = sorted(_ATTN_SIGNATURES)

from ._norm_signatures import _NORM_SIGNATURES                # noqa: E402  (include/tnn_norm.h: libtnn_hip.so only)

NORM_SYMBOLS = sorted(_NORM_SIGNATURES)

from ._token_signatures import _TOKEN_SIGNATURES              # noqa: E402  (include/tnn_token.h: libtnn_hip.so only)

TOKEN_SYMBOLS = sorted(_TOKEN_SIGNATURES)

from ._decode_signatures import _DECODE_SIGNATURES            # noqa: E402  (include/tnn_decode.h: libtnn_hip.so only)

DECODE_SYMBOLS = sorted(_DECODE_SIGNATURES)

from ._dropout_signatures import _DROPOUT_SIGNATURES          # noqa: E402  (include/tnn_dropout.h: libtnn_hip.so only)

DROPOUT_SYMBOLS = sorted(_DROPOUT_SIGNATURES)

from ._ostep_signatures import _OSTEP_SIGNATURES              # noqa: E402  (include/tnn_ostep.h: libtnn_hip.so only)

OSTEP_SYMBOLS = sorted(_OSTEP_SIGNATURES)

from ._ragged_signatures import _RAGGED_SIGNATURES            # noqa: E402  (include/tnn_ragged.h: libtnn_hip.so only)

RAGGED_SYMBOLS = sorted(_RAGGED_SIGNATURES)

from ._gqa_signatures import _GQA_SIGNATURES                  # noqa: E402  (include/tnn_gqa.h: libtnn_hip.so only)

GQA_SYMBOLS = sorted(_GQA_SIGNATURES)

from ._rope_signatures import _ROPE_SIGNATURES                # noqa: E402  (include/tnn_rope.h: libtnn_hip.so only)

ROPE_SYMBOLS = sorted(_ROPE_SIGNATURES)

from ._gated_signatures import _GATED_SIGNATURES              # noqa: E402  (include/tnn_gated.h: libtnn_hip.so only)

GATED_SYMBOLS = sorted(_GATED_SIGNATURES)

from ._extend_signatures import _EXTEND_SIGNATURES            # noqa: E402  (include/tnn_extend.h: libtnn_hip.so only)

EXTEND_SYMBOLS = sorted(_EXTEND_SIGNATURES)

from ._varlen_signatures import _VARLEN_SIGNATURES            # noqa: E402  (include/tnn_varlen.h: libtnn_hip.so only)

VARLEN_SYMBOLS = sorted(_VARLEN_SIGNATURES)


class TnnError(RuntimeError):
    """A native call returned non-zero; the message is tnn_last_error()."""


def _fast_wrappers(path):
    """{entry point: callable} from the compiled call-wrapper module (_host_build.py builds it; TNN_HOST_COMPILED=0 or a
    signature table that has changed since it was built -> {}: every call goes through ctypes)."""
    if os.environ.get("TNN_HOST_COMPILED", "1") == "0":
        return {}
    try:
        import importlib.util
        import sysconfig
        so = os.path.join(_HERE, "_compiled", "_tnn_fastcall" + (sysconfig.get_config_var("EXT_SUFFIX") or ".so"))
        if not os.path.exists(so):
            return {}
        from . import _fastcall_gen
        spec = importlib.util.spec_from_file_location("_tnn_fastcall", so)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        if mod.SIGNATURE_HASH != _fastcall_gen.signature_hash(_SIGNATURES):
            return {}
        return mod.bind(path, TnnError)
    except (ImportError, OSError):
        return {}


class _Lib(object):
    """Holds the CDLL and one bound callable per entry point that raises on failure."""

    def __init__(self, path):
        if not os.path.exists(path):
            raise ImportError(
                "native library %s not found — build it first: "
                "`python -c 'import __graft_entry__ as g; g.build()'` or "
                "`make -C tinynn-autograd_amd/csrc -j8`" % path)
        self.path = path
        self.cdll = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
        self.cdll.tnn_last_error.restype = c_char_p
        self.cdll.tnn_last_error.argtypes = []
        fast = _fast_wrappers(path)
        for name, argtypes in _SIGNATURES.items():
            fn = getattr(self.cdll, name)     # AttributeError here = header/library mismatch
            fn.argtypes = argtypes
            fn.restype = c_int
            # the compiled call wrapper of this entry point when there is one (same function, same error behaviour,
            # arguments converted in C: _fastcall_gen.py), else the ctypes binding
            setattr(self, name[4:], fast.get(name) or self._wrap(name, fn))
        self.fast_calls = len(fast)
        self.kind = self.cdll.tnn_backend_kind()
        # the advanced-indexing entry points (include/tnn_index.h): required of the product library; the CPU test twin has
        # none, and the paths that need them raise there
        # and the strided-batched GEMM (include/tnn_bmm.h), likewise: under the twin device_array.matmul loops over tnn_gemm
        # and convolution / pooling (include/tnn_conv.h): under the twin device_array composes them from slices and products
        # and fused attention (include/tnn_attn.h): under the twin device_array composes it from products, exp and sums
        # and layer norm, RMS norm and GELU (include/tnn_norm.h): under the twin device_array composes them from sums,
        # products, sqrt and tanh (the exact GELU has no composed form and raises there)
        # and the embedding and the per-row cross-entropy (include/tnn_token.h): under the twin device_array composes them
        # from take, a one-hot product, max / exp / sum / log and the advanced-index gather
        # and decode attention and token sampling (include/tnn_decode.h): under the twin device_array appends by a slice
        # assignment and runs the composed attention over the live prefix; sampling reads the logits back
        # and the random generator and dropout (include/tnn_dropout.h): under the twin rng.Generator keeps its state in two
        # host integers and device_array draws the mask with the planner's numpy generator (dropout.py)
        # and the device-resident optimizer step (include/tnn_ostep.h): under the twin core/optimizer.AdamW and
        # Model.clip_grad_norm evaluate the same maths on DeviceArray arithmetic and read the norm back
        # and the ragged decoding step (include/tnn_ragged.h): under the twin device_array loops over the sequences with the
        # host mirror of the lengths and advances the step's state in numpy (ragged.py)
        # and grouped-query attention (include/tnn_gqa.h): under the twin device_array repeats k and v over the group, runs
        # the composed attention / decode and sums dk and dv over the group (gqa.py)
        # and the rotary position embedding (include/tnn_rope.h): under the twin device_array rotates with slice reads,
        # products and slice assignments (rope.py)
        # and the gated activations (include/tnn_gated.h): under the twin device_array composes them from sigmoid or tanh,
        # products and sums on slices (gated.py; the exact-GELU gate has no composed form and raises there)
        # and cache-extending attention (include/tnn_extend.h): under the twin device_array slice-assigns the new rows and
        # runs the composed attention over the live prefix with the offset mask (extend.py)
        # and training attention with per-sequence lengths (include/tnn_varlen.h): under the twin device_array runs the
        # composed attention with a key mask and a row mask built from the lengths on the host (varlen.py)
        for table, header, what in ((_INDEX_SIGNATURES, "tnn_index.h", "advanced indexing"),
                                    (_BMM_SIGNATURES, "tnn_bmm.h", "batched matmul"),
                                    (_CONV_SIGNATURES, "tnn_conv.h", "convolution"),
                                    (_ATTN_SIGNATURES, "tnn_attn.h", "attention"),
                                    (_NORM_SIGNATURES, "tnn_norm.h", "normalisation"),
                                    (_TOKEN_SIGNATURES, "tnn_token.h", "embedding / cross-entropy"),
                                    (_DECODE_SIGNATURES, "tnn_decode.h", "decode attention / sampling"),
                                    (_DROPOUT_SIGNATURES, "tnn_dropout.h", "random generator / dropout"),
                                    (_OSTEP_SIGNATURES, "tnn_ostep.h", "optimizer step"),
                                    (_RAGGED_SIGNATURES, "tnn_ragged.h", "ragged decoding step"),
                                    (_GQA_SIGNATURES, "tnn_gqa.h", "grouped-query attention"),
                                    (_ROPE_SIGNATURES, "tnn_rope.h", "rotary position embedding"),
                                    (_GATED_SIGNATURES, "tnn_gated.h", "gated activation"),
                                    (_EXTEND_SIGNATURES, "tnn_extend.h", "cache-extending attention"),
                                    (_VARLEN_SIGNATURES, "tnn_varlen.h", "attention with per-sequence lengths")):
            for name, argtypes in table.items():
                fn = getattr(self.cdll, name, None)
                if fn is None:
                    if self.kind == 1:
                        raise ImportError("%s lacks %s (include/%s) — rebuild it" % (path, name, header))
                    setattr(self, name[4:], self._absent(name, what))
                    continue
                fn.argtypes = argtypes
                fn.restype = c_int
                setattr(self, name[4:], self._wrap(name, fn))
        self.has_bmm = hasattr(self.cdll, "tnn_gemm_batched")
        self.has_conv = hasattr(self.cdll, "tnn_conv2d_fwd")
        self.has_attn = hasattr(self.cdll, "tnn_attn_fwd")
        self.has_norm = hasattr(self.cdll, "tnn_norm_fwd")
        self.has_token = hasattr(self.cdll, "tnn_embed_fwd")
        self.has_decode = hasattr(self.cdll, "tnn_decode_attn")
        self.has_dropout = hasattr(self.cdll, "tnn_dropout_fwd")
        self.has_ostep = hasattr(self.cdll, "tnn_ostep_adamw")
        self.has_ragged = hasattr(self.cdll, "tnn_ragged_decode_attn")
        self.has_gqa = hasattr(self.cdll, "tnn_gqa_decode_attn")
        self.has_rope = hasattr(self.cdll, "tnn_rope_apply")
        self.has_gated = hasattr(self.cdll, "tnn_gated_fwd")
        self.has_extend = hasattr(self.cdll, "tnn_extend_attn")
        self.has_varlen = hasattr(self.cdll, "tnn_varlen_fwd")

    @staticmethod
    def _absent(name, what):
        def call(*args):
            raise TnnError("%s (%s) needs libtnn_hip.so; the CPU test twin does not implement it" % (name, what))
        call.__name__ = name
        return call

    def _wrap(self, name, fn):
        last_error = self.cdll.tnn_last_error

        def call(*args):
            rc = fn(*args)
            if rc != 0:
                msg = last_error()
                raise TnnError("%s failed (rc=%d): %s" % (
                    name, rc, msg.decode("utf-8", "replace") if msg else "?"))
        call.__name__ = name
        return call


_lib = None
_is_test_twin = False


class _TorchAfterLoadGuard:
    """torch bundles its own libamdhip64 / librccl and loads them by absolute path.  Imported BEFORE libtnn_hip.so they are
    the one HIP runtime both bind to; imported AFTER it, the process holds two runtimes (torch.cuda sees no device memory of
    ours, RCCL communicators cannot be shared, abort at interpreter exit).  get() imports torch itself when the environment
    says a communicator will be needed; for everybody else this finder turns the late import into a loud warning."""

    def find_spec(self, name, path=None, target=None):
        if name == "torch" and _lib is not None and not _is_test_twin:
            import warnings
            warnings.warn("torch is being imported AFTER tinynn_autograd_amd initialised its HIP runtime: the process now "
                          "holds two HIP runtimes (torch.cuda and RCCL will not see this package's memory). "
                          "`import torch` before the first tinynn_autograd_amd device call.", RuntimeWarning, stacklevel=2)
        return None


_guard_installed = False


def get():
    """The initialised library.  Raises if libtnn_hip.so is missing or no MI355X is visible."""
    global _lib, _guard_installed
    if _lib is None:
        import sys
        if "torch" not in sys.modules:
            if int(os.environ.get("WORLD_SIZE", "1")) > 1 or os.environ.get("TNN_FORCE_COMM") == "1":
                import torch  # noqa: F401  (a communicator will be built: torch's HIP runtime must be the process's one)
            elif not _guard_installed:
                sys.meta_path.insert(0, _TorchAfterLoadGuard())
                _guard_installed = True
        lib = _Lib(LIB_PATH)
        # one process per GPU: torchrun's LOCAL_RANK picks the device; TNN_DEVICE overrides (e.g. several ranks
        # sharing one GPU in the peer-to-peer transport test)
        device = int(os.environ.get("TNN_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        lib.init(device)              # raises TnnError when no HIP device is visible
        _lib = lib
    return _lib


def is_loaded():
    return _lib is not None


def backend_name():
    if _lib is None:
        return "unloaded"
    return "hip-gfx950" if _lib.kind == 1 else "cpu-twin(test only)"


def install_test_twin(path):
    """TESTS ONLY: route the ABI to the CPU twin built from oracle/cpu_twin (no GPU in the container).

    Never called by the package itself; bench.py and __graft_entry__.smoke() assert that
    backend_name() == "hip-gfx950".
    """
    global _lib, _is_test_twin
    import sys
    da = sys.modules.get(__name__.rsplit(".", 1)[0] + ".device_array")
    if da is not None:
        da.trim_cache()               # buffers of the library being replaced
    lib = _Lib(path)
    if lib.kind != 2:
        raise TnnError("install_test_twin: %s is not the CPU test twin" % path)
    lib.init(0)
    _lib = lib
    _is_test_twin = True
    return lib


def device_props():
    lib = get()
    cu, clk, hbm = c_int(0), c_int(0), c_int64(0)
    name = ctypes.create_string_buffer(256)
    lib.device_props(ctypes.byref(cu), ctypes.byref(clk), ctypes.byref(hbm), name, 256)
    return {"name": name.value.decode(), "cus": cu.value, "clock_khz": clk.value,
            "hbm_bytes": hbm.value}


def pool_stats():
    lib = get()
    a, b, c = c_int64(0), c_int64(0), c_int64(0)
    lib.pool_stats(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
    import sys
    da = sys.modules.get(__name__.rsplit(".", 1)[0] + ".device_array")
    return {"live_bytes": a.value, "cached_bytes": b.value, "device_allocs": c.value,
            "host_cached_bytes": da._cache_bytes if da is not None else 0}     # part of live_bytes: device_array's free lists


def synchronize():
    get().stream_sync()


class Event(object):
    """HIP event on the library stream (what bench.py times kernels with)."""

    def __init__(self):
        self._h = c_void_p()
        get().event_create(ctypes.byref(self._h))

    def record(self):
        get().event_record(self._h)
        return self

    def elapsed_ms(self, later):
        ms = ctypes.c_float(0)
        get().event_elapsed_ms(self._h, later._h, ctypes.byref(ms))
        return ms.value

    def __del__(self):
        try:
            if _lib is not None and self._h:
                _lib.event_destroy(self._h)
        except Exception:
            pass


capturing = False     # a hipGraph capture is open (Graph.__enter__ .. __exit__)


class Graph(object):
    """hipGraph captured from everything enqueued on the library stream inside the `with` block."""

    def __init__(self):
        self._h = None

    def __enter__(self):
        global capturing
        get().graph_capture_begin()
        capturing = True                 # device_array's buffer cache steps aside: the pool tags capture-time buffers
        return self

    def __exit__(self, exc_type, exc, tb):
        global capturing
        capturing = False
        h = c_void_p()
        try:
            get().graph_capture_end(ctypes.byref(h))
            self._h = h
        except TnnError:
            if exc_type is None:
                raise
        return False

    def launch(self):
        get().graph_launch(self._h)

    def __del__(self):
        try:
            if _lib is not None and self._h:
                _lib.graph_destroy(self._h)
        except Exception:
            pass
