"""DeviceArray: the HBM-resident stand-in for the numpy ndarray behind reference Tensors.

The reference keeps a numpy array in `Tensor._values` / `Tensor.grad` (core/tensor.py:20,171) and its
callers use ndarray idioms on them (`.tolist()`, `.shape`, `np.ravel`, `np.concatenate`, slicing,
arithmetic — core/optimizer.py:14-15,27,47,70-77, examples/mnist/run.py:89).  DeviceArray implements
that surface on top of the C-ABI (include/tnn_hip.h): operators, `__array_ufunc__`,
`__array_function__`, slicing/reshape views and an explicit, synchronising `__array__` (D2H).

Design points
  * always dense row-major; slices of the leading axis, `reshape`, `ravel` are zero-copy views that keep
    their base alive; a 2-D `.T` is a lazy flag consumed by matmul (so `grad @ w.T` and `x.T @ grad`
    become NT / TN GEMMs without materialising a transpose, core/ops.py:157,160).
  * Python / numpy scalars never become device buffers: they ride along as "host scalars" and are
    passed as kernel arguments (tnn_ewise_scalar).
  * no CPU fallback: an operation that has no device implementation raises TypeError.
  * dtypes: float32 (default), float64 (exact mode / explicit), int64 (indices), bool (masks).
    Integer and bool operands of arithmetic are cast to the default float on device.
"""

import collections
import ctypes
import math
import numbers

import weakref

import numpy as np

from . import _lib
from . import attention as _at
from . import batching as _bt
from . import conv as _cv
from . import decoding as _dc
from . import dropout as _dp
from . import extend as _ex
from . import gated as _gt
from . import gqa as _gq
from . import indexing as _ix
from . import norm as _nm
from . import ragged as _rg
from . import rope as _rp
from . import tokens as _tk
from . import varlen as _vl
from ._lib import F32, F64, I64, U8

_CODE = {np.dtype(np.float32): F32, np.dtype(np.float64): F64, np.dtype(np.int64): I64,
         np.dtype(np.bool_): U8,
         np.dtype(np.uint16): _lib.BF16}     # raw bf16 bit patterns: storage only (tinynn_autograd_amd.bf16)
_default_float = np.dtype(np.float32)
READONLY_COPY = "readonly-copy"      # DeviceArray._tag of a snapshot that must not be mistaken for a view (fused.MLPTrainer.param_view)
MAX_NDIM = 6


def set_default_float(dtype):
    """float32 (hot path, default) or float64 (bit-for-bit mode of the reference's known-answer tests)."""
    global _default_float
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError("default float must be float32 or float64")
    _default_float = dtype


def get_default_float():
    return _default_float


def _i64arr(values):
    return (ctypes.c_int64 * len(values))(*values)


_prod = math.prod


def _dense_strides(shape):
    st, acc = [], 1
    for s in reversed(shape):
        st.append(acc)
        acc *= int(s)
    return tuple(reversed(st))


def _is_scalar_like(x):
    tx = type(x)
    if tx is float or tx is int:                     # (no ABC instance check for the exact Python types)
        return True
    return isinstance(x, (numbers.Number, np.generic)) or (isinstance(x, np.ndarray) and x.ndim == 0)


# ---- host-side buffer cache in front of tnn_malloc / tnn_free.  The native pool already recycles HBM, but every
# tnn_malloc / tnn_free is a ctypes call (~1.5 us each, 18 of them per eager MNIST-size training step, more than its
# nine kernel launches cost the host).  Freed buffers of an eager step are kept here by size class and handed out again
# without leaving Python; one stream orders all work, so a recycled buffer is safe to reuse at once (the native pool's own
# argument).  Buffers allocated while a hipGraph is being captured belong to that graph in the native pool and never enter
# this cache (own == 2), and nothing is taken from it during a capture.
_cache = {}                       # size class (bytes) -> [ptr, ...]
_cache_bytes = 0
_CACHE_LIMIT = 256 << 20          # beyond this the buffers go back to the native pool
_CACHE_MAX_BLOCK = 32 << 20       # large buffers are rare and expensive to keep twice


def _size_class(nbytes):
    return (nbytes + 511) & ~511 if nbytes > 0 else 512


def trim_cache():
    """Return every cached buffer to the native pool (tests that audit tnn_pool_stats, shutdown)."""
    global _cache_bytes
    lib = _lib._lib
    _ATTN_MASKS.clear()               # the composed attention route's causal masks: device buffers like any other
    for cls, ptrs in _cache.items():
        for ptr in ptrs:
            if lib is not None:
                lib.free(ptr)
    _cache.clear()
    _cache_bytes = 0


class DeviceArray(object):
    __slots__ = ("_ptr", "shape", "dtype", "_base", "_hv", "_t", "_tag", "_own", "_aux", "_sc", "__weakref__")
    __array_priority__ = 1000.0

    # ------------------------------------------------------------------ construction
    def __init__(self):
        raise TypeError("use asarray()/empty()/zeros() to create a DeviceArray")

    @classmethod
    def _raw(cls, ptr, shape, dtype, base=None, hv=None, t=False):
        self = object.__new__(cls)
        self._ptr = ptr
        # (shapes reach this point as tuples of Python ints from every internal caller: checked, not rebuilt)
        if type(shape) is tuple:
            n = len(shape)
            if n == 2:
                ok = type(shape[0]) is int and type(shape[1]) is int
            elif n == 1:
                ok = type(shape[0]) is int
            else:
                ok = n == 0 or all(type(v) is int for v in shape)
        else:
            ok = False
        if not ok:
            shape = tuple(map(int, shape))
        self.shape = shape
        self.dtype = dtype if type(dtype) is np.dtype else np.dtype(dtype)
        self._base = base
        self._hv = hv
        self._t = t
        self._own = 0                # 0: the native pool's (or not owned), 1: recyclable through _cache, 2: graph-owned
        self._sc = 0                 # size class of an owned buffer (bytes), set by _new
        self._aux = None             # by-product of the producing launch riding along (core/ops.py: the partial logits)
        self._tag = None             # free-form marker: RELU_SIGN on a fused Dense+ReLU output; the producer's output array
                                     # on a gradient whose ReLU mask has already been applied (core/ops.py dense_)
        return self

    @classmethod
    def _new(cls, shape, dtype):
        global _cache_bytes
        dtype = dtype if type(dtype) is np.dtype else np.dtype(dtype)
        nbytes = _prod(shape) * dtype.itemsize
        sc = _size_class(nbytes)
        if not _lib.capturing:
            ptrs = _cache.get(sc)
            if ptrs:
                self = cls._raw(ptrs.pop(), shape, dtype)
                _cache_bytes -= sc
                self._own = 1
                self._sc = sc
                return self
        p = ctypes.c_void_p()
        _lib.get().malloc(sc, ctypes.byref(p))
        self = cls._raw(p.value, shape, dtype)
        self._own = 2 if _lib.capturing else 1
        self._sc = sc
        return self

    @classmethod
    def _scalar(cls, value):
        """Host scalar (weakly typed, like a Python number under numpy promotion)."""
        tv = type(value)
        if tv is not float and tv is not int:        # (exact Python floats / ints: nothing to normalise, no ABC instance checks)
            if isinstance(value, np.ndarray):
                value = value[()]
            if isinstance(value, (bool, np.bool_)):
                value = float(value)
            elif isinstance(value, (numbers.Integral, np.integer)):
                value = int(value)
            else:
                value = float(value)
        return cls._raw(None, (), _default_float, hv=value)

    def __del__(self):
        global _cache_bytes
        try:
            if self._base is None and self._ptr is not None and _lib._lib is not None:
                if self._own == 1 and not _lib.capturing:
                    sc = self._sc or _size_class(_prod(self.shape) * self.dtype.itemsize)
                    if sc <= _CACHE_MAX_BLOCK and _cache_bytes + sc <= _CACHE_LIMIT:
                        _cache.setdefault(sc, []).append(self._ptr)
                        _cache_bytes += sc
                        return
                _lib._lib.free(self._ptr)
        except Exception:
            pass

    # ------------------------------------------------------------------ basic properties
    @property
    def ndim(self):
        return len(self.shape)

    @property
    def size(self):
        return _prod(self.shape)

    @property
    def nbytes(self):
        return self.size * self.dtype.itemsize

    @property
    def itemsize(self):
        return self.dtype.itemsize

    @property
    def is_host_scalar(self):
        return self._hv is not None

    def __len__(self):
        if not self.shape:
            raise TypeError("len() of unsized object")
        return self.shape[0]

    def __repr__(self):
        if self._hv is not None:
            return "DeviceArray(host scalar %r)" % (self._hv,)
        return "DeviceArray(shape=%s, dtype=%s)" % (self.shape, self.dtype.name)

    __hash__ = object.__hash__

    def _code(self):
        return _CODE[self.dtype]

    def _dev(self):
        """Pointer to a dense row-major device buffer holding this array's logical content."""
        if self._hv is not None:
            return self._materialise_scalar()._ptr
        if self._t:
            return self._contig()._ptr
        return self._ptr

    def _materialise_scalar(self):
        out = DeviceArray._new((), self.dtype)
        _lib.get().fill(out._ptr, float(self._hv), 1, out._code())    # a kernel, not an H2D copy: capturable, no sync
        return out

    def _contig(self):
        """Same logical array without the lazy-transpose flag (materialises the transpose)."""
        if self._hv is not None:
            return self._materialise_scalar()
        if not self._t:
            return self
        rows, cols = self.shape           # logical; stored as [cols, rows]
        out = DeviceArray._new(self.shape, self.dtype)
        _lib.get().strided_copy(self._ptr, _i64arr((1, rows)), out._ptr, 2, _i64arr((rows, cols)),
                                self._code())
        return out

    # ------------------------------------------------------------------ host transfer
    def __array__(self, dtype=None, copy=None):
        if self._hv is not None:
            out = np.asarray(self._hv, dtype=self.dtype)
        else:
            src = self._contig()
            host_dtype = np.bool_ if self.dtype == np.bool_ else self.dtype
            out = np.empty(self.shape, dtype=host_dtype)
            if out.size:
                _lib.get().memcpy_d2h(out.ctypes.data, src._ptr, out.nbytes)
        if dtype is not None and np.dtype(dtype) != out.dtype:
            out = out.astype(dtype)
        return out

    def numpy(self):
        return self.__array__()

    def tolist(self):
        return self.__array__().tolist()

    def item(self):
        if self.size != 1:
            raise ValueError("can only convert an array of size 1 to a Python scalar")
        if self._hv is not None:
            return self._hv
        return self.__array__().reshape(()).item()

    def __float__(self):
        return float(self.item())

    def __int__(self):
        return int(self.item())

    def __bool__(self):
        if self.size != 1:
            raise ValueError("The truth value of an array with more than one element is ambiguous.")
        return bool(self.item())

    def __iter__(self):
        for i in range(len(self)):
            yield self[i]

    # ------------------------------------------------------------------ dtype handling
    def astype(self, dtype):
        if dtype is self.dtype:                      # (np.dtype objects are singletons per type: the common no-op case)
            return self
        dtype = np.dtype(dtype)
        if dtype == self.dtype:
            return self
        if dtype not in _CODE:
            raise TypeError("unsupported device dtype %s" % dtype)
        if self._hv is not None:
            return DeviceArray._raw(None, (), dtype, hv=self._hv)
        src = self._contig()
        out = DeviceArray._new(self.shape, dtype)
        _lib.get().cast(src._ptr, src._code(), out._ptr, _CODE[dtype], self.size)
        return out

    def _as_float(self, dtype=None):
        if dtype is None:
            dtype = self.dtype if self.dtype.kind == "f" else _default_float
        return self.astype(dtype)

    def copy(self):
        src = self._contig()
        if src._hv is not None:
            return DeviceArray._raw(None, (), self.dtype, hv=self._hv)
        out = DeviceArray._new(self.shape, self.dtype)
        _lib.get().memcpy_d2d(out._ptr, src._ptr, self.nbytes)
        return out

    def fill(self, value):
        _lib.get().fill(self._ptr, float(value), self.size, self._code())

    # ------------------------------------------------------------------ shape manipulation (views)
    def reshape(self, *newshape):
        if len(newshape) == 1 and not isinstance(newshape[0], numbers.Integral):
            newshape = tuple(newshape[0])
        newshape = [int(s) for s in newshape]
        if newshape.count(-1) > 1:
            raise ValueError("can only specify one unknown dimension")
        if -1 in newshape:
            known = _prod([s for s in newshape if s != -1])
            newshape[newshape.index(-1)] = self.size // known if known else 0
        if _prod(newshape) != self.size:
            raise ValueError("cannot reshape array of size %d into shape %s" % (self.size, tuple(newshape)))
        src = self._contig()
        return DeviceArray._raw(src._ptr, newshape, src.dtype, base=src if src._base is None else src._base)

    def ravel(self):
        return self.reshape(self.size)

    def flatten(self):
        return self.ravel().copy()

    @property
    def T(self):
        return self.transpose()

    def transpose(self, *axes):
        if len(axes) == 1 and (axes[0] is None or not isinstance(axes[0], numbers.Integral)):
            axes = axes[0]
        if axes is None or len(axes) == 0:
            axes = tuple(reversed(range(self.ndim)))
        axes = tuple(int(a) % max(self.ndim, 1) for a in axes)
        if sorted(axes) != list(range(self.ndim)):
            raise ValueError("axes don't match array")
        if axes == tuple(range(self.ndim)):
            return self
        if self._hv is not None:
            return self
        if self.ndim == 2:   # lazy flag, flipped
            return DeviceArray._raw(self._ptr, (self.shape[1], self.shape[0]), self.dtype,
                                    base=self if self._base is None else self._base, t=not self._t)
        src = self._contig()
        st = _dense_strides(src.shape)
        new_shape = tuple(src.shape[a] for a in axes)
        new_st = tuple(st[a] for a in axes)
        if len(new_shape) > MAX_NDIM:
            raise TypeError("transpose supports up to %d dimensions on device" % MAX_NDIM)
        out = DeviceArray._new(new_shape, src.dtype)
        _lib.get().strided_copy(src._ptr, _i64arr(new_st), out._ptr, len(new_shape), _i64arr(new_shape),
                                src._code())
        return out

    def swapaxes(self, axis1, axis2):
        """np.swapaxes: a transpose with the two axes exchanged (2-D: the lazy `.T`)."""
        nd = self.ndim
        for ax in (axis1, axis2):
            if not -nd <= int(ax) < nd:
                raise np.exceptions.AxisError("axis %d is out of bounds for array of dimension %d" % (ax, nd))
        perm = list(range(nd))
        i, j = int(axis1) % nd, int(axis2) % nd
        perm[i], perm[j] = perm[j], perm[i]
        return self.transpose(perm)

    def _broadcast_to(self, shape):
        """Materialised broadcast (np.broadcast_to + copy)."""
        shape = tuple(int(s) for s in shape)
        if self.shape == shape and not self._t:
            return self
        src = self._contig()
        st = _broadcast_strides(src.shape, shape)
        out = DeviceArray._new(shape, src.dtype)
        if out.size:
            _lib.get().strided_copy(src._ptr, _i64arr(st), out._ptr, len(shape), _i64arr(shape),
                                    src._code())
        return out

    # ------------------------------------------------------------------ indexing
    def _basic_index(self, key):
        """Resolve ints / slices / None / Ellipsis into (offset, shape, strides) over the dense base."""
        if not isinstance(key, tuple):
            key = (key,)
        if any(k is Ellipsis for k in key):
            i = [j for j, k in enumerate(key) if k is Ellipsis][0]
            n_real = len([k for k in key if k is not None and k is not Ellipsis])
            key = key[:i] + (slice(None),) * (self.ndim - n_real) + key[i + 1:]
        base_st = _dense_strides(self.shape)
        offset, shape, strides, dim = 0, [], [], 0
        for k in key:
            if k is None:
                shape.append(1)
                strides.append(0)
                continue
            if dim >= self.ndim:
                raise IndexError("too many indices for array")
            n = self.shape[dim]
            if isinstance(k, (numbers.Integral, np.integer)):
                k = int(k)
                if k < 0:
                    k += n
                if not 0 <= k < n:
                    raise IndexError("index %d is out of bounds for axis %d with size %d" % (k, dim, n))
                offset += k * base_st[dim]
            elif isinstance(k, slice):
                start, stop, step = k.indices(n)
                length = len(range(start, stop, step))
                offset += start * base_st[dim] if length else 0
                shape.append(length)
                strides.append(step * base_st[dim])
            else:
                raise TypeError("unsupported index %r" % (k,))
            dim += 1
        for d in range(dim, self.ndim):
            shape.append(self.shape[d])
            strides.append(base_st[d])
        return offset, tuple(shape), tuple(strides)

    @staticmethod
    def _is_advanced(key):
        return isinstance(key, (list, np.ndarray, DeviceArray)) and not _is_scalar_like(key)

    @staticmethod
    def _is_rows_key(key):
        """A 1-D integer key on axis 0 (a list, ndarray or device array): the row gather / scatter of tnn_ewise.hip.  Every
        other array key (boolean masks, N-d index arrays, tuples that hold arrays) goes through indexing.py."""
        if isinstance(key, DeviceArray):
            return key.ndim == 1 and key.dtype != np.bool_
        idx = np.asarray(key)
        return idx.ndim == 1 and idx.dtype != np.bool_

    def nonzero(self):
        return _nonzero(self)

    def _index_array(self, key):
        if isinstance(key, DeviceArray):
            if key.dtype == np.bool_:
                raise TypeError("boolean mask indexing is not supported on device")
            return key.astype(np.int64)._contig()
        idx = np.asarray(key)
        if idx.dtype == np.bool_:
            raise TypeError("boolean mask indexing is not supported on device")
        if idx.ndim != 1:
            raise TypeError("only 1-D integer index arrays are supported on device")
        n = self.shape[0]
        if idx.size and (idx.min() < -n or idx.max() >= n):
            raise IndexError("index out of bounds for axis 0 with size %d" % n)
        return asarray(idx.astype(np.int64))

    def __getitem__(self, key):
        if self._hv is not None:
            if key == () or key is Ellipsis:
                return self
            raise IndexError("too many indices for array")
        src = self._contig()
        if DeviceArray._is_advanced(key) and DeviceArray._is_rows_key(key):
            if src.ndim < 1:
                raise IndexError("too many indices for array")
            idx = src._index_array(key)
            row = _prod(src.shape[1:])
            out = DeviceArray._new((idx.size,) + src.shape[1:], src.dtype)
            if out.size:
                _lib.get().gather_rows(src._ptr, idx._ptr, out._ptr, idx.size, row, src.shape[0],
                                       src._code())
            return out
        if not _ix.is_basic(key):
            return _index_gather(src, key)
        offset, shape, strides = src._basic_index(key)
        ptr = src._ptr + offset * src.itemsize
        owner = src if src._base is None else src._base
        if strides == _dense_strides(shape) or _prod(shape) <= 1:
            return DeviceArray._raw(ptr, shape, src.dtype, base=owner)
        if len(shape) > MAX_NDIM:
            raise TypeError("slicing supports up to %d dimensions on device" % MAX_NDIM)
        out = DeviceArray._new(shape, src.dtype)
        if out.size:
            _lib.get().strided_copy(ptr, _i64arr(strides), out._ptr, len(shape), _i64arr(shape),
                                    src._code())
        return out

    def take(self, indices, axis=0, out=None, mode="raise"):
        """np.take(a, indices, axis=0[, out]): the row gather of `a[indices]` (tnn_gather_rows), optionally INTO an existing
        array — a per-epoch permutation of a resident dataset (utils/data_iterator.py:27-28) then lands at the same HBM
        addresses every epoch, which is what lets a hipGraph captured over the epoch's batches be replayed."""
        if mode != "raise":
            raise TypeError("take: only mode 'raise' is implemented on device")
        src = self._contig()
        if axis is None and src.ndim != 1:
            src, axis = src.ravel(), 0
        elif axis is None:
            axis = 0
        if src.ndim < 1:
            raise IndexError("too many indices for array")
        axis = int(axis)
        if not -src.ndim <= axis < src.ndim:
            raise np.exceptions.AxisError("axis %d is out of bounds for array of dimension %d" % (axis, src.ndim))
        axis %= src.ndim
        if axis != 0 or not DeviceArray._is_rows_key(indices):
            # any other axis or index shape: one gather of a[:, ..., indices]
            res = _index_gather(src, (slice(None),) * axis + (indices,))
            if out is None:
                return res
            if (not isinstance(out, DeviceArray) or out.shape != res.shape or out.dtype != src.dtype or out._t
                    or out._hv is not None):
                raise ValueError("take: `out` must be a dense device array of shape %s and dtype %s"
                                 % (res.shape, src.dtype))
            if res.size:
                _lib.get().memcpy_d2d(out._ptr, res._ptr, res.nbytes)
            return out
        idx = src._index_array(indices)
        shape = (idx.size,) + src.shape[1:]
        if out is None:
            out = DeviceArray._new(shape, src.dtype)
        elif (not isinstance(out, DeviceArray) or out.shape != shape or out.dtype != src.dtype or out._t
              or out._hv is not None):
            raise ValueError("take: `out` must be a dense device array of shape %s and dtype %s" % (shape, src.dtype))
        if out.size:
            _lib.get().gather_rows(src._ptr, idx._ptr, out._ptr, idx.size, _prod(src.shape[1:]), src.shape[0],
                                   src._code())
        return out

    def __setitem__(self, key, value):
        if self._t or self._hv is not None:
            raise TypeError("cannot assign into a transposed view or host scalar")
        if self._tag is READONLY_COPY:
            raise ValueError("assignment destination is a read-only COPY (a padded trainer's logical parameter block): "
                             "use MLPTrainer.set_param(layer, key, value)")
        lib = _lib.get()
        if DeviceArray._is_advanced(key) and DeviceArray._is_rows_key(key):
            idx = self._index_array(key)
            if isinstance(key, DeviceArray) or np.unique(np.asarray(key) % max(self.shape[0], 1)).size != idx.size:
                # indices that may repeat: numpy's assignment, the last one wins (deterministic scatter)
                _index_scatter(self, idx, value)
                return
            row_shape = (idx.size,) + self.shape[1:]
            val = asarray(value).astype(self.dtype)._broadcast_to(row_shape)
            if val.size:
                lib.scatter_rows(val._ptr, idx._ptr, self._ptr, idx.size, _prod(self.shape[1:]),
                                 self.shape[0], self._code())
            return
        if not _ix.is_basic(key):
            _index_scatter(self, key, value)
            return
        offset, shape, strides = self._basic_index(key)
        if _prod(shape) == 0:
            return
        val = asarray(value).astype(self.dtype)._broadcast_to(shape)
        ptr = self._ptr + offset * self.itemsize
        if strides == _dense_strides(shape):
            lib.memcpy_d2d(ptr, val._dev(), _prod(shape) * self.itemsize)
        else:
            lib.strided_scatter(val._dev(), ptr, _i64arr(strides), len(shape), _i64arr(shape), self._code())

    # ------------------------------------------------------------------ arithmetic
    def __add__(self, o): return _binary(_lib.ADD, self, o)
    def __radd__(self, o): return _binary(_lib.ADD, o, self)
    def __sub__(self, o): return _binary(_lib.SUB, self, o)
    def __rsub__(self, o): return _binary(_lib.SUB, o, self)
    def __mul__(self, o): return _binary(_lib.MUL, self, o)
    def __rmul__(self, o): return _binary(_lib.MUL, o, self)
    def __truediv__(self, o): return _binary(_lib.DIV, self, o)
    def __rtruediv__(self, o): return _binary(_lib.DIV, o, self)
    def __pow__(self, o): return _binary(_lib.POW, self, o)
    def __rpow__(self, o): return _binary(_lib.POW, o, self)
    def __neg__(self): return _unary(_lib.NEG, self)
    def __pos__(self): return self
    def __abs__(self): return _unary(_lib.ABS, self)
    def __matmul__(self, o): return matmul(self, o)
    def __rmatmul__(self, o): return matmul(o, self)

    def __iadd__(self, o): return _binary(_lib.ADD, self, o, out=self)
    def __isub__(self, o): return _binary(_lib.SUB, self, o, out=self)
    def __imul__(self, o): return _binary(_lib.MUL, self, o, out=self)
    def __itruediv__(self, o): return _binary(_lib.DIV, self, o, out=self)

    def __gt__(self, o): return _compare(_lib.GT, self, o)
    def __ge__(self, o): return _compare(_lib.GE, self, o)
    def __lt__(self, o): return _compare(_lib.LT, self, o)
    def __le__(self, o): return _compare(_lib.LE, self, o)
    def __eq__(self, o): return False if o is None else _compare(_lib.EQ, self, o)
    def __ne__(self, o): return True if o is None else _compare(_lib.NE, self, o)

    def __and__(self, o):   # bool masks: a & b  ==  a * b on {0,1}
        a, b = asarray(self), asarray(o)
        if a.dtype != np.bool_ or b.dtype != np.bool_:
            raise TypeError("& is only defined for boolean device arrays")
        return _compare(_lib.NE, _binary(_lib.MUL, a, b), 0.0)

    __rand__ = __and__

    # ------------------------------------------------------------------ reductions & friends
    def sum(self, axis=None, keepdims=False, dtype=None, out=None):
        return _reduce(_lib.RSUM, self, axis, keepdims)

    def max(self, axis=None, keepdims=False, out=None):
        return _reduce(_lib.RMAX, self, axis, keepdims)

    def min(self, axis=None, keepdims=False, out=None):
        return _reduce(_lib.RMIN, self, axis, keepdims)

    def mean(self, axis=None, keepdims=False):
        s = self.sum(axis=axis, keepdims=keepdims)
        n = self.size // max(s.size, 1)
        return s / float(n)

    def argmax(self, axis=None):
        return argmax(self, axis)

    def clip(self, min=None, max=None):
        return clip(self, min, max)

    def dot(self, o):
        return _np_dot(self, o)

    # ------------------------------------------------------------------ numpy protocols
    def __array_ufunc__(self, ufunc, method, *inputs, **kwargs):
        out = kwargs.pop("out", None)
        if kwargs:
            kwargs = {k: v for k, v in kwargs.items() if v is not None}
        if out is not None:
            if len(out) != 1 or not isinstance(out[0], DeviceArray):
                return NotImplemented
            out = out[0]
        if method == "__call__" and not kwargs:
            if ufunc in _UFUNC_BINARY and len(inputs) == 2:
                return _binary(_UFUNC_BINARY[ufunc], inputs[0], inputs[1], out=out)
            if ufunc in _UFUNC_COMPARE and len(inputs) == 2 and out is None:
                return _compare(_UFUNC_COMPARE[ufunc], inputs[0], inputs[1])
            if ufunc in _UFUNC_UNARY and len(inputs) == 1:
                res = _unary(_UFUNC_UNARY[ufunc], inputs[0])
                if out is not None:
                    out[...] = res
                    return out
                return res
            if ufunc is np.matmul and len(inputs) == 2 and out is None:
                return matmul(inputs[0], inputs[1])
            if ufunc is np.positive and len(inputs) == 1:
                return asarray(inputs[0])
            if ufunc is np.logical_and and len(inputs) == 2:
                return asarray(inputs[0]).__and__(inputs[1])
        if method == "reduce" and len(inputs) == 1 and ufunc in _UFUNC_REDUCE:
            axis = kwargs.get("axis", 0)
            return _reduce(_UFUNC_REDUCE[ufunc], asarray(inputs[0]), axis, bool(kwargs.get("keepdims", False)))
        raise TypeError("ufunc %s (method %s) has no device implementation; "
                        "convert explicitly with np.asarray(x) if a host copy is intended"
                        % (ufunc.__name__, method))

    def __array_function__(self, func, types, args, kwargs):
        impl = _ARRAY_FUNCTIONS.get(func)
        if impl is None:
            raise TypeError("numpy.%s has no device implementation; convert explicitly with "
                            "np.asarray(x) if a host copy is intended" % func.__name__)
        return impl(*args, **kwargs)


# ---------------------------------------------------------------------- creation helpers
def empty(shape, dtype=None):
    if type(shape) is not tuple:                     # (the hot callers pass tuples: no ABC instance check for them)
        shape = (shape,) if isinstance(shape, numbers.Integral) else tuple(shape)
    return DeviceArray._new(shape, dtype or _default_float)


def full(shape, value, dtype=None):
    out = empty(shape, dtype)
    if out.size:
        _lib.get().fill(out._ptr, float(value), out.size, out._code())
    return out


def zeros(shape, dtype=None):
    return full(shape, 0.0, dtype)


def ones(shape, dtype=None):
    return full(shape, 1.0, dtype)


def zeros_like(a, dtype=None, **_):
    a = asarray(a)
    return zeros(a.shape, dtype or a.dtype)


def ones_like(a, dtype=None, **_):
    a = asarray(a)
    return ones(a.shape, dtype or a.dtype)


def asarray(obj, dtype=None):
    """Device counterpart of np.asarray (core/tensor.py:20).

    Floating host data is stored as the default device float unless `dtype` says otherwise; integer
    arrays stay int64 (index / label arrays) and are cast to float by the first arithmetic op; Python and
    numpy scalars stay on the host as kernel arguments.
    """
    if isinstance(obj, DeviceArray):
        if dtype is not None and dtype is not obj.dtype and np.dtype(dtype) != obj.dtype:
            return obj.astype(dtype)
        return obj
    if _is_scalar_like(obj):
        s = DeviceArray._scalar(obj)
        if dtype is not None and np.dtype(dtype).kind == "f":
            s.dtype = np.dtype(dtype)
        return s
    host = np.asarray(obj)
    if host.dtype == object:
        raise TypeError("cannot move an object array to the device")
    if dtype is not None:
        target = np.dtype(dtype)
    elif host.dtype.kind == "f":
        target = _default_float
    elif host.dtype.kind in "iu":
        target = np.dtype(np.int64)
    elif host.dtype.kind == "b":
        target = np.dtype(np.bool_)
    else:
        raise TypeError("unsupported host dtype %s" % host.dtype)
    if target not in _CODE:
        raise TypeError("unsupported device dtype %s" % target)
    host = np.ascontiguousarray(host, dtype=target)
    out = DeviceArray._new(host.shape, target)
    if host.size:
        _lib.get().memcpy_h2d(out._ptr, host.ctypes.data, host.nbytes)
    return out


class LazyArray(DeviceArray):
    """An array whose producing launch is deferred until something first asks for its buffer (`_ptr`).

    Used for two things: the gradient views of a Model's arena (`view` / `defer`, see core/model.py) and, first, the logits of
    a classifier head in TRAIN mode (core/nn.py, core/ops.py dense_(lazy=True)).  When the
    loss node gets there first it produces them together with the loss and the head's backward in one launch
    (ops.softmax_nll_); any other first use — printing, argmax, a custom loss — runs the ordinary GEMM, so the values are the
    same either way.  The deferral is visible only to code that mutates the producer's inputs IN PLACE between forward()
    and the first use of the logits (they would be computed from the mutated operands)."""
    __slots__ = ("_thunk",)

    def _get_ptr(self):
        thunk = self._thunk
        if thunk is not None:
            self._thunk = None
            thunk(self)
        return DeviceArray._ptr.__get__(self, DeviceArray)

    def _set_ptr(self, value):
        DeviceArray._ptr.__set__(self, value)

    _ptr = property(_get_ptr, _set_ptr)

    @classmethod
    def deferred(cls, shape, dtype, thunk):
        self = cls._new(shape, dtype)          # the buffer exists; only its content is pending
        self._thunk = thunk
        if _lib.capturing:                     # graph.py re-arms what is still pending when the capture ends
            _CAPTURE_LAZIES.append(weakref.ref(self))
        return self

    @classmethod
    def view(cls, base, offset, shape):
        """A view of `shape` over base's buffer from element `offset` on whose content may be declared pending (`defer`):
        the gradient views of a Model's arena (core/model.py) — the launch that fills them can then wait for the optimizer."""
        ptr = DeviceArray._ptr.__get__(base, DeviceArray) if type(base) is not DeviceArray else base._ptr
        self = cls._raw(ptr + offset * base.dtype.itemsize, shape, base.dtype, base=base)
        self._thunk = None
        return self

    def defer(self, thunk):
        """Declare the content pending: `thunk(self)` runs before the first access to the buffer (or never, see drop)."""
        self._thunk = thunk

    def drop(self):
        """Forget a pending producer (the content is about to be overwritten or is no longer wanted)."""
        self._thunk = None

    @property
    def pending(self):
        return self._thunk is not None

    def fulfilled_ptr(self):
        """The buffer for the launch that fulfils the deferral some other way (and ends it)."""
        self._thunk = None
        return DeviceArray._ptr.__get__(self, DeviceArray)

    def __del__(self):
        self._thunk = None
        DeviceArray.__del__(self)


_CAPTURE_LAZIES = []       # weak references to the LazyArray.deferred objects created inside the open hipGraph capture


def take_capture_lazies():
    """End of a capture (graph.py): the deferred arrays created inside it that NOTHING has asked for yet, with their producers.
    Their launch is not in the graph; a replay refreshes the operands they would be computed from, so the captured function
    re-arms them after every replay — a later read then computes them from the replay's data (eagerly, once) instead of
    returning what the first read after some earlier replay produced."""
    out = []
    for ref in _CAPTURE_LAZIES:
        arr = ref()
        if arr is not None and arr._thunk is not None:
            out.append((ref, arr._thunk))
    del _CAPTURE_LAZIES[:]
    return out


def gather_scalars(arrays, out=None, pointers=None):
    """One vector from n 0-d device arrays that live in n separate buffers (a loop's per-step losses): ONE launch
    (tnn_gather_scalars) instead of n 4-byte copies.  `pointers`: a device array of their addresses from an earlier call
    (returned as the second value) — the arrays of a replayed hipGraph keep their addresses, so the list is uploaded once.
    Returns (vector, pointers)."""
    if pointers is None:
        arrays = [asarray(a) for a in arrays]
        if any(a._hv is not None or a.size != 1 for a in arrays) or len({a.dtype for a in arrays}) != 1:
            raise TypeError("gather_scalars: n one-element device arrays of one dtype are required")
        pointers = asarray(np.array([a._dev() for a in arrays], dtype=np.int64))
        pointers._aux = arrays                       # the buffers stay alive as long as their address list does
    n = pointers.size
    if out is None:
        out = DeviceArray._new((n,), pointers._aux[0].dtype)
    _lib.get().gather_scalars(pointers._ptr, out._ptr, n, out._code())
    return out, pointers


def from_ptr(ptr, shape, dtype, owner):
    """View over memory owned by something else (e.g. the trainer's arenas); `owner` is kept alive."""
    return DeviceArray._raw(ptr, shape, dtype, base=owner)


# ---------------------------------------------------------------------- kernels: elementwise
def _broadcast_strides(src_shape, dst_shape):
    nd = len(dst_shape)
    if len(src_shape) > nd:
        raise ValueError("cannot broadcast %s to %s" % (src_shape, dst_shape))
    padded = (1,) * (nd - len(src_shape)) + tuple(src_shape)
    dense = (0,) * (nd - len(src_shape)) + _dense_strides(src_shape)
    st = []
    for p, d, s in zip(padded, dst_shape, dense):
        if p == d:
            st.append(s if p != 1 else 0)
        elif p == 1:
            st.append(0)
        else:
            raise ValueError("operands could not be broadcast together with shapes %s %s"
                             % (src_shape, dst_shape))
    return tuple(st)


def _float_result_dtype(a, b):
    cands = [x.dtype for x in (a, b) if x._hv is None and x.dtype.kind == "f"]
    if not cands:
        return _default_float
    return np.dtype(np.float64) if np.dtype(np.float64) in cands else np.dtype(np.float32)


_PY_BIN = {
    _lib.ADD: lambda x, y: x + y, _lib.SUB: lambda x, y: x - y, _lib.MUL: lambda x, y: x * y,
    _lib.DIV: lambda x, y: x / y, _lib.POW: lambda x, y: x ** y,
    _lib.MAX: lambda x, y: x if x >= y else y, _lib.MIN: lambda x, y: x if x <= y else y,
}
_PY_CMP = {
    _lib.GT: lambda x, y: x > y, _lib.GE: lambda x, y: x >= y, _lib.LT: lambda x, y: x < y,
    _lib.LE: lambda x, y: x <= y, _lib.EQ: lambda x, y: x == y, _lib.NE: lambda x, y: x != y,
}
_SWAP_CMP = {_lib.GT: _lib.LT, _lib.GE: _lib.LE, _lib.LT: _lib.GT, _lib.LE: _lib.GE,
             _lib.EQ: _lib.EQ, _lib.NE: _lib.NE}


def _binary(op, a, b, out=None):
    a, b = asarray(a), asarray(b)
    lib = _lib.get()
    if a._hv is not None and b._hv is not None:
        res = DeviceArray._scalar(_PY_BIN[op](a._hv, b._hv))
        if out is not None:
            out[...] = res
            return out
        return res
    dt = _float_result_dtype(a, b)
    if out is not None:
        if out.dtype.kind != "f":
            raise TypeError("in-place arithmetic needs a floating device array")
        dt = out.dtype
    if a._hv is not None or b._hv is not None:
        arr, s, lhs = (b, a._hv, 1) if a._hv is not None else (a, b._hv, 0)
        arr = arr._as_float(dt)._contig()
        res = out if out is not None else DeviceArray._new(arr.shape, dt)
        if out is not None and out.shape != arr.shape:
            raise ValueError("non-broadcastable output operand")
        if res.size:
            lib.ewise_scalar(op, arr._ptr, float(s), lhs, res._ptr, res.size, res._code())
        return res
    a, b = a._as_float(dt)._contig(), b._as_float(dt)._contig()
    shape = np.broadcast_shapes(a.shape, b.shape)
    if len(shape) > MAX_NDIM:
        raise TypeError("elementwise ops support up to %d dimensions on device" % MAX_NDIM)
    if out is not None:
        if out.shape != tuple(shape) or out._t:
            raise ValueError("non-broadcastable output operand with shape %s" % (out.shape,))
        res = out
    else:
        res = DeviceArray._new(shape, dt)
    if res.size:
        if op == _lib.ADD and out is not None and a is out and b.shape == out.shape:
            lib.axpy(out._ptr, 1.0, b._ptr, out.size, out._code())     # grad += g, param += step
        else:
            lib.ewise_binary(op, a._ptr, _i64arr(_broadcast_strides(a.shape, shape)), b._ptr,
                             _i64arr(_broadcast_strides(b.shape, shape)), res._ptr, len(shape),
                             _i64arr(shape), res._code())
    return res


def _compare(cmp, a, b):
    a, b = asarray(a), asarray(b)
    lib = _lib.get()
    if a._hv is not None and b._hv is not None:
        return asarray(np.asarray(_PY_CMP[cmp](a._hv, b._hv)))
    dt = _float_result_dtype(a, b)
    if a._hv is not None or b._hv is not None:
        if a._hv is not None:
            arr, s, cmp = b, a._hv, _SWAP_CMP[cmp]
        else:
            arr, s = a, b._hv
        arr = arr._as_float(dt)._contig()
        res = DeviceArray._new(arr.shape, np.bool_)
        if res.size:
            lib.compare_scalar(cmp, arr._ptr, float(s), res._ptr, res.size, arr._code())
        return res
    a, b = a._as_float(dt)._contig(), b._as_float(dt)._contig()
    shape = np.broadcast_shapes(a.shape, b.shape)
    if len(shape) > MAX_NDIM:
        raise TypeError("comparisons support up to %d dimensions on device" % MAX_NDIM)
    res = DeviceArray._new(shape, np.bool_)
    if res.size:
        lib.ewise_compare(cmp, a._ptr, _i64arr(_broadcast_strides(a.shape, shape)), b._ptr,
                          _i64arr(_broadcast_strides(b.shape, shape)), res._ptr, len(shape),
                          _i64arr(shape), a._code())
    return res


_PY_UNA = {
    _lib.NEG: lambda x: -x, _lib.EXP: math.exp, _lib.LOG: math.log, _lib.SQRT: math.sqrt,
    _lib.SQUARE: lambda x: x * x, _lib.ABS: abs, _lib.RECIP: lambda x: 1.0 / x,
    _lib.SIGMOID: lambda x: 1.0 / (1.0 + math.exp(-x)), _lib.TANH: math.tanh, _lib.COPY: lambda x: x,
}


def _unary(op, a):
    a = asarray(a)
    if a._hv is not None:
        return DeviceArray._scalar(_PY_UNA[op](a._hv))
    a = a._as_float()._contig()
    res = DeviceArray._new(a.shape, a.dtype)
    if res.size:
        _lib.get().ewise_unary(op, a._ptr, res._ptr, res.size, res._code())
    return res


def exp(a): return _unary(_lib.EXP, a)
def log(a): return _unary(_lib.LOG, a)
def sqrt(a): return _unary(_lib.SQRT, a)
def sigmoid(a): return _unary(_lib.SIGMOID, a)
def tanh(a): return _unary(_lib.TANH, a)
def maximum(a, b): return _binary(_lib.MAX, a, b)
def minimum(a, b): return _binary(_lib.MIN, a, b)


def clip(a, a_min=None, a_max=None, **_):
    a = asarray(a)
    if a._hv is not None:
        v = a._hv
        if a_min is not None:
            v = max(v, a_min)
        if a_max is not None:
            v = min(v, a_max)
        return DeviceArray._scalar(v)
    a = a._as_float()._contig()
    res = DeviceArray._new(a.shape, a.dtype)
    if res.size:
        _lib.get().clip(a._ptr, int(a_min is not None), float(a_min or 0.0), int(a_max is not None),
                        float(a_max or 0.0), res._ptr, res.size, res._code())
    return res


def clip_bwd(grad, x, a_min=None, a_max=None):
    """grad * [(x >= a_min) & (x <= a_max)]  — core/ops.py:336-343 with the mask recomputed from x."""
    x = asarray(x)._as_float()._contig()
    grad = asarray(grad)._as_float(x.dtype)._broadcast_to(x.shape)
    res = DeviceArray._new(x.shape, x.dtype)
    if res.size:
        _lib.get().clip_bwd(grad._dev(), x._ptr, int(a_min is not None), float(a_min or 0.0),
                            int(a_max is not None), float(a_max or 0.0), res._ptr, res.size, res._code())
    return res


RELU_SIGN = "relu-mask-in-sign-bit"      # _tag of a fused Dense+ReLU output (core/ops.py dense_(relu=True))


def mul_signmask(grad, y):
    """grad where the sign bit of y is clear, else 0 (y: sign-encoded ReLU output)."""
    y = asarray(y)._contig()
    grad = asarray(grad)._as_float(y.dtype)._broadcast_to(y.shape)._contig()
    res = DeviceArray._new(y.shape, y.dtype)
    if res.size:
        _lib.get().mul_signmask(grad._ptr, y._ptr, res._ptr, res.size, res._code())
    return res


def mul_mask(grad, mask):
    """grad * mask for a boolean device mask (vjps of maximum/minimum/max/min)."""
    mask = asarray(mask)
    if mask.dtype != np.bool_:
        return _binary(_lib.MUL, grad, mask)
    grad = asarray(grad)
    shape = tuple(np.broadcast_shapes(grad.shape, mask.shape))
    g = grad._as_float()._broadcast_to(shape)
    m = mask._broadcast_to(shape)
    res = DeviceArray._new(shape, g.dtype)
    if res.size:
        _lib.get().mul_mask(g._dev(), m._dev(), res._ptr, res.size, res._code())
    return res


# ---------------------------------------------------------------------- kernels: reductions
def _reduce(rop, a, axis=None, keepdims=False):
    a = asarray(a)
    if a._hv is not None:
        return a
    a = a._as_float()._contig()
    lib = _lib.get()
    if axis is None:
        axes = tuple(range(a.ndim))
    elif isinstance(axis, (tuple, list)):
        axes = tuple(sorted(int(x) % a.ndim for x in axis))
    else:
        if a.ndim == 0:
            raise np.exceptions.AxisError("axis %d is out of bounds for array of dimension 0" % axis)
        if not -a.ndim <= int(axis) < a.ndim:
            raise np.exceptions.AxisError("axis %d is out of bounds for array of dimension %d"
                                          % (axis, a.ndim))
        axes = (int(axis) % a.ndim,)
    if a.ndim == 0 or not axes:
        return a
    contiguous = axes == tuple(range(axes[0], axes[0] + len(axes)))
    cur = a
    groups = [axes] if contiguous else [(ax,) for ax in reversed(axes)]
    for grp in groups:
        lo, hi = grp[0], grp[-1] + 1
        outer, red, inner = _prod(cur.shape[:lo]), _prod(cur.shape[lo:hi]), _prod(cur.shape[hi:])
        if red == 0 and rop != _lib.RSUM:
            raise ValueError("zero-size array to reduction operation which has no identity")
        kept = cur.shape[:lo] + (1,) * (hi - lo) + cur.shape[hi:]
        res = DeviceArray._new(kept, cur.dtype)
        if res.size:
            lib.reduce(rop, cur._ptr, res._ptr, outer, red, inner, cur._code())
        cur = res
    if not keepdims:
        cur = cur.reshape([s for i, s in enumerate(cur.shape) if i not in axes])
    return cur


def argmax(a, axis=None, **_):
    a = asarray(a)._as_float()._contig()
    if axis is None:
        a2, out_shape = a.reshape(1, a.size), ()
    elif a.ndim >= 1 and int(axis) % a.ndim == a.ndim - 1:
        a2, out_shape = a.reshape(_prod(a.shape[:-1]), a.shape[-1]), a.shape[:-1]
    else:
        perm = [i for i in range(a.ndim) if i != int(axis) % a.ndim] + [int(axis) % a.ndim]
        moved = a.transpose(perm)._contig()
        a2, out_shape = moved.reshape(_prod(moved.shape[:-1]), moved.shape[-1]), moved.shape[:-1]
    res = DeviceArray._new((a2.shape[0],), np.int64)
    if res.size:
        _lib.get().argmax_rows(a2._ptr, res._ptr, a2.shape[0], a2.shape[1], a2._code())
    return res.reshape(out_shape)


# ---------------------------------------------------------------------- kernels: matmul
def matmul(a, b, swap_a=False, swap_b=False):
    """a @ b by numpy's matmul rules.  1-D / 2-D operands: one tnn_gemm, a lazy `.T` on either side selects the NT / TN / TT
    kernel.  N-d operands (stacks of matrices, broadcast batch dimensions): planned by batching.py — one 2-D GEMM where the
    stack folds into the rows, one tnn_gemm_batched launch otherwise, a loop of tnn_gemm for few large matrices.
    swap_a / swap_b: use that operand with its last two axes exchanged, by stride (the vjps of core/ops.py dot_)."""
    a, b = asarray(a), asarray(b)
    if a._hv is not None or b._hv is not None or a.ndim == 0 or b.ndim == 0:
        raise ValueError("matmul: input operand does not have enough dimensions")
    if a.ndim > 2 or b.ndim > 2 or swap_a or swap_b:
        return _matmul_nd(a, b, swap_a, swap_b)
    dt = _float_result_dtype(a, b)
    a, b = a._as_float(dt), b._as_float(dt)
    squeeze_m = a.ndim == 1
    squeeze_n = b.ndim == 1
    if squeeze_m:
        a = a.reshape(1, a.shape[0])
    if squeeze_n:
        b = b.reshape(b.shape[0], 1)
    M, K = a.shape
    K2, N = b.shape
    if K != K2:
        raise ValueError("matmul: Input operand 1 has a mismatch in its core dimension 0 "
                         "(size %d is different from %d)" % (K2, K))
    res = DeviceArray._new((M, N), dt)
    if res.size:
        ta, tb = int(a._t), int(b._t)
        lda = M if ta else K       # stored [K,M] when transposed
        ldb = K if tb else N       # stored [N,K] when transposed
        _lib.get().gemm(ta, tb, M, N, K, 1.0, a._ptr, lda, b._ptr, ldb, 0.0, res._ptr, N, res._code())
    if squeeze_m and squeeze_n:
        return res.reshape(())
    if squeeze_m:
        return res.reshape(N)
    if squeeze_n:
        return res.reshape(M)
    return res


BMM_ROUTE = None      # tests / probes: "batched" or "loop" overrides the planner's choice between those two routes
BMM_FORM = 0          # tests / probes: TNN_BMM_FORM_* of the batched launches (0: the library picks by shape)


def _matmul_nd(a, b, swap_a, swap_b):
    """The N-d product (and the 2-D one with an exchanged operand): plan on the host, then one of the three routes."""
    dt = _float_result_dtype(a, b)
    a, b = a._as_float(dt), b._as_float(dt)
    lib = _lib.get()
    plan = _bt.plan_matmul(a.shape, b.shape, a_t=a._t, b_t=b._t, swap_a=swap_a, swap_b=swap_b, native=lib.has_bmm)
    if plan.copy_a or plan.copy_b:     # (dense arrays and 2-D lazy transposes are always expressible by stride)
        raise TypeError("matmul: operand layout not expressible by strides")
    if len(plan.out_shape) > MAX_NDIM:
        raise TypeError("matmul supports results of up to %d dimensions on device" % MAX_NDIM)
    res = DeviceArray._new(plan.out_shape, dt)
    if not res.size:
        return res
    M, N, K = plan.M, plan.N, plan.K
    code = res._code()
    if K == 0:
        lib.fill(res._ptr, 0.0, res.size, code)
        return res
    route = plan.route
    if route != "gemm2d" and BMM_ROUTE is not None:
        route = BMM_ROUTE
    if route == "gemm2d":
        lib.gemm(plan.ta, plan.tb, M, N, K, 1.0, a._ptr, plan.lda, b._ptr, plan.ldb, 0.0, res._ptr, N, code)
    elif route == "batched":
        nb = len(plan.batch)
        lib.gemm_batched(plan.ta, plan.tb, M, N, K, a._ptr, plan.lda, b._ptr, plan.ldb, res._ptr, nb,
                         _i64arr(plan.batch), _i64arr(plan.a_bstrides), _i64arr(plan.b_bstrides), code, BMM_FORM)
    else:
        isz = res.itemsize
        step = M * N * isz
        gemm, pa, pb, pc = lib.gemm, a._ptr, b._ptr, res._ptr
        for i, (oa, ob) in enumerate(_bt.batch_offsets(plan)):
            gemm(plan.ta, plan.tb, M, N, K, 1.0, pa + oa * isz, plan.lda, pb + ob * isz, plan.ldb, 0.0,
                 pc + i * step, N, code)
    return res


def _np_dot(a, b):
    """np.dot for operands of at most two dimensions (where it is matmul); numpy's N-d dot is a different contraction."""
    a, b = asarray(a), asarray(b)
    if a.ndim > 2 or b.ndim > 2:
        raise TypeError("np.dot with an N-d operand is not matmul (it contracts the last axis of a with the second-to-last "
                        "of b for every pair of stacks) and has no device implementation; use a @ b / np.matmul")
    return matmul(a, b)


# ---------------------------------------------------------------------- kernels: convolution and pooling (csrc/tnn_conv.hip)
CONV_ROUTE = None     # tests / probes: "native" or "composed" overrides the planner's choice (conv.py)
CONV_FORM = 0         # tests / probes: TNN_CONV_FORM_* of the float32 launches (0: the library picks by channel count)
CONV_SPLITS = None    # tests / probes: ranges of the filter gradient's contraction (None: conv.filter_splits)


def _conv_operands(*arrays):
    """The operands as dense arrays of one float dtype (None stays None)."""
    present = [asarray(a) for a in arrays if a is not None]
    dt = None
    for a in present:
        if a.dtype.kind == "f":
            dt = a.dtype if dt is None or a.dtype.itemsize > dt.itemsize else dt
    dt = dt or _default_float
    return dt, [None if a is None else asarray(a)._as_float(dt)._contig() for a in arrays]


def _conv_plan(x_shape, w_shape, b_shape, stride, padding, route):
    return _cv.plan_conv2d(x_shape, w_shape, b_shape, stride, padding, native=_lib.get().has_conv,
                           route=route or CONV_ROUTE)


def _pad_hw(x, ph, pw, value=0.0):
    if not ph and not pw:
        return x
    return _np_pad(x, ((0, 0), (0, 0), (ph, ph), (pw, pw)), constant_values=value)


def conv2d(x, w, b=None, stride=1, padding=0, relu=False, route=None):
    """y[n, f] = b[f] + sum_c x[n, c] (*) w[f, c]: 2-D cross-correlation of an NCHW batch with [F, C, KH, KW] filters, zero
    padding, output extent (H + 2 p - KH) // s + 1.  relu=True: clip(., 0) in the same launch, the vjp mask z >= 0 kept in the
    sign bit of zero (RELU_SIGN, as the fused Dense does).  One tnn_conv2d_fwd launch, or the tap loop of conv.py's composed
    route (`route`, here and in the functions below: "native" / "composed" for this call, None = CONV_ROUTE / the planner)."""
    dt, (x, w, b) = _conv_operands(x, w, b)
    plan = _conv_plan(x.shape, w.shape, None if b is None else b.shape, stride, padding, route)
    if plan.route == "native":
        out = DeviceArray._new(plan.out_shape, dt)
        if out.size:
            _lib.get().conv2d_fwd(x._ptr, w._ptr, None if b is None else b._ptr, out._ptr, *plan.geometry(),
                                  1 if relu else 0, out._code(), CONV_FORM)
        if relu:
            out._tag = RELU_SIGN
        return out
    n, ohw = plan.N, plan.OH * plan.OW
    xp = _pad_hw(x, plan.ph, plan.pw)
    acc = None
    for kh, kw, rows, cols in _cv.taps(plan):
        patch = xp[:, :, rows, cols].reshape(n, plan.C, ohw)
        term = matmul(w[:, :, kh, kw], patch)                  # [F, C] @ [N, C, OH OW]
        acc = term if acc is None else acc + term
    out = acc.reshape(plan.out_shape)
    if b is not None:
        out = out + b.reshape(1, plan.F, 1, 1)
    if relu:                                               # the same sign encoding: z < 0 -> -0.0, z >= 0 -> |z|
        out = clip(out, 0.0) * (1.0 - 2.0 * (out < 0.0).astype(dt))
        out._tag = RELU_SIGN
    return out


def conv2d_bwd_data(dy, w, x_shape, stride=1, padding=0, route=None):
    """dx of conv2d for the gradient dy of its output: every input pixel collects dy * w over the taps that reach it."""
    dt, (dy, w) = _conv_operands(dy, w)
    plan = _conv_plan(x_shape, w.shape, None, stride, padding, route)
    if dy.shape != plan.out_shape:
        raise ValueError("conv2d_bwd_data: dy has shape %s, the output of this convolution %s" % (dy.shape, plan.out_shape))
    if plan.route == "native":
        dx = DeviceArray._new((plan.N, plan.C, plan.H, plan.W), dt)
        if dx.size:
            _lib.get().conv2d_bwd_data(dy._ptr, w._ptr, dx._ptr, *plan.geometry(), dx._code(), CONV_FORM)
        return dx
    dxp = zeros((plan.N, plan.C, plan.H + 2 * plan.ph, plan.W + 2 * plan.pw), dt)
    dy3 = dy.reshape(plan.N, plan.F, plan.OH * plan.OW)
    for kh, kw, rows, cols in _cv.taps(plan):
        key = (slice(None), slice(None), rows, cols)
        term = matmul(w[:, :, kh, kw].T, dy3).reshape(plan.N, plan.C, plan.OH, plan.OW)
        dxp[key] = dxp[key] + term
    return dxp[:, :, plan.ph:plan.ph + plan.H, plan.pw:plan.pw + plan.W]


def _grad_dest(out, shape, dt):
    """`out` when it is a dense array of this many elements and dtype that the launch may write (an arena view), else None."""
    if (out is not None and isinstance(out, DeviceArray) and type(out) is DeviceArray and out.size == _prod(shape)
            and out.dtype == dt and not out._t and out._hv is None and out._tag is not READONLY_COPY):
        return out
    return None


def _dest(need, out, shape, dt, exact=False):
    """What a launch writes a gradient of this shape into: None when it is not needed, `out` when it was lent and _grad_dest
    accepts it (exact: and it has exactly this shape — the attention kernels address it with the operand's strides), else a
    new array."""
    if not need:
        return None
    d = _grad_dest(out, shape, dt)
    if d is None or (exact and tuple(d.shape) != tuple(shape)):
        return DeviceArray._new(shape, dt)
    return d


def conv2d_bwd_filter(x, dy, w_shape, stride=1, padding=0, with_db=True, dw_out=None, db_out=None, route=None):
    """(dw, db) of conv2d: dw[f, c, kh, kw] = sum over batch and output pixels of dy * the input under that tap, db[f] = the
    sum of dy (None when with_db is false) — both from ONE tnn_conv2d_bwd_filter launch, whose split contraction is reduced
    in a fixed order (run-to-run identical bits).  dw_out / db_out: dense arrays the results are written into."""
    dt, (x, dy) = _conv_operands(x, dy)
    plan = _conv_plan(x.shape, w_shape, None, stride, padding, route)
    if dy.shape != plan.out_shape:
        raise ValueError("conv2d_bwd_filter: dy has shape %s, the output of this convolution %s" % (dy.shape, plan.out_shape))
    w_shape = (plan.F, plan.C, plan.KH, plan.KW)
    if plan.route == "native":
        lib = _lib.get()
        dw, db = _dest(True, dw_out, w_shape, dt), _dest(with_db, db_out, (plan.F,), dt)
        splits = 1
        if dt == np.float32 and plan.N:
            splits = CONV_SPLITS if CONV_SPLITS is not None else _cv.filter_splits(plan, with_db, CONV_FORM)
        nbytes = _cv.filter_workspace_bytes(plan, with_db, CONV_FORM, splits)
        ws = None
        if nbytes:
            ws = DeviceArray._new((nbytes // 4,), np.float32)
            counters = (nbytes - splits * _cv.tiles(plan.F, plan.C * plan.KH * plan.KW + int(with_db), CONV_FORM)
                        * _cv.TILE_ELEMS * 4) // 4
            lib.fill(ws._ptr, 0.0, counters, F32)              # the arrival counters start at zero (and end there)
        lib.conv2d_bwd_filter(x._ptr, dy._ptr, dw._ptr, None if db is None else db._ptr, None if ws is None else ws._ptr,
                              nbytes, *plan.geometry(), dw._code(), CONV_FORM, splits)
        return dw, db
    xp = _pad_hw(x, plan.ph, plan.pw)
    dy3 = dy.reshape(plan.N, plan.F, plan.OH * plan.OW)
    dw = zeros(w_shape, dt)
    for kh, kw, rows, cols in _cv.taps(plan):
        patch = xp[:, :, rows, cols].reshape(plan.N, plan.C, plan.OH * plan.OW)
        dw[:, :, kh, kw] = matmul(dy3, patch, swap_b=True).sum(axis=0)       # [N, F, C] summed over the batch
    db = dy.sum(axis=(0, 2, 3)) if with_db else None
    return dw, db


def _pool_offsets(plan, kh, kw, dt):
    """[OH, OW] flat offsets h * W + w of tap (kh, kw) of every window (taps in the padding get offsets outside the plane's
    rows or columns; they hold -inf and are never recorded)."""
    h = np.arange(plan.OH) * plan.sh - plan.ph + kh
    w = np.arange(plan.OW) * plan.sw - plan.pw + kw
    return asarray((h[:, None] * plan.W + w[None, :]).astype(dt))


def max_pool2d(x, kernel, stride=None, padding=0, route=None):
    """(y, idx): the maximum of every kernel window of every [H, W] plane (padding = -inf) and the flat offset h * W + w of
    the FIRST maximum of the window in row-major order inside its input plane — numpy's argmax rule.  NaN propagates like
    max.  Native: int32 offsets from tnn_maxpool2d_fwd; composed: a fold of `maximum` over the shifted slices in row-major
    tap order (ties stay with the earlier tap), offsets as whole numbers of x's dtype."""
    x = asarray(x)
    dt, (x,) = _conv_operands(x)
    plan = _cv.plan_pool2d(x.shape, kernel, stride, padding, native=_lib.get().has_conv, route=route or CONV_ROUTE)
    if plan.route == "native":
        y = DeviceArray._new(plan.out_shape, dt)
        idx = DeviceArray._new(plan.out_shape, np.int32)
        if y.size:
            _lib.get().maxpool2d_fwd(x._ptr, y._ptr, idx._ptr, *plan.geometry(), y._code())
        return y, idx
    xp = _pad_hw(x, plan.ph, plan.pw, -math.inf)
    best = idx = None
    for kh, kw, rows, cols in _cv.taps(plan):
        v = xp[:, :, rows, cols]
        off = _pool_offsets(plan, kh, kw, dt)
        if best is None:
            best, idx = v, off._broadcast_to(plan.out_shape)
        else:
            idx = _np_where(v > best, off, idx)
            best = maximum(best, v)
    return best, idx


def max_pool2d_bwd(dy, idx, x_shape, kernel, stride=None, padding=0, route=None):
    """dx of max_pool2d: every window's gradient goes, whole, to the pixel whose offset it recorded; a pixel recorded by several
    (overlapping) windows receives their sum."""
    dt, (dy,) = _conv_operands(dy)
    plan = _cv.plan_pool2d(x_shape, kernel, stride, padding, native=_lib.get().has_conv, route=route or CONV_ROUTE)
    if dy.shape != plan.out_shape or tuple(idx.shape) != plan.out_shape:
        raise ValueError("max_pool2d_bwd: dy %s / idx %s do not match the pooled shape %s" % (dy.shape, idx.shape, plan.out_shape))
    if plan.route == "native":
        if idx.dtype != np.int32:
            raise TypeError("max_pool2d_bwd: the native route takes the int32 offsets of its own forward")
        dx = DeviceArray._new((plan.N, plan.C, plan.H, plan.W), dt)
        if dx.size:
            _lib.get().maxpool2d_bwd(dy._ptr, idx._ptr, dx._ptr, *plan.geometry(), dx._code())
        return dx
    if idx.dtype.kind != "f":
        raise TypeError("max_pool2d_bwd: the composed route takes the offsets of its own forward")
    dxp = zeros((plan.N, plan.C, plan.H + 2 * plan.ph, plan.W + 2 * plan.pw), dt)
    for kh, kw, rows, cols in _cv.taps(plan):
        key = (slice(None), slice(None), rows, cols)
        dxp[key] = dxp[key] + mul_mask(dy, idx == _pool_offsets(plan, kh, kw, idx.dtype))
    return dxp[:, :, plan.ph:plan.ph + plan.H, plan.pw:plan.pw + plan.W]


# ---------------------------------------------------------------------- kernels: fused attention (csrc/tnn_attn.hip)
ATTN_ROUTE = None     # tests / probes: "native" or "composed" overrides the planner's choice (attention.py)
_ATTN_MASKS = {}      # (Tq, Tk, dtype) -> [Tq, Tk] array, 0 where key j <= query i and -inf above the diagonal
_ATTN_MASKS_MAX = 8   # masks kept (4 MiB each at T = 1024); trim_cache() drops them all


def _operands(*arrays):
    """The operands (None stays None) as dense arrays of one float dtype, promoted the way matmul promotes
    (_float_result_dtype)."""
    arrays = [None if a is None else asarray(a) for a in arrays]
    cands = [a.dtype for a in arrays if a is not None and a._hv is None and a.dtype.kind == "f"]
    dt = _default_float if not cands else np.dtype(np.float64) if np.dtype(np.float64) in cands else np.dtype(np.float32)
    return dt, [None if a is None else a._as_float(dt)._contig() for a in arrays]


def _attn_plan(q, k, v, causal, scale, layout, route):
    return _at.plan_attention(q.shape, k.shape, v.shape, causal, scale, layout, native=_lib.get().has_attn,
                              route=route or ATTN_ROUTE)


def _attn_mask(tq, tk, dt):
    key = (tq, tk, dt)
    m = _ATTN_MASKS.get(key)
    if m is None:
        if _lib.capturing:
            raise RuntimeError("attention (composed route): the causal mask of a new (Tq, Tk, dtype) is uploaded from the "
                               "host, which a graph capture cannot do; run one step outside the capture first")
        host = np.zeros((tq, tk), dtype=dt)
        host[np.triu_indices(tq, 1, tk)] = -np.inf
        if len(_ATTN_MASKS) >= _ATTN_MASKS_MAX:
            _ATTN_MASKS.clear()
        m = _ATTN_MASKS[key] = asarray(host, dtype=dt)
    return m


def _attn3(x, plan, rows, width):
    """[B H, rows, width] view of an operand (layout "bthd": a transposed copy)."""
    if plan.layout == "bthd":
        x = x.transpose(0, 2, 1, 3)
    return x.reshape(plan.B * plan.H, rows, width)


def _attn_from3(x3, plan, rows, width):
    if plan.layout == "bthd":
        return x3.reshape(plan.B, plan.H, rows, width).transpose(0, 2, 1, 3)
    return x3.reshape(plan.out_shape[:-2] + (rows, width))


def _attn_scores(q, k, plan):
    """scale q k^T (+ the causal mask) as [B H, Tq, Tk] — the composed route's score array."""
    s = matmul(_attn3(q, plan, plan.Tq, plan.D), _attn3(k, plan, plan.Tk, plan.D), swap_b=True) * plan.scale
    if plan.causal:
        s = s + _attn_mask(plan.Tq, plan.Tk, s.dtype)
    return s


# What differs between the plain and the grouped-query training entry points (the rest is _attn_fwd, _attn_bwd_q, _attn_bwd_kv):
# the planner, the library's three entry points, the prefix of the messages, and whether dk and dv are summed over the group.
_AttnForm = collections.namedtuple("_AttnForm", "plan fwd bwd_q bwd_kv what fold")
_PLAIN = _AttnForm(_attn_plan, "attn_fwd", "attn_bwd_q", "attn_bwd_kv", "attention", False)

VARLEN_ROUTE = None   # tests / probes: "native" or "composed" overrides the planner's choice when lens= is given (varlen.py)


class _Varlen(object):
    """What lens= adds to one call of _attn_fwd / _attn_bwd_q / _attn_bwd_kv: the plan of varlen.py, the device array of the
    lengths, and on the composed route the two masks built from their host values."""
    __slots__ = ("plan", "dev", "lens")

    def __init__(self, form, q, k, v, lens, causal, scale, layout, route):
        what = form.what
        if not isinstance(lens, (_rg.Lengths, DeviceArray)):
            raise TypeError("%s: lens must be a ragged.Lengths or a dense int64 device array [B], got %s (a host sequence is "
                            "refused: upload it once with device_array.lengths)" % (what, type(lens).__name__))
        self.lens = lens
        self.dev = _ragged_state(lens, what, "lens")
        self.plan = _vl.plan_varlen(q.shape, k.shape, v.shape, self.dev.shape, causal, scale, layout, grouped=form.fold,
                                    native=_lib.get().has_varlen, route=route or VARLEN_ROUTE)
        if isinstance(lens, _rg.Lengths):
            _vl.check_lens(lens.host, self.plan.T, what)

    def native(self, entry, *args):
        """ONE call of a tnn_varlen_* entry point: the arguments of its tnn_attn_* counterpart, then lens and the group."""
        getattr(_lib.get(), entry)(*(args + (self.dev._ptr, self.plan.group)))

    def masks(self, dt):
        """(key mask [B H, T, T], row mask [B H, T, 1]) of the composed route, from the host values of the lengths."""
        what = self.plan.grouped and "gqa_attention" or "attention"
        if _lib.capturing:
            raise RuntimeError("%s (composed route): the masks of lens= are built on the host and uploaded, which a graph "
                               "capture cannot do; the native route reads the lengths on the device" % what)
        host = _vl.check_lens(_ragged_mirror(self.lens, what), self.plan.T, what)
        plan = self.plan
        return (asarray(_vl.key_mask(host, plan.T, plan.H, dt), dtype=dt), asarray(_vl.row_mask(host, plan.T, plan.H, dt), dtype=dt))


def _attn_call_plan(form, q, k, v, causal, scale, layout, route, lens):
    """(plan, varlen state or None) of one call."""
    if lens is None:
        return form.plan(q, k, v, causal, scale, layout, route), None
    vl = _Varlen(form, q, k, v, lens, causal, scale, layout, route)
    return vl.plan, vl


def _zeroed(x3, rows):
    """x3 with its dead rows set to +0 (x * 0 may be -0; -0 + 0 is +0)."""
    return x3 * rows + 0.0


def _attn_fwd(form, q, k, v, causal, scale, layout, route, lens=None):
    """attention / gqa_attention.  Native: ONE call of the form's forward entry point (with lens=: of tnn_varlen_fwd).
    Composed: k and v repeated over the plan's group (1 for the plain form: nothing is repeated), two batched products,
    max-subtract, exp, sum, divide; with lens= the key mask joins the scores and the row mask zeroes the dead rows."""
    dt, (q, k, v) = _operands(q, k, v)
    plan, vl = _attn_call_plan(form, q, k, v, causal, scale, layout, route, lens)
    if plan.empty():
        return zeros(plan.out_shape, dt), zeros(plan.lse_shape, dt)
    if plan.route == "native":
        out = DeviceArray._new(plan.out_shape, dt)
        lse = DeviceArray._new(plan.lse_shape, dt)
        args = (q._ptr, k._ptr, v._ptr, out._ptr, lse._ptr) + tuple(plan.geometry()) + (
            _i64arr(plan.strides("q", "k", "v", "o")), plan.scale, int(plan.causal), out._code())
        if vl is None:
            getattr(_lib.get(), form.fwd)(*args)
        else:
            vl.native("varlen_fwd", *args)
        return out, lse
    k, v = _gqa_expand(k, plan.group), _gqa_expand(v, plan.group)
    s = _attn_scores(q, k, plan)
    if vl is not None:
        keys, rows = vl.masks(s.dtype)
        s = s + keys
    m = s.max(axis=-1, keepdims=True)
    e = exp(s - m)
    l = e.sum(axis=-1, keepdims=True)
    o3 = matmul(e / l, _attn3(v, plan, plan.Tk, plan.Dv))
    lse = m + log(l)
    if vl is not None:
        o3, lse = _zeroed(o3, rows), _zeroed(lse, rows)
    return _attn_from3(o3, plan, plan.Tq, plan.Dv), lse.reshape(plan.lse_shape)


def _attn_bwd_q(form, q, k, v, o, do, lse, causal, scale, layout, route, need_dq, dq_out, lens=None):
    """attention_bwd_q / gqa_attention_bwd_q.  Native: ONE call of the form's backward-q entry point; dq_out is used when it
    has exactly q's shape.  Composed: as _attn_fwd, on the repeated k and v."""
    dt, (q, k, v, o, do, lse) = _operands(q, k, v, o, do, lse)
    plan, vl = _attn_call_plan(form, q, k, v, causal, scale, layout, route, lens)
    if tuple(o.shape) != plan.out_shape or tuple(lse.shape) != plan.lse_shape:
        raise ValueError("%s_bwd_q: do / o %s and lse %s do not match the output %s and row statistics %s of this attention"
                         % (form.what, tuple(o.shape), tuple(lse.shape), plan.out_shape, plan.lse_shape))
    if do.shape != plan.out_shape:
        do = do._broadcast_to(plan.out_shape)
    if plan.empty():
        return (zeros(q.shape, dt) if need_dq else None), zeros(plan.lse_shape, dt)
    if plan.route == "native":
        dq = _dest(need_dq, dq_out, q.shape, dt, exact=True)
        delta = DeviceArray._new(plan.lse_shape, dt)
        args = (q._ptr, k._ptr, v._ptr, o._ptr, do._ptr, lse._ptr, _ptr_of(dq), delta._ptr) + tuple(plan.geometry()) + (
            _i64arr(plan.strides("q", "k", "v", "o", "o", "q")), plan.scale, int(plan.causal), delta._code())
        if vl is None:
            getattr(_lib.get(), form.bwd_q)(*args)
        else:
            vl.native("varlen_bwd_q", *args)
        return dq, delta
    k, v = _gqa_expand(k, plan.group), _gqa_expand(v, plan.group)
    do3 = _attn3(do, plan, plan.Tq, plan.Dv)
    delta3 = (do3 * _attn3(o, plan, plan.Tq, plan.Dv)).sum(axis=-1, keepdims=True)
    if vl is not None:
        keys, rows = vl.masks(delta3.dtype)
        delta3 = _zeroed(delta3, rows)
    dq = None
    if need_dq:
        s = _attn_scores(q, k, plan)
        if vl is not None:
            s = s + keys
        p = exp(s - lse.reshape(plan.B * plan.H, plan.Tq, 1))
        ds = p * (matmul(do3, _attn3(v, plan, plan.Tk, plan.Dv), swap_b=True) - delta3)
        dq3 = matmul(ds, _attn3(k, plan, plan.Tk, plan.D)) * plan.scale
        if vl is not None:
            dq3 = _zeroed(dq3, rows)
        dq = _attn_from3(dq3, plan, plan.Tq, plan.D)
    return dq, delta3.reshape(plan.lse_shape)


def _attn_bwd_kv(form, q, k, v, do, lse, delta, causal, scale, layout, route, need_dk, need_dv, dk_out, dv_out, lens=None):
    """attention_bwd_kv / gqa_attention_bwd_kv.  Native: ONE call of the form's backward-kv entry point; dk_out / dv_out are
    used when they have exactly k's / v's shape.  Composed: as _attn_fwd, on the repeated k and v; the grouped form then sums
    dk and dv over the group axis (also for a group of one)."""
    dt, (q, k, v, do, lse, delta) = _operands(q, k, v, do, lse, delta)
    plan, vl = _attn_call_plan(form, q, k, v, causal, scale, layout, route, lens)
    if tuple(lse.shape) != plan.lse_shape or tuple(delta.shape) != plan.lse_shape:
        raise ValueError("%s_bwd_kv: lse %s / delta %s do not match the row statistics %s of this attention"
                         % (form.what, tuple(lse.shape), tuple(delta.shape), plan.lse_shape))
    if do.shape != plan.out_shape:
        do = do._broadcast_to(plan.out_shape)
    if not need_dk and not need_dv:
        return None, None
    if plan.empty():
        return (zeros(k.shape, dt) if need_dk else None), (zeros(v.shape, dt) if need_dv else None)
    if plan.route == "native":
        dk, dv = _dest(need_dk, dk_out, k.shape, dt, exact=True), _dest(need_dv, dv_out, v.shape, dt, exact=True)
        args = (q._ptr, k._ptr, v._ptr, do._ptr, lse._ptr, delta._ptr, _ptr_of(dk), _ptr_of(dv)) + tuple(plan.geometry()) + (
            _i64arr(plan.strides("q", "k", "v", "o", "k", "v")), plan.scale, int(plan.causal), lse._code())
        if vl is None:
            getattr(_lib.get(), form.bwd_kv)(*args)
        else:
            vl.native("varlen_bwd_kv", *args)
        return dk, dv
    k, v = _gqa_expand(k, plan.group), _gqa_expand(v, plan.group)
    rows = plan.B * plan.H
    do3 = _attn3(do, plan, plan.Tq, plan.Dv)
    s = _attn_scores(q, k, plan)
    if vl is not None:
        keys, live = vl.masks(s.dtype)
        s = s + keys
    p = exp(s - lse.reshape(rows, plan.Tq, 1))
    if vl is not None:
        p = p * live                        # dead rows contribute to no key; dead keys of live rows have p = exp(-inf) = 0
    dk = dv = None
    if need_dv:
        dv3 = matmul(p, do3, swap_a=True)
        dv = _attn_from3(dv3 if vl is None else _zeroed(dv3, live), plan, plan.Tk, plan.Dv)
    if need_dk:
        ds = p * (matmul(do3, _attn3(v, plan, plan.Tk, plan.Dv), swap_b=True) - delta.reshape(rows, plan.Tq, 1))
        dk3 = matmul(ds, _attn3(q, plan, plan.Tq, plan.D), swap_a=True) * plan.scale
        dk = _attn_from3(dk3 if vl is None else _zeroed(dk3, live), plan, plan.Tk, plan.D)
    if form.fold:
        fold = lambda g, w: g.reshape(plan.B, plan.Tk, plan.Hkv, plan.group, w).sum(axis=3)
        dk, dv = (None if dk is None else fold(dk, plan.D)), (None if dv is None else fold(dv, plan.Dv))
    return dk, dv


def attention(q, k, v, causal=False, scale=None, layout="bhtd", route=None, lens=None):
    """(o, lse): o = softmax(scale q k^T) v over the key axis and the per-row log-sum-exp of the scaled scores (what the
    backward recomputes the probabilities from).  Layouts, the causal rule and the routes: attention.py.  Native: ONE
    tnn_attn_fwd launch, the scores never reach memory; composed: two batched products, max-subtract, exp, sum, divide.
    lens= (a ragged.Lengths or a dense int64 device array [B]; Tq == Tk, layout "bthd" or three-axis "bhtd"): sequence b of a
    right-padded batch has lens[b] live tokens — live rows attend over live keys only, dead rows get o = +0 and lse = 0
    (varlen.py: the rule, the routes).  Native: ONE tnn_varlen_fwd launch that reads the lengths on the device."""
    return _attn_fwd(_PLAIN, q, k, v, causal, scale, layout, route, lens)


def attention_bwd_q(q, k, v, o, do, lse, causal=False, scale=None, layout="bhtd", route=None, need_dq=True, dq_out=None,
                    lens=None):
    """(dq, delta) for the gradient `do` of attention's output: delta[i] = sum_c do[i, c] o[i, c] (what attention_bwd_kv
    reads) and dq = scale dS k with dS = p (dP - delta), dP = do v^T, p recomputed from lse.  need_dq=False: dq is None and
    only delta is produced (native: the key loop is skipped).  dq_out: a dense array the result is written into.  lens=: as
    attention; dead rows get delta = 0 and dq = +0."""
    return _attn_bwd_q(_PLAIN, q, k, v, o, do, lse, causal, scale, layout, route, need_dq, dq_out, lens)


def attention_bwd_kv(q, k, v, do, lse, delta, causal=False, scale=None, layout="bhtd", route=None, need_dk=True,
                     need_dv=True, dk_out=None, dv_out=None, lens=None):
    """(dk, dv): dv = p^T do and dk = scale dS^T q from ONE launch, with the delta attention_bwd_q produced (on the native
    route the launch must follow that call).  need_dk / need_dv = False: that product is skipped and None returned.  A key
    that no query sees (causal, Tk > Tq) gets exact zeros.  dk_out / dv_out: dense arrays the results are written into.
    lens=: as attention; dead keys get dk = dv = +0."""
    return _attn_bwd_kv(_PLAIN, q, k, v, do, lse, delta, causal, scale, layout, route, need_dk, need_dv, dk_out, dv_out, lens)


# ---------------------------------------------------------------------- kernels: layer norm, RMS norm, GELU (csrc/tnn_norm.hip)
NORM_ROUTE = None     # tests / probes: "native" or "composed" overrides the planner's choice (norm.py)
_GELU_C = math.sqrt(2.0 / math.pi)
_GELU_A = 0.044715


def _norm_plan(x, gamma, beta, kind, eps, route):
    return _nm.plan_norm(x.shape, None if gamma is None else gamma.shape, None if beta is None else beta.shape, kind, eps,
                         native=_lib.get().has_norm, route=route or NORM_ROUTE)


def _ptr_of(a):
    return None if a is None else a._ptr


def _norm_fwd(x, gamma, beta, kind, eps, route):
    dt, (x, gamma, beta) = _operands(x, gamma, beta)
    plan = _norm_plan(x, gamma, beta, kind, eps, route)
    layer = kind == "layer"
    if plan.empty():
        return zeros(plan.x_shape, dt), (zeros(plan.stats_shape, dt) if layer else None), zeros(plan.stats_shape, dt)
    if plan.route == "native":
        y = DeviceArray._new(plan.x_shape, dt)
        mean = DeviceArray._new(plan.stats_shape, dt) if layer else None
        rstd = DeviceArray._new(plan.stats_shape, dt)
        _lib.get().norm_fwd(x._ptr, _ptr_of(gamma), _ptr_of(beta), y._ptr, _ptr_of(mean), rstd._ptr, plan.M, plan.N,
                            plan.eps, _nm.KIND_CODE[kind], y._code())
        return y, mean, rstd
    d = x.reshape(plan.M, plan.N)
    mean = None
    if layer:
        mean = d.sum(axis=1, keepdims=True) / float(plan.N)
        d = d - mean
    rstd = 1.0 / sqrt((d * d).sum(axis=1, keepdims=True) / float(plan.N) + plan.eps)
    y = d * rstd
    if gamma is not None:
        y = y * gamma.reshape(1, plan.N)
    if beta is not None:
        y = y + beta.reshape(1, plan.N)
    return (y.reshape(plan.x_shape), None if mean is None else mean.reshape(plan.stats_shape),
            rstd.reshape(plan.stats_shape))


def layer_norm(x, gamma=None, beta=None, eps=1e-5, route=None):
    """(y, mean, rstd): y = (x - mean) * rstd * gamma + beta over the LAST axis of x, with the biased variance (the mean of
    the squared deviations from the mean, never E[x^2] - mean^2) and rstd = 1 / sqrt(var + eps); mean and rstd have shape
    x.shape[:-1] and are what norm_bwd reads.  gamma / beta: [N] or [1, N] or None (1 and 0).  Native: ONE tnn_norm_fwd launch
    that reads x once and writes y once; composed (norm.py: the CPU test twin, rows wider than BLOCK_MAX_N,
    route="composed"): sums, products and a square root on the generic operations."""
    return _norm_fwd(x, gamma, beta, "layer", eps, route)


def rms_norm(x, gamma=None, eps=1e-5, route=None):
    """(y, rstd): y = x * rstd * gamma with rstd = 1 / sqrt(mean(x^2) + eps) over the LAST axis of x.  Routes: layer_norm."""
    y, _, rstd = _norm_fwd(x, gamma, None, "rms", eps, route)
    return y, rstd


def norm_bwd(x, dy, gamma, mean, rstd, kind="layer", route=None, need_dx=True, need_dgamma=True, need_dbeta=True,
             dx_out=None, dgamma_out=None, dbeta_out=None):
    """(dx, dgamma, dbeta) of layer_norm / rms_norm for the gradient `dy` of y, from the saved row statistics.  With
    g = dy * gamma and xh = (x - mean) * rstd:  dx = rstd * (g - mean_N(g) - xh * mean_N(g xh)) (RMS norm: xh = x * rstd and
    no mean_N(g) term), dgamma = sum over the rows of dy * xh, dbeta = the sum of dy.  need_* = False: that gradient is not
    computed and None is returned (RMS norm has no dbeta at all).  dgamma / dbeta take gamma's shape ([N] without one).
    Native: ONE tnn_norm_bwd call — one pass over x and dy; the parameter gradients are reduced in a fixed order, so
    repeated calls give identical bits.  *_out: dense arrays the results are written into."""
    layer = kind == "layer"
    need_dbeta = need_dbeta and layer
    dt, (x, dy, gamma, mean, rstd) = _operands(x, dy, gamma, mean if layer else None, rstd)
    plan = _norm_plan(x, gamma, None, kind, 0.0, route)
    if tuple(rstd.shape) != plan.stats_shape or (layer and (mean is None or tuple(mean.shape) != plan.stats_shape)):
        raise ValueError("norm_bwd: the row statistics must have shape %s, got mean %s and rstd %s"
                         % (plan.stats_shape, None if mean is None else tuple(mean.shape), tuple(rstd.shape)))
    if dy.shape != plan.x_shape:
        dy = dy._broadcast_to(plan.x_shape)
    if not (need_dx or need_dgamma or need_dbeta):
        return None, None, None
    p_shape = (plan.N,) if gamma is None else tuple(gamma.shape)
    if plan.empty():
        return ((zeros(plan.x_shape, dt) if need_dx else None), (zeros(p_shape, dt) if need_dgamma else None),
                (zeros(p_shape, dt) if need_dbeta else None))
    if plan.route == "native":
        dx, dgamma, dbeta = _dest(need_dx, dx_out, plan.x_shape, dt), _dest(need_dgamma, dgamma_out, p_shape, dt), \
            _dest(need_dbeta, dbeta_out, p_shape, dt)
        nbytes = plan.workspace_bytes(dt.itemsize, need_dgamma, need_dbeta)
        ws = DeviceArray._new((nbytes // dt.itemsize,), dt) if nbytes else None
        _lib.get().norm_bwd(x._ptr, dy._ptr, _ptr_of(gamma), _ptr_of(mean), rstd._ptr, _ptr_of(dx), _ptr_of(dgamma),
                            _ptr_of(dbeta), _ptr_of(ws), nbytes, plan.M, plan.N, _nm.KIND_CODE[kind], x._code())
        return dx, dgamma, dbeta
    x2, dy2, r = x.reshape(plan.M, plan.N), dy.reshape(plan.M, plan.N), rstd.reshape(plan.M, 1)
    xh = ((x2 - mean.reshape(plan.M, 1)) if layer else x2) * r
    dx = dgamma = dbeta = None
    if need_dx:
        g = dy2 if gamma is None else dy2 * gamma.reshape(1, plan.N)
        inner = g - xh * ((g * xh).sum(axis=1, keepdims=True) / float(plan.N))
        if layer:
            inner = inner - g.sum(axis=1, keepdims=True) / float(plan.N)
        dx = (r * inner).reshape(plan.x_shape)
    if need_dgamma:
        dgamma = (dy2 * xh).sum(axis=0).reshape(p_shape)
    if need_dbeta:
        dbeta = dy2.sum(axis=0).reshape(p_shape)
    return dx, dgamma, dbeta


def _gelu_route(x, approximate, route):
    return _nm.gelu_route(approximate, native=_lib.get().has_norm, route=route or NORM_ROUTE)


def _gelu_inner(x):
    """tanh(u) of the tanh form, u = sqrt(2 / pi) (x + 0.044715 x^3)."""
    return tanh((x + (x * x * x) * _GELU_A) * _GELU_C)


def gelu(x, approximate="none", route=None):
    """GELU, elementwise.  approximate="none": 0.5 x (1 + erf(x / sqrt(2))); "tanh": 0.5 x (1 + tanh(sqrt(2 / pi)
    (x + 0.044715 x^3))).  Native: ONE tnn_gelu_fwd launch.  The composed route (CPU test twin, route="composed") exists for
    the tanh form only — there is no erf among the generic elementwise operations — and the exact form raises there."""
    dt, (x,) = _operands(x)
    if _gelu_route(x, approximate, route) == "native":
        y = DeviceArray._new(x.shape, dt)
        _lib.get().gelu_fwd(x._ptr, y._ptr, x.size, _nm.GELU_CODE[approximate], y._code())
        return y
    return (x * 0.5) * (_gelu_inner(x) + 1.0)


def gelu_bwd(x, dy, approximate="none", route=None, dx_out=None):
    """dx = dy * gelu'(x), recomputed from x (ONE tnn_gelu_bwd launch on the native route).  dx_out: a dense array the result
    is written into."""
    dt, (x, dy) = _operands(x, dy)
    if dy.shape != x.shape:
        dy = dy._broadcast_to(x.shape)
    if _gelu_route(x, approximate, route) == "native":
        dx = _grad_dest(dx_out, x.shape, dt)
        if dx is None:
            dx = DeviceArray._new(x.shape, dt)
        _lib.get().gelu_bwd(x._ptr, dy._ptr, dx._ptr, x.size, _nm.GELU_CODE[approximate], dx._code())
        return dx
    t = _gelu_inner(x)
    slope = (t + 1.0) * 0.5 + (x * 0.5) * (1.0 - t * t) * ((x * x) * (3.0 * _GELU_A) + 1.0) * _GELU_C
    return dy * slope


# ---------------------------------------------------------------------- kernels: random generator, dropout (csrc/tnn_dropout.hip)
DROPOUT_ROUTE = None  # tests / probes: "native" or "composed" overrides the planner's choice (dropout.py)


class DropoutMask(object):
    """What dropout_bwd needs of ONE dropout call.  Native: the 16-byte ticket of the forward launch (the mask is regenerated
    from it, never stored).  Composed: the uploaded boolean keep mask."""
    __slots__ = ("plan", "dtype", "ticket", "keep")

    def __init__(self, plan, dtype, ticket=None, keep=None):
        self.plan, self.dtype, self.ticket, self.keep = plan, dtype, ticket, keep

    def scale(self):
        """s: the plan's scale rounded ONCE to the operand dtype, as a Python float (exact)."""
        return float(self.dtype.type(self.plan.scale))


def _dropout_dest(out, shape, dt, what):
    if out is None:
        return DeviceArray._new(shape, dt)
    dest = _grad_dest(out, shape, dt)
    if dest is None:
        raise ValueError("%s: `out` must be a dense %s device array of %d elements" % (what, dt.name, _prod(shape)))
    return dest


def dropout(x, p, residual=None, generator=None, route=None, first=0, out=None):
    """(y, mask): y = keep ? x * s : +0 with s = 1 / (1 - p) rounded once to the operand dtype, plus `residual` (same shape)
    when there is one — product and sum rounded separately.  An element is kept iff the 24-bit draw of its stream index
    first + j (row-major j) is >= round(p 2^24) (dropout.py states the generator); the call consumes ONE value of the
    generator's `calls` (rng.Generator; None: rng.default_generator).  `mask` is what dropout_bwd takes.

    p == 0: nothing is drawn and nothing new is launched — (x, None), or (x + residual, None) through the existing add.
    Native: a one-thread ticket launch and ONE tnn_dropout_fwd data launch; capturable.  Composed (dropout.py: the CPU test
    twin, route="composed"): the generator's state is read (host integers, or a read-back), the keep mask is drawn on the host
    with the planner's generator and uploaded, the existing scalar multiply, masked select (mul_mask — a select, so a dropped
    element is +0 whatever x holds) and add apply it, and the state is advanced — so it raises inside an open graph capture.
    Both routes give identical bits and leave the generator in the same state.  out: a dense array the result is written
    into; it may be x or the residual."""
    from . import rng as _rng
    gen = _rng.default_generator if generator is None else generator
    dt, (x, residual) = _operands(x, residual)
    plan = _dp.plan_dropout(x.shape, p, dt, first=first, native=_lib.get().has_dropout, route=route or DROPOUT_ROUTE)
    if residual is not None and residual.shape != x.shape:
        raise ValueError("dropout: the residual must have x's shape %s, got %s" % (x.shape, residual.shape))
    if plan.threshold == 0 and plan.p == 0.0:
        if out is not None:
            raise ValueError("dropout: p == 0 writes nothing — `out` is not supported")
        return (x if residual is None else residual + x), None
    if plan.route == "native":
        state = gen.device_state()
        ticket = DeviceArray._new((2,), np.int64)
        y = _dropout_dest(out, x.shape, dt, "dropout")
        _lib.get().dropout_fwd(state._ptr, ticket._ptr, x._ptr, _ptr_of(residual), y._ptr, plan.first, plan.n, plan.threshold,
                               plan.scale, y._code())
        return y, DropoutMask(plan, dt, ticket=ticket)
    if _lib.capturing:
        raise RuntimeError("dropout: the composed route draws its mask on the host and cannot be captured into a graph")
    seed, calls = gen.state()
    keep = asarray(_dp.keep_mask(seed, calls, plan.first, plan.n, plan.threshold).reshape(x.shape))
    gen.advance(seed, calls)
    mask = DropoutMask(plan, dt, keep=keep)
    y = mul_mask(x * mask.scale(), keep)
    if residual is not None:
        y = residual + y
    if out is not None:
        dest = _dropout_dest(out, x.shape, dt, "dropout")
        dest.reshape(x.shape)[...] = y
        y = dest
    return y, mask


def dropout_bwd(dy, mask, dx_out=None):
    """dx = keep ? dy * s : +0 for the `mask` a dropout call returned (None — p was 0 — gives dy back).  Native: ONE
    tnn_dropout_bwd launch that regenerates the forward's mask from its ticket, whatever the generator has drawn since.  The
    residual's gradient is dy itself.  dx_out: a dense array the result is written into; it may be dy."""
    if mask is None:
        return dy
    dt, shape = mask.dtype, mask.plan.shape
    dy = asarray(dy)._as_float(dt)
    if dy.shape != shape:
        dy = dy._broadcast_to(shape)
    dy = dy._contig()
    if mask.ticket is not None:
        dx = _dest(True, dx_out, shape, dt)
        plan = mask.plan
        _lib.get().dropout_bwd(mask.ticket._ptr, dy._ptr, dx._ptr, plan.first, plan.n, plan.threshold, plan.scale, dx._code())
        return dx
    return mul_mask(dy * mask.scale(), mask.keep)


# ---------------------------------------------------------------------- kernels: embedding, per-row cross-entropy (csrc/tnn_token.hip)
TOKEN_ROUTE = None    # tests / probes: "native" or "composed" overrides the planner's choice (tokens.py)


def _token_ids(ids, limit, what, also=None):
    """(dense int64 device array, host copy or None) of ids / targets.  Host values (numpy, lists) are range-checked here —
    outside [0, limit) and not `also` raises IndexError; device-resident ones are NOT read back (the kernels skip them)."""
    if isinstance(ids, DeviceArray):
        if ids._hv is not None or ids.dtype.kind not in "iu":
            raise TypeError("%s: integer ids are needed, got a device array of dtype %s" % (what, ids.dtype))
        return ids.astype(np.int64)._contig(), None
    host = np.asarray(ids)
    if host.dtype.kind not in "iu":
        raise TypeError("%s: integer ids are needed, got dtype %s" % (what, host.dtype))
    host = np.ascontiguousarray(host, dtype=np.int64)
    bad = (host < 0) | (host >= limit)
    if also is not None:
        bad &= host != also
    if bad.any():
        raise IndexError("%s: index %d is out of bounds for %d entries" % (what, int(host[bad].flat[0]), limit))
    return asarray(host), host


def embedding(table, ids, pos=None, route=None):
    """out[..., :] = table[ids[...], :] (+ pos[t, :], t the index along the LAST axis of ids; pos may hold more rows than
    that axis is long).  table [V, E]; ids: integers of any shape, numpy / list (range-checked on the host: IndexError) or a
    device int64 array (not read back; an id outside [0, V) gives a zero token row).  Native: ONE tnn_embed_fwd launch;
    composed (tokens.py: the CPU test twin, route="composed"): a row gather and a broadcast addition."""
    dt, (table, pos) = _operands(table, pos)
    if table.ndim != 2:
        raise ValueError("embedding: the table must be [V, E], got shape %s" % (tuple(table.shape),))
    idd, _ = _token_ids(ids, table.shape[0], "embedding")
    plan = _tk.plan_embedding(table.shape, idd.shape, None if pos is None else pos.shape, None,
                              native=_lib.get().has_token, route=route or TOKEN_ROUTE)
    if plan.empty():
        return zeros(plan.out_shape, dt)
    if plan.route == "native":
        out = DeviceArray._new(plan.out_shape, dt)
        _lib.get().embed_fwd(table._ptr, idd._ptr, _ptr_of(pos), out._ptr, plan.M, plan.V, plan.E, plan.T, out._code())
        return out
    out = table.take(idd.reshape(plan.M))
    if pos is not None:
        out = out.reshape(plan.M // plan.T, plan.T, plan.E) + pos[:plan.T]
    return out.reshape(plan.out_shape)


def embedding_bwd(dy, ids, table_shape, pos_shape=None, padding_idx=None, need_dtable=True, need_dpos=True, dtable_out=None,
                  dpos_out=None, route=None):
    """(dtable, dpos) of embedding for the gradient `dy` of its output.  dtable[v] = the SUM of dy over the positions that
    hold v — repeated ids accumulate — with EVERY row written (zeros for absent tokens and for padding_idx); dpos[t] = the sum
    of dy over the sequences (rows past the sequence length: zeros).  need_* = False: not computed, None is returned.
    Native: ONE tnn_embed_bwd call (a deterministic sort of the positions by token, then segmented sums: no floating-point
    atomics, identical bits on every call).  Composed: one-hot^T @ dy through matmul; the one-hot is built from a HOST copy of
    the ids, so the composed backward cannot be captured into a graph.  *_out: dense arrays the results are written into."""
    dt, (dy,) = _operands(dy)
    idd, host = _token_ids(ids, int(table_shape[0]), "embedding")
    need_dpos = need_dpos and pos_shape is not None
    plan = _tk.plan_embedding(table_shape, idd.shape, pos_shape, padding_idx, native=_lib.get().has_token,
                              route=route or TOKEN_ROUTE)
    if dy.shape != plan.out_shape:
        dy = dy._broadcast_to(plan.out_shape)._contig()
    if not (need_dtable or need_dpos):
        return None, None
    t_shape = (plan.V, plan.E)
    p_shape = None if pos_shape is None else tuple(int(s) for s in pos_shape)
    if plan.empty():
        return (zeros(t_shape, dt) if need_dtable else None), (zeros(p_shape, dt) if need_dpos else None)
    if plan.route == "native":
        dtable, dpos = _dest(need_dtable, dtable_out, t_shape, dt), _dest(need_dpos, dpos_out, p_shape, dt)
        if dpos is not None and p_shape[0] > plan.T:
            dpos.fill(0.0)                                       # the launch writes the first T rows
        nbytes = plan.workspace_bytes(dt.itemsize) if need_dtable else 0
        ws = DeviceArray._new((nbytes // dt.itemsize,), dt) if nbytes else None
        _lib.get().embed_bwd(dy._ptr, idd._ptr, _ptr_of(dtable), _ptr_of(dpos), _ptr_of(ws), nbytes, plan.M, plan.V, plan.E,
                             plan.T, plan.padding_idx, dy._code())
        return dtable, dpos
    dy2 = dy.reshape(plan.M, plan.E)
    dtable = dpos = None
    if need_dtable:
        if host is None:
            _need_eager("the composed embedding backward (its one-hot is built from a host copy of the ids)")
            host = np.asarray(idd)
        flat = host.reshape(plan.M)
        one_hot = (flat[:, None] == np.arange(plan.V)[None, :]) & (flat[:, None] != plan.padding_idx)
        dtable = matmul(asarray(one_hot.astype(dt), dtype=dt), dy2, swap_a=True)
    if need_dpos:
        dpos = dy2.reshape(plan.M // plan.T, plan.T, plan.E).sum(axis=0)
        if p_shape[0] > plan.T:
            full_rows = zeros(p_shape, dt)
            full_rows[:plan.T] = dpos
            dpos = full_rows
    return dtable, dpos


def _xent_plan(x, tg, ignore_index, reduction, route):
    return _tk.plan_cross_entropy(x.shape, tg.shape, ignore_index, reduction, native=_lib.get().has_token,
                                  route=route or TOKEN_ROUTE)


def _xent_valid(plan, tg, host):
    """Host view of the targets of the composed route: (flat targets, bool mask of the counted rows)."""
    if host is None:
        _need_eager("the composed cross-entropy with device-resident targets (they are read back)")
        host = np.asarray(tg)
    flat = host.reshape(plan.M)
    return flat, (flat != plan.ignore_index) & (flat >= 0) & (flat < plan.V)


def cross_entropy(logits, targets, ignore_index=None, reduction="mean", route=None):
    """(loss, losses, lse, count) of the PER-ROW softmax cross-entropy over the last axis of logits [..., V] with integer
    targets [...]: lse = log sum exp of the row, losses = lse - x[target]; a row whose target is ignore_index has loss 0 and is
    not counted; count = the counted rows (a device scalar in the operand dtype), loss = sum of losses ("sum") or sum / count
    ("mean"; 0 when nothing is counted).  targets: numpy / list (range-checked on the host: IndexError unless in [0, V) or
    ignore_index) or a device int64 array (not read back; out-of-range rows are not counted).  -inf logits contribute 0; a
    row of nothing but -inf is out of scope.  Native: ONE tnn_xent_fwd call that reads every logit once; composed: max, exp,
    sum, log and the gather x[arange, t] as a row gather of the flattened logits, which the CPU test twin has too
    (device-resident targets are read back there)."""
    dt, (x,) = _operands(logits)
    if x.ndim < 1:
        raise ValueError("cross_entropy: the logits need a last axis of classes, got a scalar")
    tg, host = _token_ids(targets, x.shape[-1], "cross_entropy", also=ignore_index)
    plan = _xent_plan(x, tg, ignore_index, reduction, route)
    if plan.route == "native":
        losses, lse = DeviceArray._new(plan.rows_shape, dt), DeviceArray._new(plan.rows_shape, dt)
        loss, count = DeviceArray._new((), dt), DeviceArray._new((), dt)
        _lib.get().xent_fwd(x._ptr, tg._ptr, losses._ptr, lse._ptr, loss._ptr, count._ptr, plan.M, plan.V, plan.ignore_index,
                            _tk.REDUCTION_CODE[reduction], x._code())
        return loss, losses, lse, count
    if plan.empty():
        return zeros((), dt), zeros(plan.rows_shape, dt), zeros(plan.rows_shape, dt), zeros((), dt)
    flat, valid = _xent_valid(plan, tg, host)
    x2 = x.reshape(plan.M, plan.V)
    mx = x2.max(axis=1, keepdims=True)
    lse = (log(exp(x2 - mx).sum(axis=1, keepdims=True)) + mx).reshape(plan.M)
    rows = np.nonzero(valid)[0]
    losses = zeros((plan.M,), dt)
    if rows.size:
        losses[rows] = lse.take(rows) - x.reshape(plan.M * plan.V).take(rows * plan.V + flat[rows])     # x[rows, t]
    loss = losses.sum()
    if reduction == "mean":
        loss = loss / float(max(rows.size, 1))
    return loss.reshape(()), losses.reshape(plan.rows_shape), lse.reshape(plan.rows_shape), full((), float(rows.size), dt)


def cross_entropy_bwd(logits, targets, lse, count, g=1.0, ignore_index=None, reduction="mean", route=None, dlogits_out=None):
    """dlogits = (softmax(x) - one_hot(target)) * g / count ("sum": without / count) from the saved per-row lse; rows that
    were not counted get zeros, and count == 0 gives all zeros.  g (the gradient of the loss) and count (cross_entropy's) are
    used as DEVICE scalars on the native route — nothing is read on the host, a training step stays capturable — which is
    ONE tnn_xent_bwd launch: the logits are read once, dlogits written once.  dlogits_out: a dense array to write into."""
    dt, (x, lse) = _operands(logits, lse)
    tg, host = _token_ids(targets, x.shape[-1], "cross_entropy", also=ignore_index)
    plan = _xent_plan(x, tg, ignore_index, reduction, route)
    if tuple(lse.shape) != plan.rows_shape:
        raise ValueError("cross_entropy_bwd: lse must have shape %s, got %s" % (plan.rows_shape, tuple(lse.shape)))
    g = asarray(g)
    if g.size != 1:
        raise ValueError("cross_entropy_bwd: the loss is a scalar, got a gradient of shape %s" % (tuple(g.shape),))
    if plan.empty():
        return zeros(plan.logits_shape, dt)
    if plan.route == "native":
        gd, cd = g.astype(dt)._contig(), asarray(count).astype(dt)._contig()
        dx = _dest(True, dlogits_out, plan.logits_shape, dt)
        _lib.get().xent_bwd(x._ptr, tg._ptr, lse._ptr, cd._ptr, gd._ptr, dx._ptr, plan.M, plan.V, plan.ignore_index,
                            _tk.REDUCTION_CODE[reduction], x._code())
        return dx
    flat, valid = _xent_valid(plan, tg, host)
    n = int(valid.sum())
    if n == 0:
        return zeros(plan.logits_shape, dt)
    x2 = x.reshape(plan.M, plan.V)
    one_hot = (flat[:, None] == np.arange(plan.V)[None, :]) & valid[:, None]
    p = exp(x2 - lse.reshape(plan.M, 1))
    rows = asarray(valid.astype(dt).reshape(plan.M, 1) * (1.0 / n if reduction == "mean" else 1.0), dtype=dt)
    g = g if g._hv is not None else g.astype(dt).reshape(1, 1)
    return ((p - asarray(one_hot.astype(dt), dtype=dt)) * rows * g).reshape(plan.logits_shape)


# ---------------------------------------------------------------------- kernels: decode attention, sampling (csrc/tnn_decode.hip)
DECODE_ROUTE = None   # tests / probes: "native" or "composed" overrides the planner's choice (decoding.py)


def _decode_cache(a, dt, what):
    """A cache is written IN PLACE: it must already be a dense device array of the operand dtype (a copy would lose the row)."""
    if not isinstance(a, DeviceArray) or a._hv is not None or a._t or a.dtype != dt:
        raise TypeError("attention_decode: %s must be a dense device array of dtype %s (it is written in place)" % (what, dt))
    return a


def _decode_operands(what, q, k_cache, v_cache, k_new, v_new, lens=None):
    """(dt, q, k_cache, v_cache, k_new, v_new, lens) of a decode call — attention_decode, attention_decode_ragged, gqa_decode:
    the dtype is the caches', which are taken as they are; q and the step's row (when there is one) are cast and made dense;
    lens (when given) must be a dense int64 device array."""
    cands = [a.dtype for a in (k_cache, v_cache) if isinstance(a, DeviceArray) and a.dtype.kind == "f"]
    dt = cands[0] if cands else _default_float
    k_cache, v_cache = _decode_cache(k_cache, dt, "k_cache"), _decode_cache(v_cache, dt, "v_cache")
    q = asarray(q)._as_float(dt)._contig()
    if k_new is not None:
        k_new, v_new = asarray(k_new)._as_float(dt)._contig(), asarray(v_new)._as_float(dt)._contig()
    return dt, q, k_cache, v_cache, k_new, v_new, (None if lens is None else _ragged_state(lens, what, "lens"))


def _decode_float_ok(dt):
    return dt in (np.dtype(np.float32), np.dtype(np.float64))


def _decode_native(entry, plan, dt, q, k_cache, v_cache, k_new, v_new, lens=None):
    """ONE call of `entry` (lib.decode_attn, lib.ragged_decode_attn, lib.gqa_decode_attn or lib.gqa_ragged_decode_attn — the
    ragged ones take the lengths' address after the workspace); the workspace of a split call comes from the buffer cache."""
    out = DeviceArray._new(plan.out_shape, dt)
    nbytes = plan.workspace_bytes(dt.itemsize)
    ws = DeviceArray._new((nbytes // dt.itemsize,), dt) if nbytes else None
    entry(q._ptr, _ptr_of(k_new), _ptr_of(v_new), k_cache._ptr, v_cache._ptr, out._ptr, _ptr_of(ws), nbytes,
          *(() if lens is None else (lens._ptr,)), *plan.geometry(), _i64arr(plan.strides()), plan.scale, plan.splits, out._code())
    return out


_DECODE_AXES = {"bthd": (1, 2), "bhtd": (2, 1)}       # layout -> the (time, head) axes of a cache


def _decode_append(plan, k_cache, v_cache, k_new, v_new):
    """The step's row by a slice assignment into cache row plan.length (nothing without a row)."""
    if k_new is not None:
        row = (slice(None),) * _DECODE_AXES[plan.layout][0] + (plan.length,)
        k_cache[row] = k_new
        v_cache[row] = v_new


def _decode_composed(plan, q, k_cache, v_cache, k_new, v_new):
    """The append, then attention() on its composed route over the live prefix with the heads of the caches repeated over the
    plan's group (1 for the ungrouped forms: nothing is repeated)."""
    _decode_append(plan, k_cache, v_cache, k_new, v_new)
    t_axis, h_axis = _DECODE_AXES[plan.layout]
    live = (slice(None),) * t_axis + (slice(None, plan.keys),)
    group = getattr(plan, "group", 1)
    q_shape = [plan.B, plan.H, plan.D]
    q_shape.insert(t_axis, 1)
    o, _ = attention(q.reshape(*q_shape), _gqa_expand(k_cache[live], group, h_axis), _gqa_expand(v_cache[live], group, h_axis),
                     False, plan.scale, plan.layout, "composed")
    return o.reshape(plan.out_shape)


def _decode_composed_ragged(what, step, plan, dt, lens, q, k_cache, v_cache, k_new, v_new):
    """The ragged composed route: a loop over the sequences that calls `step` (attention_decode or gqa_decode) on its composed
    route on batch slices with the host values of the lengths; it raises inside an open capture."""
    if _lib.capturing:
        raise RuntimeError("%s (composed route) loops over the sequences with host lengths, which a graph capture cannot do" % what)
    host = _ragged_mirror(lens, what)
    out = zeros(plan.out_shape, dt)
    for b in range(plan.B):
        if not 0 <= int(host[b]) < plan.Tmax:
            continue                                           # zeros, the caches untouched
        one = slice(b, b + 1)
        out[one] = step(q[one], k_cache[one], v_cache[one], int(host[b]), k_new[one], v_new[one], scale=plan.scale,
                        layout=plan.layout, route="composed")
    return out


def attention_decode(q, k_cache, v_cache, length, k_new=None, v_new=None, scale=None, layout="bthd", route=None, splits=None):
    """o [B, H, Dv] = softmax(scale q k^T) v for ONE query per (batch, head) over the live rows of a key / value cache
    (decoding.py: layouts, the key split, the routes).  q [B, H, D].  With k_new [B, H, D] and v_new [B, H, Dv] the step's own
    row is written into cache row `length` — the caches are modified in place — and the keys are [0, length]; without them
    the keys are [0, length).  `length` is a host integer.  Native: ONE tnn_decode_attn call (a second small launch inside
    it when the keys are split), nothing synchronises; composed: a slice assignment of the new row, then attention() on its
    composed route over the live prefix.  The workspace of a split call comes from the buffer cache."""
    if (k_new is None) != (v_new is None):
        raise ValueError("attention_decode: k_new and v_new come together or not at all")
    append = k_new is not None
    dt, q, k_cache, v_cache, k_new, v_new, _ = _decode_operands("attention_decode", q, k_cache, v_cache, k_new, v_new)
    lib = _lib.get()
    plan = _dc.plan_decode(q.shape, k_cache.shape, v_cache.shape, length, append, k_new.shape if append else None,
                           v_new.shape if append else None, scale, layout, splits, native=lib.has_decode,
                           float_ok=_decode_float_ok(dt), route=route or DECODE_ROUTE)
    if plan.empty():
        return zeros(plan.out_shape, dt)
    if plan.route == "native":
        return _decode_native(lib.decode_attn, plan, dt, q, k_cache, v_cache, k_new, v_new)
    if plan.route == "fwd":                                    # the route that existed before: tnn_attn_fwd with Tq = 1, in place
        _decode_append(plan, k_cache, v_cache, k_new, v_new)
        out, lse = DeviceArray._new(plan.out_shape, dt), DeviceArray._new((plan.B, plan.H, 1), dt)
        lib.attn_fwd(q._ptr, k_cache._ptr, v_cache._ptr, out._ptr, lse._ptr, plan.B, plan.H, 1, plan.keys, plan.D, plan.Dv,
                     _i64arr(plan.q_strides + plan.kcache_strides + plan.vcache_strides + plan.o_strides), plan.scale, 0,
                     out._code())
        return out
    return _decode_composed(plan, q, k_cache, v_cache, k_new, v_new)


def sample_rows(logits, u, temperature=1.0, top_k=None, route=None):
    """ids int64 [M] on the device: one token per row of logits [M, V] from one uniform number u[m] in [0, 1) (decoding.py and
    include/tnn_decode.h state the rule: greedy at temperature 0, else the inverse CDF of softmax(x / temperature) over the
    top_k largest).  Native: ONE tnn_sample_rows launch — nothing is read back, the ids can feed embedding() as they are.
    Composed: the logits (and u) are READ BACK and the rule runs in numpy; that is a host synchronisation and cannot be
    captured into a graph."""
    dt, (x,) = _operands(logits)
    lib = _lib.get()
    greedy = float(temperature) == 0.0
    ud = None
    if not greedy:
        if u is None:
            raise ValueError("sample_rows: u is needed unless temperature is 0")
        ud = asarray(u)._as_float(dt)._contig()
    plan = _dc.plan_sample(x.shape, None if ud is None else ud.shape, temperature, top_k, dt.itemsize, native=lib.has_decode,
                           route=route or DECODE_ROUTE)
    if plan.empty():
        return zeros((0,), np.int64)
    if plan.route == "native":
        out = DeviceArray._new((plan.M,), np.int64)
        lib.sample_rows(x._ptr, _ptr_of(ud), out._ptr, plan.M, plan.V, plan.temperature, plan.top_k, x._code())
        return out
    if _lib.capturing:
        raise RuntimeError("sample_rows (composed route) reads the logits back to the host, which a graph capture cannot do")
    return asarray(_dc.sample_host(np.asarray(x), None if ud is None else np.asarray(ud), plan.temperature, plan.top_k))


# ---------------------------------------------------------------------- kernels: the ragged decoding step (csrc/tnn_ragged.hip)
RAGGED_ROUTE = None   # tests / probes: "native" or "composed" overrides the planner's choice (ragged.py)


def lengths(host):
    """A ragged.Lengths from host integers [B]: the device int64 array and its host mirror."""
    host = np.ascontiguousarray(host, dtype=np.int64).reshape(-1)
    return _rg.Lengths(asarray(host), host)


def _ragged_state(a, what, name):
    """An integer state array is read (and mostly written) IN PLACE by a launch: a dense int64 device array."""
    if isinstance(a, _rg.Lengths):
        a = a.dev
    if not isinstance(a, DeviceArray) or a._hv is not None or a._t or a.dtype != np.dtype(np.int64):
        raise TypeError("%s: %s must be a dense int64 device array" % (what, name))
    return a


def _ragged_mirror(lens, what):
    """The host values of the lengths on the composed route: the mirror when there is one, else a read-back."""
    if isinstance(lens, _rg.Lengths):
        return lens.host
    if _lib.capturing:
        raise RuntimeError("%s (composed route) reads the lengths on the host, which a graph capture cannot do" % what)
    return np.asarray(lens)


def attention_decode_ragged(q, k_cache, v_cache, lens, k_new, v_new, scale=None, layout="bthd", route=None, splits=None):
    """attention_decode with the append for a RAGGED batch: sequence b writes k_new[b] / v_new[b] into cache row lens[b] and
    attends over keys [0, lens[b]].  lens: a ragged.Lengths (device int64 [B] + host mirror) or a dense int64 device array.
    Native: ONE tnn_ragged_decode_attn call that reads the lengths on the device — its arguments do not depend on them, so
    the call can be captured and replayed; a sequence whose length is outside [0, Tmax) gets zeros and its caches stay
    untouched.  Composed (ragged.py: the CPU test twin, route="composed"): a loop over the sequences that calls the composed
    attention_decode on batch slices with the host values of the lengths; it raises inside an open capture."""
    what = "attention_decode_ragged"
    if k_new is None or v_new is None:
        raise ValueError("%s: k_new and v_new are required (the step appends its row)" % what)
    dt, q, k_cache, v_cache, k_new, v_new, ld = _decode_operands(what, q, k_cache, v_cache, k_new, v_new, lens)
    lib = _lib.get()
    plan = _rg.plan_ragged_decode(q.shape, k_cache.shape, v_cache.shape, ld.shape, k_new.shape, v_new.shape, scale, layout,
                                  splits, native=lib.has_ragged, float_ok=_decode_float_ok(dt), route=route or RAGGED_ROUTE)
    if plan.empty():
        return zeros(plan.out_shape, dt)
    if plan.route == "native":
        return _decode_native(lib.ragged_decode_attn, plan, dt, q, k_cache, v_cache, k_new, v_new, ld)
    return _decode_composed_ragged(what, attention_decode, plan, dt, lens, q, k_cache, v_cache, k_new, v_new)


def embedding_at(table, ids, positions, pos=None, route=None):
    """out[..., :] = table[ids[...], :] + pos[positions[...], :]: every id sits at its OWN position.  table [V, E], pos
    [Tpos, E] or None (nothing is added); ids and positions: dense int64 device arrays of one shape (positions may be a
    ragged.Lengths), neither is read back — an id outside [0, V) gives a zero token row, a position outside [0, Tpos) a zero
    position row.  Native: ONE tnn_ragged_embed_fwd launch; composed: two row gathers and an addition (in-range indices only)."""
    what = "embedding_at"
    dt, (table, pos) = _operands(table, pos)
    if table.ndim != 2 or (pos is not None and (pos.ndim != 2 or pos.shape[1] != table.shape[1])):
        raise ValueError("%s: the table must be [V, E] and pos [Tpos, E], got shapes %s and %s"
                         % (what, tuple(table.shape), None if pos is None else tuple(pos.shape)))
    idd = _ragged_state(ids, what, "ids")._contig()
    shape = tuple(idd.shape)
    m, e = _prod(shape), int(table.shape[1])
    pd = None
    if pos is not None:
        pd = _ragged_state(positions, what, "positions")
        if _prod(pd.shape) != m:
            raise ValueError("%s: ids %s and positions %s must hold one position per id" % (what, shape, tuple(pd.shape)))
    lib = _lib.get()
    route = _rg.pick_route(lib.has_ragged and dt in (np.dtype(np.float32), np.dtype(np.float64)), route or RAGGED_ROUTE, what)
    if m == 0:
        return zeros(shape + (e,), dt)
    if route == "native":
        out = DeviceArray._new(shape + (e,), dt)
        lib.ragged_embed_fwd(table._ptr, idd._ptr, _ptr_of(pos), _ptr_of(pd), out._ptr, m, int(table.shape[0]), e,
                             0 if pos is None else int(pos.shape[0]), out._code())
        return out
    out = table.take(idd.reshape(m))
    if pos is not None:
        out = out + pos.take(pd.reshape(m))
    return out.reshape(shape + (e,))


def ragged_advance(picked, lens, start, done, out, cur, u_all=None, u_cur=None, eos=None, pad=0, route=None):
    """The bookkeeping of one token step of a ragged batch, IN PLACE (include/tnn_ragged.h states the rule; ragged.advance_host
    is its numpy form): every sequence's length grows by one, its id — `picked`, or `pad` once it has ended — goes to
    out[b, lens[b]] and to cur[b], the end-of-sequence flag done[b] is set on `eos` (None: there is none), and the next
    step's uniform numbers are copied from u_all [N, B] into u_cur [B].  All integer arrays: dense int64 device arrays
    (lens may be a ragged.Lengths, whose host mirror is advanced too — except while a graph capture records the launch, which
    does not run it).  Native: ONE tnn_ragged_advance launch; composed: the arrays are read back, advanced in numpy and
    uploaded, which a graph capture cannot do."""
    what = "ragged_advance"
    ld, sd, dd, od, cd, pk = (_ragged_state(a, what, n) for a, n in ((lens, "lens"), (start, "start"), (done, "done"),
                                                                      (out, "out"), (cur, "cur"), (picked, "picked")))
    if (u_all is None) != (u_cur is None):
        raise ValueError("%s: u_all and u_cur come together or not at all" % what)
    dt = np.dtype(np.float32)
    if u_all is not None:
        dt = u_all.dtype
        for a, n in ((u_all, "u_all"), (u_cur, "u_cur")):
            if not isinstance(a, DeviceArray) or a._hv is not None or a._t or a.dtype != dt or dt.kind != "f":
                raise TypeError("%s: %s must be a dense floating-point device array (u_all and u_cur of one dtype)" % (what, n))
    B, Tout, N = _rg.check_advance(pk.shape, ld.shape, sd.shape, dd.shape, od.shape, cd.shape,
                                   None if u_all is None else u_all.shape, None if u_cur is None else u_cur.shape)
    eos = -1 if eos is None else int(eos)
    lib = _lib.get()
    route = _rg.pick_route(lib.has_ragged and dt in (np.dtype(np.float32), np.dtype(np.float64)), route or RAGGED_ROUTE, what)
    if B == 0:
        return
    if route == "native":
        lib.ragged_advance(pk._ptr, ld._ptr, sd._ptr, dd._ptr, od._ptr, cd._ptr, _ptr_of(u_all), _ptr_of(u_cur), B, Tout, N, eos,
                           int(pad), _CODE[dt])
        if isinstance(lens, _rg.Lengths) and not _lib.capturing:
            lens.host += 1
        return
    if _lib.capturing:
        raise RuntimeError("%s (composed route) advances the state on the host, which a graph capture cannot do" % what)
    h_lens = np.array(_ragged_mirror(lens, what))
    h_done, h_out, h_cur = np.asarray(dd).copy(), np.asarray(od).copy(), np.asarray(cd).copy()
    h_u = None if u_all is None else np.asarray(u_cur).copy()
    _rg.advance_host(np.asarray(pk), h_lens, np.asarray(sd), h_done, h_out, h_cur, None if u_all is None else np.asarray(u_all),
                     h_u, eos, int(pad))
    for dev, host in ((ld, h_lens), (dd, h_done), (od, h_out), (cd, h_cur)):
        dev[...] = asarray(host)
    if u_all is not None:
        u_cur[...] = asarray(h_u)
    if isinstance(lens, _rg.Lengths):
        lens.host[:] = h_lens


# ---------------------------------------------------------------------- kernels: grouped-query attention (csrc/tnn_gqa.hip)
GQA_ROUTE = None      # tests / probes: "native" or "composed" overrides the planner's choice (gqa.py)


def _gqa_plan(q, k, v, causal, scale, route):
    return _gq.plan_gqa_attention(q.shape, k.shape, v.shape, causal, scale, native=_lib.get().has_gqa, route=route or GQA_ROUTE)


def _gqa_expand(x, group, axis=2):
    """k or v with every head repeated `group` times along the head axis: head h of the result is head h // group."""
    return x if group == 1 else _np_repeat(x, group, axis)


_GROUPED = _AttnForm(lambda q, k, v, causal, scale, layout, route: _gqa_plan(q, k, v, causal, scale, route),
                     "gqa_fwd", "gqa_bwd_q", "gqa_bwd_kv", "gqa_attention", True)


def gqa_attention(q, k, v, causal=False, scale=None, route=None, lens=None):
    """(o, lse) of grouped-query attention in layout "bthd": q [B, Tq, H, D], k [B, Tk, Hkv, D], v [B, Tk, Hkv, Dv] ->
    o [B, Tq, H, Dv], lse [B, H, Tq]; query head h reads key / value head h // (H / Hkv) (gqa.py: the checks, the routes).
    Native: ONE tnn_gqa_fwd launch, k and v are never expanded; composed: k and v repeated over the group, then attention()
    on its composed route.  lens=: per-sequence lengths of a right-padded batch, as attention (ONE tnn_varlen_fwd launch)."""
    return _attn_fwd(_GROUPED, q, k, v, causal, scale, "bthd", route, lens)


def gqa_attention_bwd_q(q, k, v, o, do, lse, causal=False, scale=None, route=None, need_dq=True, dq_out=None, lens=None):
    """(dq, delta) of gqa_attention, as attention_bwd_q: delta [B, H, Tq] is what gqa_attention_bwd_kv reads; need_dq=False:
    only delta.  Native: ONE tnn_gqa_bwd_q launch (lens=: tnn_varlen_bwd_q)."""
    return _attn_bwd_q(_GROUPED, q, k, v, o, do, lse, causal, scale, "bthd", route, need_dq, dq_out, lens)


def gqa_attention_bwd_kv(q, k, v, do, lse, delta, causal=False, scale=None, route=None, need_dk=True, need_dv=True,
                         dk_out=None, dv_out=None, lens=None):
    """(dk, dv) of gqa_attention with the shapes of k and v: the sums over every key / value head's group of query heads.
    Native: ONE tnn_gqa_bwd_kv launch (it must follow gqa_attention_bwd_q on the stream: it reads that call's delta) — one
    workgroup per (b, key / value head, key block) adds the group's heads in ascending order and writes once.  Composed:
    attention_bwd_kv on k and v repeated over the group, then a sum over the group axis.  lens=: tnn_varlen_bwd_kv."""
    return _attn_bwd_kv(_GROUPED, q, k, v, do, lse, delta, causal, scale, "bthd", route, need_dk, need_dv, dk_out, dv_out, lens)


def gqa_decode(q, k_cache, v_cache, length=None, k_new=None, v_new=None, lens=None, scale=None, layout="bthd", route=None,
               splits=None):
    """o [B, H, Dv] for ONE query per (batch, query head) over the live rows of caches that hold Hkv heads (gqa.py); query
    head h reads key / value head h // (H / Hkv).  q [B, H, D]; k_new [B, Hkv, D], v_new [B, Hkv, Dv].
        length=   a host integer shared by the batch, as attention_decode (with k_new / v_new the row is written into cache
                  row `length` IN PLACE and the keys are [0, length]; without, [0, length))
        lens=     a ragged.Lengths or a dense int64 device array [B], read on the device, as attention_decode_ragged (k_new
                  and v_new are required; a length outside [0, Tmax) gives zeros and leaves the caches untouched)
    Native: ONE tnn_gqa_decode_attn / tnn_gqa_ragged_decode_attn call: a workgroup serves all H / Hkv queries of a key / value
    head from one read of each K / V row; the ragged call's arguments are fixed by the shapes, so it can be captured.
    Composed: the append by a slice assignment, then the composed attention over the live prefix repeated over the group;
    with lens= a loop over the sequences on the host, which raises inside an open capture."""
    what = "gqa_decode"
    if (k_new is None) != (v_new is None):
        raise ValueError("%s: k_new and v_new come together or not at all" % what)
    if (length is None) == (lens is None):
        raise ValueError("%s: give length= (a host integer shared by the batch) or lens= (one per sequence), not both" % what)
    ragged = lens is not None
    append = k_new is not None
    if ragged and not append:
        raise ValueError("%s: with lens= k_new and v_new are required (the step appends its row)" % what)
    dt, q, k_cache, v_cache, k_new, v_new, ld = _decode_operands(what, q, k_cache, v_cache, k_new, v_new, lens)
    lib = _lib.get()
    plan = _gq.plan_gqa_decode(q.shape, k_cache.shape, v_cache.shape, length, append, k_new.shape if append else None,
                               v_new.shape if append else None, scale, layout, splits, ld.shape if ragged else None,
                               native=lib.has_gqa, float_ok=_decode_float_ok(dt), route=route or GQA_ROUTE)
    if plan.empty():
        return zeros(plan.out_shape, dt)
    if plan.route == "native":
        entry = lib.gqa_ragged_decode_attn if ragged else lib.gqa_decode_attn
        return _decode_native(entry, plan, dt, q, k_cache, v_cache, k_new, v_new, ld)
    if ragged:
        return _decode_composed_ragged(what, gqa_decode, plan, dt, lens, q, k_cache, v_cache, k_new, v_new)
    return _decode_composed(plan, q, k_cache, v_cache, k_new, v_new)


# ---------------------------------------------------------------------- kernels: cache-extending attention (csrc/tnn_extend.hip)
EXTEND_ROUTE = None   # tests / probes: "native" or "composed" overrides the planner's choice (extend.py)


def _extend_mask(t, keys, offset, dt):
    """[t, keys]: 0 where key j <= offset + i and -inf above that diagonal; kept with the causal masks, under a key that
    holds the offset."""
    key = ("extend", t, keys, offset, dt)
    m = _ATTN_MASKS.get(key)
    if m is None:
        if _lib.capturing:
            raise RuntimeError("attention_extend (composed route): the mask of a new (T, keys, offset, dtype) is uploaded from "
                               "the host, which a graph capture cannot do; run one step outside the capture first")
        host = np.zeros((t, keys), dtype=dt)
        host[np.triu_indices(t, offset + 1, keys)] = -np.inf
        if len(_ATTN_MASKS) >= _ATTN_MASKS_MAX:
            _ATTN_MASKS.clear()
        m = _ATTN_MASKS[key] = asarray(host, dtype=dt)
    return m


def _extend_composed(plan, q, k_cache, v_cache, k_new, v_new):
    """The new rows by a slice assignment, k and v repeated over the group, then the composed attention over rows
    [0, length + T) with the offset mask."""
    t_axis, h_axis = _DECODE_AXES[plan.layout]
    fresh = (slice(None),) * t_axis + (slice(plan.length, plan.keys),)
    k_cache[fresh] = k_new
    v_cache[fresh] = v_new
    live = (slice(None),) * t_axis + (slice(None, plan.keys),)
    _, (k, v) = _operands(_gqa_expand(k_cache[live], plan.group, h_axis), _gqa_expand(v_cache[live], plan.group, h_axis))
    s = matmul(_attn3(q, plan, plan.T, plan.D), _attn3(k, plan, plan.keys, plan.D), swap_b=True) * plan.scale
    s = s + _extend_mask(plan.T, plan.keys, plan.length, s.dtype)
    e = exp(s - s.max(axis=-1, keepdims=True))
    o3 = matmul(e / e.sum(axis=-1, keepdims=True), _attn3(v, plan, plan.keys, plan.Dv))
    return _attn_from3(o3, plan, plan.T, plan.Dv)


def attention_extend(q, k_cache, v_cache, length, k_new, v_new, scale=None, layout="bthd", route=None):
    """o = attention of T NEW rows per sequence over the `length` cached rows and over themselves, with the append
    (extend.py: the layouts, the routes).  "bthd": q [B, T, H, D], k_new [B, T, Hkv, D], v_new [B, T, Hkv, Dv], caches
    [B, Tmax, Hkv, D | Dv] -> o [B, T, H, Dv]; query row i sees the absolute keys j <= length + i (bottom-right causal), head h
    reads key / value head h // (H / Hkv).  The caches are modified IN PLACE: rows [length, length + T) become k_new / v_new
    bit for bit.  `length` is a host integer; 0 is a prefill straight into the cache.  Native: ONE tnn_extend_attn call,
    nothing synchronises; its rows do not depend on how they are cut into calls.  Composed: a slice assignment, then two
    batched products, the offset mask, max-subtract, exp, sum, divide."""
    what = "attention_extend"
    cands = [a.dtype for a in (k_cache, v_cache) if isinstance(a, DeviceArray) and a.dtype.kind == "f"]
    dt = cands[0] if cands else _default_float
    for a, name in ((k_cache, "k_cache"), (v_cache, "v_cache")):
        if not isinstance(a, DeviceArray) or a._hv is not None or a._t or a.dtype != dt:
            raise TypeError("%s: %s must be a dense device array of dtype %s (it is written in place)" % (what, name, dt))
    if k_new is None or v_new is None:
        raise ValueError("%s: k_new and v_new are required (the new rows are the call's own keys)" % what)
    q, k_new, v_new = (asarray(a)._as_float(dt)._contig() for a in (q, k_new, v_new))
    lib = _lib.get()
    plan = _ex.plan_extend(q.shape, k_cache.shape, v_cache.shape, length, k_new.shape, v_new.shape, scale, layout,
                           native=lib.has_extend, route=route or EXTEND_ROUTE, float_ok=_decode_float_ok(dt),
                           pointers=(k_new._ptr, v_new._ptr, k_cache._ptr, v_cache._ptr))
    if plan.empty():
        return zeros(plan.out_shape, dt)
    if plan.route == "native":
        out = DeviceArray._new(plan.out_shape, dt)
        lib.extend_attn(q._ptr, k_new._ptr, v_new._ptr, k_cache._ptr, v_cache._ptr, out._ptr, *plan.geometry(),
                        _i64arr(plan.strides()), plan.scale, out._code())
        return out
    return _extend_composed(plan, q, k_cache, v_cache, k_new, v_new)


# ---------------------------------------------------------------------- kernels: rotary position embedding (csrc/tnn_rope.hip)
ROPE_ROUTE = None    # tests / probes: "native" or "composed" overrides the planner's choice (rope.py)


def _rope_tables(rotary, R, dt):
    """The device tables of `rotary` for (R, dt): uploaded once, at first use, and kept at their addresses."""
    if _lib.capturing and (int(R), dt) not in rotary._device:
        raise RuntimeError("rope: the tables of a Rotary are uploaded at first use, which a graph capture cannot do; run one "
                           "step outside the capture first")
    return rotary.device_tables(R, dt, lambda host: asarray(host, dtype=dt))


def _rope_composed(plan, x, y, cos_t, sin_t, host_positions):
    """One tensor on the composed route: slice reads, products and slice assignments; both halves are computed before either
    is written, so y may be x."""
    half, R = plan.R // 2, plan.R
    lo, hi = (slice(0, half), slice(half, R)) if plan.pairing == "half" else (slice(0, R, 2), slice(1, R, 2))
    table_shape = (1, -1, 1, half) if plan.layout == "bthd" else (1, 1, -1, half)

    def rotate(src, dst, first, rows):
        c = cos_t[first:first + rows].reshape(*table_shape)
        s = sin_t[first:first + rows].reshape(*table_shape)
        if plan.inverse:
            s = -s
        x_lo, x_hi = src[..., lo], src[..., hi]
        y_lo, y_hi = x_lo * c - x_hi * s, x_hi * c + x_lo * s
        if dst is not src and R < plan.D:
            dst[..., R:] = src[..., R:]
        dst[..., lo] = y_lo
        dst[..., hi] = y_hi

    if host_positions is None:
        rotate(x, y, plan.offset, plan.T)
        return
    for b in range(plan.B):
        one = slice(b, b + 1)
        pos = int(host_positions[b])
        if 0 <= pos < plan.P:
            rotate(x[one], y[one] if y is not x else x[one], pos, 1)
        else:
            y[one] = zeros(y[one].shape, y.dtype)


def rope(xa, xb=None, rotary=None, offset=0, positions=None, layout="bthd", inverse=False, route=None, blocks=0, out=None):
    """The rotary position embedding of xa — and of xb in the same launch: ya, or (ya, yb).  xa [B, T, Ha, D] and xb
    [B, T, Hb, D] (layout "bthd") or [B, Ha, T, D] and [B, Hb, T, D] ("bhtd"); rotary: a rope.Rotary (tables, width, pairing).
    Row (b, t) sits at position offset + t, or — positions: a ragged.Lengths or a dense int64 device array [B], T == 1 — at
    positions[b], read on the device (a position outside [0, max_len) gives zeros).  inverse=True is the inverse rotation,
    which is also the vjp.  out: None (fresh arrays), "inplace" (the operands are overwritten and returned), or the output
    array(s); rope.plan_rope states every check.  blocks: the workgroup count of the native launch (0: the library's).
    Native: ONE tnn_rope_apply launch.  Composed (rope.py: the CPU test twin, route="composed"): slice reads, products and
    slice assignments; with positions= it reads their host values per sequence and raises inside an open capture."""
    what = "rope"
    if rotary is None:
        raise ValueError("%s: rotary= (a rope.Rotary) is required" % what)
    arrays = [xa] if xb is None else [xa, xb]
    cands = [a.dtype for a in arrays if isinstance(a, DeviceArray) and a.dtype.kind == "f"]
    dt = cands[0] if cands else _default_float
    inplace = isinstance(out, str)
    if inplace and out != "inplace":
        raise ValueError("%s: out must be None, \"inplace\" or the output array(s), got %r" % (what, out))
    xs = []
    for a in arrays:
        if inplace and (not isinstance(a, DeviceArray) or a._hv is not None or a._t or a.dtype != dt):
            raise TypeError("%s: in-place operation needs dense device arrays of one float dtype" % what)
        xs.append(asarray(a)._as_float(dt)._contig())
    if inplace:
        ys = list(xs)
    elif out is None:
        ys = [None] * len(xs)
    else:
        ys = list(out) if isinstance(out, (tuple, list)) else [out]
        if len(ys) != len(xs):
            raise ValueError("%s: %d output arrays for %d operands" % (what, len(ys), len(xs)))
        for x, y in zip(xs, ys):
            if not isinstance(y, DeviceArray) or y._hv is not None or y._t or y.dtype != dt or tuple(y.shape) != tuple(x.shape):
                raise TypeError("%s: an output must be a dense device array of the operand's shape %s and dtype %s"
                                % (what, tuple(x.shape), dt))
    pd = None if positions is None else _ragged_state(positions, what, "positions")
    lib = _lib.get()
    if len(xs[0].shape) != 4:
        raise ValueError("%s: the operands must have four axes (layout %r), got shape %s" % (what, layout, tuple(xs[0].shape)))
    d = int(xs[0].shape[3])
    R = rotary.width(d)
    float_ok = _decode_float_ok(dt)
    known = (R, dt) in rotary._device
    tabs = rotary._device[(R, dt)] if known else (None, None)
    plan = _rp.plan_rope(xs[0].shape, None if xb is None else xs[1].shape, R, rotary.max_len, offset,
                         None if pd is None else pd.shape, layout, rotary.pairing, inverse, blocks, dt.itemsize,
                         addresses=(xs[0]._ptr, _ptr_of(ys[0]), None if xb is None else xs[1]._ptr,
                                    None if xb is None else _ptr_of(ys[1]), _ptr_of(tabs[0]), _ptr_of(tabs[1])),
                         native=lib.has_rope, float_ok=float_ok, route=route or ROPE_ROUTE)
    ys = [DeviceArray._new(tuple(x.shape), dt) if y is None else y for x, y in zip(xs, ys)]
    result = ys[0] if xb is None else (ys[0], ys[1])
    if plan.empty():
        return result
    cos_t, sin_t = _rope_tables(rotary, R, dt)
    if plan.route == "native":
        xb_, yb_ = (xs[1], ys[1]) if xb is not None else (None, None)
        lib.rope_apply(xs[0]._ptr, ys[0]._ptr, _ptr_of(xb_), _ptr_of(yb_), cos_t._ptr, sin_t._ptr, _ptr_of(pd),
                       _i64arr(plan.geometry()), _i64arr(plan.strides()), plan.offset, int(plan.inverse), plan.pairing_code(),
                       plan.blocks, ys[0]._code())
        return result
    host = None
    if pd is not None:
        if _lib.capturing:
            raise RuntimeError("%s (composed route) reads the positions on the host, which a graph capture cannot do" % what)
        host = _ragged_mirror(positions, what)
    for x, y in zip(xs, ys):
        if x.size:
            _rope_composed(plan, x, y, cos_t, sin_t, host)
    return result


# ---------------------------------------------------------------------- kernels: gated activations (csrc/tnn_gated.hip)
GATED_ROUTE = None    # tests / probes: "native" or "composed" overrides the planner's choice (gated.py)


def _gated_act(g, act):
    """(a, act') of the composed route: a is always there, act' is a thunk evaluated only by the backward."""
    if act == "silu":
        sig = sigmoid(g)
        return g * sig, lambda: sig * ((g * (1.0 - sig)) + 1.0)
    t = _gelu_inner(g)
    return (g * 0.5) * (t + 1.0), lambda: (t + 1.0) * 0.5 + (g * 0.5) * (1.0 - t * t) * ((g * g) * (3.0 * _GELU_A) + 1.0) * _GELU_C


def _gated_operands(what, gate, up, dy, packed):
    """(dt, gate, up, dy, lead shape, M, F): dense operands of one float dtype; packed: gate is [.., 2 F] and up is None."""
    if packed and up is not None:
        raise ValueError("%s: packed=True takes ONE array [.., 2 F] (gate columns, then up columns), not gate and up" % what)
    dt, (gate, up, dy) = _operands(gate, up, dy)
    if len(gate.shape) < 1:
        raise ValueError("%s: the operands need at least one axis, got shape %s" % (what, tuple(gate.shape)))
    last = int(gate.shape[-1])
    if packed and last % 2:
        raise ValueError("%s: a packed operand holds gate and up columns, its last axis must be even, got shape %s"
                         % (what, tuple(gate.shape)))
    f = last // 2 if packed else last
    lead = tuple(int(s) for s in gate.shape[:-1])
    if up is not None and tuple(up.shape) != tuple(gate.shape):
        raise ValueError("%s: gate and up must have one shape, got %s and %s" % (what, tuple(gate.shape), tuple(up.shape)))
    if dy is not None and tuple(dy.shape) != lead + (f,):
        dy = dy._broadcast_to(lead + (f,))
    return dt, gate, up, dy, lead, _prod(lead), f


def gated(gate, up=None, act="silu", packed=False, route=None, blocks=0):
    """y = act(gate) * up, elementwise over arrays [.., F]; up=None: y = act(gate) (act="silu": the SiLU activation).
    act: "silu" (SwiGLU), "gelu_tanh" or "gelu" (GEGLU; gated.py).  packed=True: `gate` is ONE array [.., 2 F] — the gate
    columns, then the up columns, what a Dense(2 F) produces — and both halves are read in place, nothing is sliced or copied.
    Native: ONE tnn_gated_fwd launch (blocks: its workgroup count, 0 = the library's).  Composed (gated.py: the CPU test twin,
    route="composed"): sigmoid or tanh and products on the generic operations; the exact-GELU gate raises there."""
    what = "gated"
    dt, gate, up, _, lead, m, f = _gated_operands(what, gate, up, None, packed)
    lib = _lib.get()
    item = dt.itemsize
    has_up = packed or up is not None
    ld = 2 * f if packed else f
    addr = dict(gate=gate._ptr)
    if has_up:
        addr["up"] = gate._ptr + f * item if packed else up._ptr
    plan = _gt.plan_gated(m, f, act, False, has_up, lds=dict(gate=ld, up=ld), addresses=addr,
                          blocks=blocks, itemsize=item, native=lib.has_gated, float_ok=_decode_float_ok(dt),
                          route=route or GATED_ROUTE)
    if plan.empty():
        return zeros(lead + (f,), dt)
    if plan.route == "native":
        y = DeviceArray._new(lead + (f,), dt)
        lib.gated_fwd(addr["gate"], addr.get("up"), y._ptr, m, f, _i64arr(plan.strides()), plan.act_code(), plan.blocks,
                      y._code())
        return y
    g = gate[..., :f] if packed else gate
    u = gate[..., f:] if packed else up
    a, _ = _gated_act(g, act)
    return a if u is None else a * u


def gated_bwd(gate, up, dy, act="silu", packed=False, route=None, blocks=0, need_dgate=True, need_dup=True, dz_out=None):
    """The gradients of `gated` for the gradient dy of y, recomputed from gate: (dgate, dup) with dup = dy * act(gate) and
    dgate = (dy * up) * act'(gate) — None for one that is not needed (need_*) and for dup without up; packed=True: ONE array
    dz [.., 2 F] holding dgate columns, then dup columns, so the Dense backward behind it is one GEMM (dz_out: a dense array
    it is written into).  Native: ONE tnn_gated_bwd launch for whatever is asked."""
    what = "gated_bwd"
    dt, gate, up, dy, lead, m, f = _gated_operands(what, gate, up, dy, packed)
    lib = _lib.get()
    item = dt.itemsize
    has_up = packed or up is not None
    if packed:
        need_dgate = need_dup = True
    need_dup = need_dup and has_up
    if not (need_dgate or need_dup):
        return None, None
    ld = 2 * f if packed else f
    addr = dict(gate=gate._ptr, dy=dy._ptr)
    if has_up:
        addr["up"] = gate._ptr + f * item if packed else up._ptr
    dz = None
    if packed:
        dz = _grad_dest(dz_out, lead + (2 * f,), dt)
        if dz is not None:
            addr["dgate"], addr["dup"] = dz._ptr, dz._ptr + f * item
    plan = _gt.plan_gated(m, f, act, True, has_up, need_dgate, need_dup,
                          lds=dict(gate=ld, up=ld, dgate=ld, dup=ld), addresses=addr, blocks=blocks, itemsize=item,
                          native=lib.has_gated, float_ok=_decode_float_ok(dt), route=route or GATED_ROUTE)
    if plan.empty():
        if packed:
            return zeros(lead + (2 * f,), dt)
        return (zeros(lead + (f,), dt) if need_dgate else None), (zeros(lead + (f,), dt) if need_dup else None)
    if plan.route == "native":
        if packed:
            if dz is None:
                dz = DeviceArray._new(lead + (2 * f,), dt)
            lib.gated_bwd(addr["gate"], addr["up"], dy._ptr, dz._ptr, dz._ptr + f * item, m, f, _i64arr(plan.strides()),
                          plan.act_code(), plan.blocks, dz._code())
            return dz
        dgate = DeviceArray._new(lead + (f,), dt) if need_dgate else None
        dup = DeviceArray._new(lead + (f,), dt) if need_dup else None
        lib.gated_bwd(addr["gate"], addr.get("up"), dy._ptr, _ptr_of(dgate), _ptr_of(dup), m, f, _i64arr(plan.strides()),
                      plan.act_code(), plan.blocks, dy._code())
        return dgate, dup
    g = gate[..., :f] if packed else gate
    u = gate[..., f:] if packed else up
    a, slope = _gated_act(g, act)
    dgate = ((dy if u is None else dy * u) * slope()) if need_dgate else None
    dup = dy * a if need_dup else None
    if not packed:
        return dgate, dup
    out = dz if dz is not None else DeviceArray._new(lead + (2 * f,), dt)
    out[..., :f] = dgate
    out[..., f:] = dup
    return out


# ---------------------------------------------------------------------- kernels: advanced indexing (csrc/tnn_index.hip)
def _need_eager(what):
    if _lib.capturing:
        raise RuntimeError("%s inside a graph capture: the output shape depends on the data (a device boolean mask must "
                           "be counted and read back), which a captured graph cannot do; index with integer arrays or "
                           "run it outside the capture" % what)


class _DeviceHooks(_ix.HostHooks):
    """indexing.normalize's view of device-resident keys: they stay on the device."""

    def is_device(self, obj):
        return isinstance(obj, DeviceArray)

    def dtype_kind(self, obj):
        return obj.dtype.kind

    def as_index(self, obj):
        return obj.astype(np.int64)._contig()

    def nonzero(self, obj):
        return _nonzero(obj)

    def scalar_bool(self, obj):
        _need_eager("a device boolean index")
        return bool(obj.item())


_HOOKS = _DeviceHooks()


def _index_desc(plan):
    """indexing.IndexPlan -> the tnn_index_desc structure; host index arrays are uploaded (returned, to stay alive)."""
    desc = _lib.IndexDesc()
    desc.ndim = len(plan.out_shape)
    desc.narr = len(plan.arrays)
    desc.base = plan.base
    for d, (n, st) in enumerate(zip(plan.out_shape, plan.strides)):
        desc.shape[d] = n
        desc.stride[d] = st
    keep = []
    for k, (a, ist, astride, alen) in enumerate(plan.arrays):
        a = asarray(a) if isinstance(a, np.ndarray) else a
        keep.append(a)
        desc.idx[k] = a._ptr
        for d, s in enumerate(ist):
            desc.istride[k][d] = s
        desc.astride[k] = astride
        desc.alen[k] = alen
    return desc, keep


def _index_gather(src, key):
    """src[key] for any numpy key (indexing.py): ONE tnn_index_gather launch.  src: dense."""
    plan = _ix.normalize(src.shape, key, _HOOKS)
    out = DeviceArray._new(plan.out_shape, src.dtype)
    if out.size:
        desc, keep = _index_desc(plan)
        _lib.get().index_gather(src._ptr, out._ptr, ctypes.byref(desc), src.itemsize)
    return out


def _index_scatter(dst, key, value):
    """dst[key] = value for any numpy key: numpy's assignment — where targets repeat, the last position in C order of the
    broadcast index space wins, deterministically (tnn_index_scatter).  dst: dense, not transposed."""
    plan = _ix.normalize(dst.shape, key, _HOOKS)
    if plan.size == 0:
        return
    val = asarray(value).astype(dst.dtype)
    if val._hv is None:
        val = val._contig()
        while val.ndim > len(plan.out_shape) and val.shape[0] == 1:      # numpy drops leading unit dims of the value
            val = val.reshape(val.shape[1:])
    vst = _broadcast_strides(val.shape, plan.out_shape)
    desc, keep = _index_desc(plan)
    lib = _lib.get()
    unique = plan.unique
    winner = None
    if not unique:
        winner = DeviceArray._new((plan.target_count(),), np.int64)
        lib.fill(winner._ptr, -1.0, winner.size, I64)
    lib.index_scatter(val._dev(), _i64arr(vst) if vst else _i64arr((0,)), dst._ptr, ctypes.byref(desc), int(unique),
                      winner._ptr if winner is not None else None, dst.itemsize)


def _mask_total(m):
    """(scratch, total) of a dense bool device array: launches 1 and 2 of the mask path plus one 8-B read-back."""
    lib = _lib.get()
    elems = ctypes.c_int64(0)
    lib.mask_scratch_elems(m.size, ctypes.byref(elems))
    scratch = DeviceArray._new((elems.value,), np.int64)
    lib.mask_count(m._ptr if m.size else None, m.size, scratch._ptr)
    total = np.zeros(1, dtype=np.int64)
    lib.memcpy_d2h(total.ctypes.data, scratch._ptr + (elems.value - 1) * 8, 8)
    return scratch, int(total[0])


def _as_mask(a):
    a = asarray(a)
    if a._hv is not None:
        a = a._contig()
    return (a if a.dtype == np.bool_ else _compare(_lib.NE, a, 0.0))._contig()


def _nonzero(a):
    """np.nonzero on the device: a tuple of int64 coordinate arrays in C order (tnn_mask_count + tnn_mask_nonzero)."""
    _need_eager("nonzero of a device array")
    m = _as_mask(a)
    if m.ndim == 0:
        raise ValueError("Calling nonzero on 0d arrays is not allowed. Use np.atleast_1d(scalar).nonzero() instead.")
    if m.ndim > MAX_NDIM:
        raise TypeError("nonzero supports up to %d dimensions on device" % MAX_NDIM)
    scratch, count = _mask_total(m)
    coords = DeviceArray._new((m.ndim, count), np.int64)
    if count:
        _lib.get().mask_nonzero(m._ptr, m.size, scratch._ptr, m.ndim, _i64arr(m.shape), coords._ptr, count)
    return tuple(coords[k] for k in range(m.ndim))


def _np_count_nonzero(a, axis=None, keepdims=False):
    if axis is not None or keepdims:
        raise TypeError("np.count_nonzero on device supports axis=None only")
    _need_eager("count_nonzero of a device array")
    m = _as_mask(a)
    return _mask_total(m)[1]


def _np_flatnonzero(a):
    return _nonzero(asarray(a)._contig().ravel())[0]


def expand_masks(key):
    """The key with every DEVICE boolean mask replaced by its nonzero() coordinate arrays (numpy's own rule for a mask), so
    that a forward and its vjp index with one read-back between them (core/ops.py getitem_)."""
    items = key if isinstance(key, tuple) else (key,)
    if not any(isinstance(k, DeviceArray) and k.dtype == np.bool_ and k.ndim > 0 for k in items):
        return key
    out = []
    for k in items:
        if isinstance(k, DeviceArray) and k.dtype == np.bool_ and k.ndim > 0:
            out.extend(_nonzero(k))
        else:
            out.append(k)
    return tuple(out)


# ---------------------------------------------------------------------- numpy function overrides
def _np_concatenate(arrays, axis=0, **_):
    arrays = [asarray(x)._contig() for x in arrays]
    if not arrays:
        raise ValueError("need at least one array to concatenate")
    if axis is None:
        arrays, axis = [x.ravel() for x in arrays], 0
    nd = arrays[0].ndim
    axis = int(axis) % nd
    dts = [x.dtype for x in arrays]
    dt = dts[0] if all(d == dts[0] for d in dts) else _float_result_dtype(
        *[x for x in arrays if x.dtype.kind == "f"][:2] or arrays[:2])
    arrays = [x.astype(dt) for x in arrays]
    for x in arrays:
        if x.ndim != nd or x.shape[:axis] + x.shape[axis + 1:] != arrays[0].shape[:axis] + arrays[0].shape[axis + 1:]:
            raise ValueError("all the input array dimensions except for the concatenation axis must match exactly")
    out_shape = list(arrays[0].shape)
    out_shape[axis] = sum(x.shape[axis] for x in arrays)
    if axis == 0:
        # zero-copy when the pieces are consecutive slices of one buffer (the flat gradient arena)
        p, base, ok = arrays[0]._ptr, arrays[0]._base, arrays[0]._base is not None
        for x in arrays:
            ok = ok and x._base is base and x._ptr == p
            p = (p or 0) + x.nbytes
        if ok:
            return DeviceArray._raw(arrays[0]._ptr, out_shape, dt, base=base)
        out = DeviceArray._new(out_shape, dt)
        off = 0
        for x in arrays:
            if x.size:
                _lib.get().memcpy_d2d(out._ptr + off, x._ptr, x.nbytes)
            off += x.nbytes
        return out
    out = DeviceArray._new(out_shape, dt)
    pos = 0
    for x in arrays:
        key = [slice(None)] * nd
        key[axis] = slice(pos, pos + x.shape[axis])
        out[tuple(key)] = x
        pos += x.shape[axis]
    return out


def _np_reshape(a, *shape, **kwargs):
    if not shape:
        shape = (kwargs.get("newshape", kwargs.get("shape")),)
    return asarray(a).reshape(*shape)


def _np_expand_dims(a, axis):
    a = asarray(a)._contig()
    axis = int(axis)
    if axis < 0:
        axis += a.ndim + 1
    return a.reshape(a.shape[:axis] + (1,) + a.shape[axis:])


def _np_repeat(a, repeats, axis=None):
    a = asarray(a)._contig()
    repeats = int(repeats)
    if axis is None:
        a, axis = a.ravel(), 0
    axis = int(axis) % a.ndim
    # out[..., i*repeats + r, ...] = a[..., i, ...]  ->  view a as [..., n, 1, ...] and broadcast
    expanded = a.reshape(a.shape[:axis + 1] + (1,) + a.shape[axis + 1:])
    target = a.shape[:axis + 1] + (repeats,) + a.shape[axis + 1:]
    out = expanded._broadcast_to(target)
    return out.reshape(a.shape[:axis] + (a.shape[axis] * repeats,) + a.shape[axis + 1:])


_PAD_GATHER_MODES = ("edge", "reflect", "symmetric", "wrap")


def _np_pad(a, pad_width, mode="constant", **kwargs):
    if mode in _PAD_GATHER_MODES and not kwargs:
        # one gather: per axis a source table np.pad(arange(n), (before, after), mode) — tiny, and it handles widths past
        # the axis (which reflect repeats) — passed as np.ix_-shaped index arrays, broadcast through stride 0
        a = asarray(a)._contig()
        pw = np.broadcast_to(np.asarray(pad_width, dtype=np.int64), (a.ndim, 2))
        tables = [np.pad(np.arange(n, dtype=np.int64), (int(b), int(e)), mode) for n, (b, e) in zip(a.shape, pw)]
        if not tables:
            return a.copy()
        return _index_gather(a, np.ix_(*tables))
    cv = kwargs.get("constant_values", 0)
    if mode != "constant" or set(kwargs) - {"constant_values"} or np.ndim(cv) != 0:
        raise TypeError("np.pad on device supports the modes constant (scalar constant_values), edge, reflect, symmetric "
                        "and wrap")
    if cv != 0:
        a = asarray(a)._contig()
        pw = np.broadcast_to(np.asarray(pad_width, dtype=np.int64), (a.ndim, 2))
        out = full(tuple(int(s + b + e) for s, (b, e) in zip(a.shape, pw)), float(cv), a.dtype)
        if a.size:
            out[tuple(slice(int(b), int(b) + s) for s, (b, e) in zip(a.shape, pw))] = a
        return out
    a = asarray(a)._contig()
    pw = np.broadcast_to(np.asarray(pad_width, dtype=np.int64), (a.ndim, 2))
    out_shape = tuple(int(s + b + e) for s, (b, e) in zip(a.shape, pw))
    out = zeros(out_shape, a.dtype)
    key = tuple(slice(int(b), int(b) + s) for s, (b, e) in zip(a.shape, pw))
    if a.size:
        out[key] = a
    return out


def _np_where(cond, x=None, y=None):
    if x is None and y is None:
        return _nonzero(cond)
    if x is None or y is None:
        raise ValueError("either both or neither of x and y should be given")
    c = asarray(cond)
    c = c if c.dtype == np.bool_ else _compare(_lib.NE, c, 0.0)
    cf = c.astype(_float_result_dtype(asarray(x), asarray(y)))
    return cf * x + (1.0 - cf) * y


def _np_allclose(a, b, rtol=1e-5, atol=1e-8, equal_nan=False):
    return bool(np.allclose(np.asarray(a), np.asarray(b), rtol=rtol, atol=atol, equal_nan=equal_nan))


def _np_array_equal(a, b, **_):
    return bool(np.array_equal(np.asarray(a), np.asarray(b)))


_UFUNC_BINARY = {np.add: _lib.ADD, np.subtract: _lib.SUB, np.multiply: _lib.MUL,
                 np.true_divide: _lib.DIV, np.power: _lib.POW, np.maximum: _lib.MAX,
                 np.minimum: _lib.MIN, np.float_power: _lib.POW}
_UFUNC_COMPARE = {np.greater: _lib.GT, np.greater_equal: _lib.GE, np.less: _lib.LT,
                  np.less_equal: _lib.LE, np.equal: _lib.EQ, np.not_equal: _lib.NE}
_UFUNC_UNARY = {np.negative: _lib.NEG, np.exp: _lib.EXP, np.log: _lib.LOG, np.sqrt: _lib.SQRT,
                np.square: _lib.SQUARE, np.absolute: _lib.ABS, np.reciprocal: _lib.RECIP,
                np.tanh: _lib.TANH}
_UFUNC_REDUCE = {np.add: _lib.RSUM, np.maximum: _lib.RMAX, np.minimum: _lib.RMIN}

_ARRAY_FUNCTIONS = {
    np.ravel: lambda a, order="C": asarray(a).ravel(),
    np.reshape: _np_reshape,
    np.transpose: lambda a, axes=None: asarray(a).transpose(axes),
    np.swapaxes: lambda a, axis1, axis2: asarray(a).swapaxes(axis1, axis2),
    np.concatenate: _np_concatenate,
    np.sum: lambda a, axis=None, keepdims=False, **_: _reduce(_lib.RSUM, a, axis, keepdims),
    np.max: lambda a, axis=None, keepdims=False, **_: _reduce(_lib.RMAX, a, axis, keepdims),
    np.min: lambda a, axis=None, keepdims=False, **_: _reduce(_lib.RMIN, a, axis, keepdims),
    np.mean: lambda a, axis=None, keepdims=False, **_: asarray(a).mean(axis, keepdims),
    np.argmax: argmax,
    np.zeros_like: zeros_like,
    np.ones_like: ones_like,
    np.expand_dims: _np_expand_dims,
    np.repeat: _np_repeat,
    np.clip: clip,
    np.pad: _np_pad,
    np.where: _np_where,
    np.nonzero: _nonzero,
    np.flatnonzero: _np_flatnonzero,
    np.count_nonzero: _np_count_nonzero,
    np.copy: lambda a, **_: asarray(a).copy(),
    np.take: lambda a, indices, axis=None, out=None, mode="raise": asarray(a).take(indices, axis=axis, out=out, mode=mode),
    np.shape: lambda a: asarray(a).shape,
    np.ndim: lambda a: asarray(a).ndim,
    np.size: lambda a, axis=None: asarray(a).size if axis is None else asarray(a).shape[axis],
    np.dot: _np_dot,
    np.matmul: matmul,
    np.allclose: _np_allclose,
    np.array_equal: _np_array_equal,
    np.squeeze: lambda a, axis=None: asarray(a).reshape(
        [s for i, s in enumerate(asarray(a).shape)
         if not (s == 1 and (axis is None or i == (axis % asarray(a).ndim)))]),
}
