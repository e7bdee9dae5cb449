"""Key normaliser of numpy advanced indexing: `(shape, key)` -> one gather / scatter descriptor (IndexPlan).

Host-only and free of the library (imports numpy alone), so the whole rule set is testable without a device
(tests/test_indexing_keys.py).  device_array.py executes a plan with ONE tnn_index_gather or tnn_index_scatter launch
(csrc/tnn_index.hip).

A key is any numpy-valid mix of ints, slices, None, Ellipsis, integer arrays / lists of any dimension and boolean arrays,
on the host or on the device, with Tensors anywhere (their `.values`).  numpy's rules, followed exactly:
  * index arrays (and, once there is one, the integer scalars) broadcast against each other;
  * if the advanced indices are adjacent in the key (after Ellipsis expansion), their broadcast dims take their place in
    the output; a slice, None or a non-empty Ellipsis between them moves the broadcast dims to the front;
  * a k-dim boolean array stands for its k `nonzero()` coordinate arrays and must match the k axes it covers;
  * host integer arrays are bounds-checked and wrapped here (IndexError, as numpy); device arrays are checked in the kernel
    (an out-of-range entry gathers 0 and is skipped by a scatter).

The plan: the source element of output coordinate c is
    base + sum_d c_d * strides[d] + sum_k wrap(idx_k[sum_d c_d * istrides_k[d]]) * astride_k
with strides[d] == 0 on the dims the index arrays make.
"""

import math
import numbers

import numpy as np

MAX_NDIM = 6          # output dims of one launch (device_array.MAX_NDIM)
MAX_ARRAYS = 6        # index arrays of one launch


class IndexPlan(object):
    """out_shape, base (element offset into the dense source), strides (source stride per output dim, 0 for the advanced
    dims), arrays: [(idx, istrides, astride, alen)] — idx int64 (numpy, C-contiguous, wrapped into [0, alen), or a device
    array from the hooks, unchecked), istrides its stride per output dim (0 where it broadcasts), astride / alen the stride
    and length of the source axis it indexes.  adv = (first, count) of the broadcast dims in out_shape.  unique: the
    advanced targets are known to be distinct (a scatter needs no duplicate resolution)."""
    __slots__ = ("out_shape", "base", "strides", "arrays", "adv", "_unique", "device")

    def __init__(self, out_shape, base, strides, arrays, adv, unique, device):
        self.out_shape, self.base, self.strides, self.arrays = out_shape, base, strides, arrays
        self.adv, self._unique, self.device = adv, unique, device

    @property
    def size(self):
        return math.prod(self.out_shape)

    @property
    def unique(self):
        """The advanced targets are provably distinct: a mask alone, or host arrays that pass np.unique (computed on first
        use: only a scatter asks).  A device key with other arrays is never proved unique."""
        if self._unique is None:
            self._unique = _host_unique(self.arrays, self.out_shape[self.adv[0]:self.adv[0] + self.adv[1]], self.adv[0])
        return self._unique

    def target_count(self):
        """Entries of the duplicate-resolution table: the product of the indexed axes' lengths."""
        return math.prod(a[3] for a in self.arrays)


def dense_strides(shape):
    st, acc = [], 1
    for s in reversed(shape):
        st.append(acc)
        acc *= int(s)
    return tuple(reversed(st))


class HostHooks(object):
    """Where the index arrays live.  The default: everything is converted to a numpy array.  device_array supplies hooks
    that keep device arrays on the device."""

    def is_device(self, obj):
        return False

    def dtype_kind(self, obj):
        return obj.dtype.kind

    def as_index(self, obj):          # -> an int64 array (device hooks: a contiguous device array)
        raise NotImplementedError

    def nonzero(self, obj):           # -> tuple of k int64 coordinate arrays of a k-dim device mask
        raise NotImplementedError

    def scalar_bool(self, obj):       # 0-d device mask -> its value
        raise NotImplementedError


_HOST = HostHooks()


def _unwrap(k):
    """A Tensor (anything with `.values` that is not an ndarray) stands for its values."""
    if not isinstance(k, (np.ndarray, list, tuple, slice, numbers.Number, np.generic)) and k is not None \
            and k is not Ellipsis and hasattr(k, "values") and hasattr(k, "grad"):
        return k.values
    return k


def _is_int(k):
    return isinstance(k, (numbers.Integral, np.integer)) and not isinstance(k, (bool, np.bool_))


def _host_array(k):
    if isinstance(k, list):
        a = np.asarray(k)
        if a.size == 0 and a.dtype.kind == "f":
            a = a.astype(np.int64)           # numpy: an empty list is an empty integer index
        if a.dtype == object:
            raise IndexError("only integers, slices (`:`), ellipsis (`...`), numpy.newaxis (`None`) and integer or "
                             "boolean arrays are valid indices")
        return a
    return k


def is_basic(key):
    """True when the key holds only ints, slices, None and Ellipsis (a strided view or copy; no index arrays)."""
    items = key if isinstance(key, tuple) else (key,)
    for k in items:
        if k is None or k is Ellipsis or isinstance(k, slice):
            continue
        if _is_int(k):
            continue
        if isinstance(k, np.ndarray) and k.ndim == 0 and k.dtype.kind in "iu":
            continue
        return False
    return True


def normalize(shape, key, hooks=None):
    """(shape of a dense C-order source, key) -> IndexPlan.  Raises IndexError where numpy does; TypeError past the
    device limits (MAX_NDIM output dims, MAX_ARRAYS index arrays)."""
    hooks = hooks or _HOST
    shape = tuple(int(s) for s in shape)
    ndim = len(shape)
    src_st = dense_strides(shape)
    items = key if isinstance(key, tuple) else (key,)

    # classify: ("none",), ("ell",), ("slice", s), ("int", i), ("arr", a, dev), ("bool", a, dev)
    cls = []
    for k in items:
        k = _unwrap(k)
        if k is None:
            cls.append(("none",))
        elif k is Ellipsis:
            cls.append(("ell",))
        elif isinstance(k, slice):
            cls.append(("slice", k))
        elif isinstance(k, (bool, np.bool_)):
            cls.append(("bool", np.asarray(bool(k)), False))
        elif _is_int(k):
            cls.append(("int", int(k)))
        elif hooks.is_device(k):
            kind = hooks.dtype_kind(k)
            if kind == "b":
                if len(k.shape) == 0:
                    cls.append(("bool", np.asarray(bool(hooks.scalar_bool(k))), False))
                else:
                    cls.append(("bool", k, True))
            elif kind in "iu":
                cls.append(("arr", k, True))
            else:
                raise IndexError("arrays used as indices must be of integer (or boolean) type")
        else:
            a = _host_array(k)
            if not isinstance(a, np.ndarray):
                if isinstance(a, (numbers.Number, np.generic)):
                    raise IndexError("only integers, slices (`:`), ellipsis (`...`), numpy.newaxis (`None`) and "
                                     "integer or boolean arrays are valid indices")
                a = np.asarray(a)
            if a.dtype.kind == "b":
                cls.append(("bool", a, False))
            elif a.dtype.kind in "iu":
                if a.ndim == 0:
                    cls.append(("int", int(a)))
                else:
                    cls.append(("arr", a, False))
            else:
                raise IndexError("arrays used as indices must be of integer (or boolean) type")

    # Ellipsis -> the slices it stands for
    consumed = 0
    n_ell = 0
    for c in cls:
        if c[0] in ("slice", "int", "arr"):
            consumed += 1
        elif c[0] == "bool":
            consumed += len(c[1].shape)
        elif c[0] == "ell":
            n_ell += 1
    if n_ell > 1:
        raise IndexError("an index can only have a single ellipsis ('...')")
    if consumed > ndim:
        raise IndexError("too many indices for array: array is %d-dimensional, but %d were indexed" % (ndim, consumed))
    expanded = []
    for c in cls:
        if c[0] == "ell":
            expanded.extend([("slice", slice(None))] * (ndim - consumed))
        else:
            expanded.append(c)
    if n_ell == 0:
        expanded.extend([("slice", slice(None))] * (ndim - consumed))

    has_adv = any(c[0] in ("arr", "bool") for c in expanded)

    # walk the key: basic output dims, advanced entries [(array, dev, axis)], positions of the advanced entries in the key
    base = 0
    basic = []                  # (len, stride) in output order, with the marker "ADV" where the block would go if adjacent
    adv_entries = []            # (array or int, is_device, axis)
    adv_pos = []
    dim = 0
    first_adv_out = None
    mask_only = True            # every advanced entry comes from ONE mask (its targets are distinct)
    n_masks = 0
    for pos, c in enumerate(expanded):
        kind = c[0]
        if kind == "none":
            basic.append((1, 0))
        elif kind == "slice":
            n = shape[dim]
            start, stop, step = c[1].indices(n)
            length = len(range(start, stop, step))
            if length:
                base += start * src_st[dim]
            basic.append((length, step * src_st[dim]))
            dim += 1
        elif kind == "int":
            n = shape[dim]
            i = c[1]
            if not -n <= i < n:
                raise IndexError("index %d is out of bounds for axis %d with size %d" % (i, dim, n))
            i %= n
            if has_adv:                         # numpy: a scalar joins the advanced group (broadcast shape ())
                if first_adv_out is None:
                    first_adv_out = len(basic)
                adv_entries.append((np.asarray(i, dtype=np.int64), False, dim))
                adv_pos.append(pos)
                mask_only = False
            else:
                base += i * src_st[dim]
            dim += 1
        elif kind == "arr":
            if first_adv_out is None:
                first_adv_out = len(basic)
            adv_entries.append((c[1], c[2], dim))
            adv_pos.append(pos)
            mask_only = False
            dim += 1
        else:                                   # boolean mask over len(a.shape) axes (0-d: no axis, a 0/1-length dim)
            m, dev = c[1], c[2]
            if first_adv_out is None:
                first_adv_out = len(basic)
            n_masks += 1
            k = len(m.shape)
            if tuple(m.shape) != shape[dim:dim + k]:
                for j, s in enumerate(m.shape):
                    if s != shape[dim + j]:
                        raise IndexError("boolean index did not match indexed array along axis %d; size of axis is %d "
                                         "but size of corresponding boolean axis is %d" % (dim + j, shape[dim + j], s))
            if k == 0:
                n_true = 1 if bool(m) else 0
                adv_entries.append((np.zeros(n_true, dtype=np.int64), False, None))
                adv_pos.append(pos)
                continue
            coords = hooks.nonzero(m) if dev else np.nonzero(m)
            for j in range(k):
                adv_entries.append((coords[j], dev, dim + j))
                adv_pos.append(pos)         # one entry of the key: its coordinate arrays are adjacent
            dim += k

    if not adv_entries:
        out_shape = tuple(l for l, _ in basic)
        strides = tuple(s for _, s in basic)
        _check_ndim(out_shape)
        return IndexPlan(out_shape, base, strides, [], (0, 0), True, False)

    # adjacency over the (Ellipsis-expanded) key
    adjacent = all(adv_pos[i + 1] - adv_pos[i] <= 1 for i in range(len(adv_pos) - 1))
    # broadcast shape of the index arrays
    shapes = [tuple(a.shape) for a, _, _ in adv_entries]
    try:
        bshape = tuple(int(s) for s in np.broadcast_shapes(*shapes))
    except ValueError:
        raise IndexError("shape mismatch: indexing arrays could not be broadcast together with shapes %s"
                         % " ".join(str(s) for s in shapes)) from None
    at = first_adv_out if adjacent else 0
    out_shape = tuple(l for l, _ in basic[:at]) + bshape + tuple(l for l, _ in basic[at:])
    strides = tuple(s for _, s in basic[:at]) + (0,) * len(bshape) + tuple(s for _, s in basic[at:])
    _check_ndim(out_shape)

    arrays = []
    device = False
    for a, dev, axis in adv_entries:
        if axis is None:                        # 0-d boolean: a virtual axis of length 1
            alen, astride = 1, 0
        else:
            alen, astride = shape[axis], src_st[axis]
        if dev:
            device = True
            a = hooks.as_index(a)
        else:
            a = np.asarray(a)
            if a.size:
                lo, hi = int(a.min()), int(a.max())
                if lo < -alen or hi >= alen:
                    bad = lo if lo < -alen else hi
                    raise IndexError("index %d is out of bounds for axis %d with size %d" % (bad, axis, alen))
            a = np.asarray(np.where(a < 0, a + alen, a) if a.size and a.min() < 0 else a, dtype=np.int64)
            if not a.flags.c_contiguous:
                a = a.copy()
        if a.ndim == 0 and not dev and alen:       # a host scalar of the group: folded into the base offset
            base += int(a) * astride
            continue
        ist = [0] * len(out_shape)
        own = dense_strides(a.shape)
        lead = len(bshape) - len(a.shape)
        for j, s in enumerate(a.shape):
            ist[at + lead + j] = own[j] if s != 1 else 0
        arrays.append((a, tuple(ist), astride, alen))
    if len(arrays) > MAX_ARRAYS:
        raise TypeError("advanced indexing supports up to %d index arrays on device" % MAX_ARRAYS)

    unique = True if (mask_only and n_masks == 1) or not arrays else (False if device else None)
    return IndexPlan(out_shape, base, strides, arrays, (at, len(bshape)), unique, device)


def _check_ndim(out_shape):
    if len(out_shape) > MAX_NDIM:
        raise TypeError("indexing supports up to %d output dimensions on device" % MAX_NDIM)


def _host_unique(arrays, bshape, at):
    """The linearised targets of host index arrays are pairwise distinct (np.unique)."""
    total = math.prod(bshape)
    if total <= 1:
        return True
    lin = np.zeros(bshape, dtype=np.int64)
    for a, ist, astride, alen in arrays:
        view = np.lib.stride_tricks.as_strided(a, shape=bshape,
                                               strides=tuple(s * 8 for s in ist[at:at + len(bshape)]))
        lin = lin * alen + view
    return np.unique(lin).size == total


def evaluate(flat_src, plan):
    """Pure-numpy execution of a host plan: the gather the kernel performs (tests; no device)."""
    offs = _offsets(plan)
    return flat_src[offs] if offs.size else np.empty(plan.out_shape, flat_src.dtype)


def _offsets(plan):
    shape = plan.out_shape
    off = np.full(shape, plan.base, dtype=np.int64)
    grids = np.indices(shape, dtype=np.int64) if shape else np.zeros((0,), dtype=np.int64)
    for d in range(len(shape)):
        off = off + grids[d] * plan.strides[d]
    for a, ist, astride, alen in plan.arrays:
        ioff = np.zeros(shape, dtype=np.int64)
        for d in range(len(shape)):
            ioff = ioff + grids[d] * ist[d]
        off = off + a.ravel()[ioff] * astride if a.size else off
    return off


def scatter(flat_dst, plan, val):
    """Pure-numpy restatement of the deterministic scatter (`dst[key] = val`, numpy's assignment): pass 1 keeps, per
    target of the indexed axes, the LAST advanced position in C order of the broadcast index space (winner); pass 2
    stores the output elements whose position is their target's winner."""
    val = np.broadcast_to(np.asarray(val, dtype=flat_dst.dtype), plan.out_shape)
    shape = plan.out_shape
    if not math.prod(shape):
        return flat_dst
    offs = _offsets(plan)
    at, nb = plan.adv
    grids = np.indices(shape, dtype=np.int64)
    pos = np.zeros(shape, dtype=np.int64)
    for d in range(at, at + nb):
        pos = pos * shape[d] + grids[d]
    tgt = np.zeros(shape, dtype=np.int64)
    for a, ist, astride, alen in plan.arrays:
        ioff = np.zeros(shape, dtype=np.int64)
        for d in range(len(shape)):
            ioff = ioff + grids[d] * ist[d]
        tgt = tgt * alen + a.ravel()[ioff]
    winner = np.full(plan.target_count(), -1, dtype=np.int64)
    np.maximum.at(winner, tgt.ravel(), pos.ravel())
    keep = winner[tgt] == pos
    flat_dst[offs[keep]] = val[keep]
    return flat_dst
