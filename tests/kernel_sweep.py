"""Sweep of the generic op kernels (csrc/tnn_ewise.hip, tnn_reduce.hip, bias_act of tnn_fused.hip) against numpy at
their dispatch edges.  Backend-agnostic, like parity_suite.py: test_gpu_kernel_sweep.py runs the families through
libtnn_hip.so on the MI355X, test_kernel_sweep_twin.py through the CPU twin (which exercises the harness and the
references themselves in the container).

Every call goes through the C-ABI with raw device pointers.  An operand is a slice of a larger allocation: guard
elements filled with a sentinel lie before and after it, and a whole-element offset of 0..3 makes its base miss the
16-byte alignment that the vector kernels ask for.  After the call the guards must be unchanged, so a write outside
the range shows up as a value and not as a fault.  The reference is always numpy on the same input bits.

One entry of CASES per (family, dtype); a family loops over its cases and collects every failure as
`family/op/shape/offsets: max err, first bad index` before it asserts.
"""

import ctypes
import itertools
import math
import os

import numpy as np

from tinynn_autograd_amd import _lib
from tinynn_autograd_amd import device_array as da

# Gates of the operations that go through the device libm, in ulps of the dtype against float64 numpy: the maximum
# observed on the MI355X (profiles/kernel_sweep_ulp.txt) rounded up to the next integer, plus 1 ulp for inputs the
# sweep did not draw.  None may exceed 16 ulp (what rtol=2e-6 of parity_suite.elementwise_broadcast_reduce allows).
ULP_GATES = {
    ("exp", "float32"): 2, ("exp", "float64"): 2,              # observed 0.98, 1.00
    ("log", "float32"): 4, ("log", "float64"): 2,              # observed 2.18, 1.00
    ("tanh", "float32"): 3, ("tanh", "float64"): 2,            # observed 1.28, 1.00
    ("sigmoid", "float32"): 3, ("sigmoid", "float64"): 3,      # observed 1.84, 2.00
    ("pow", "float32"): 3, ("pow", "float64"): 2,              # observed 1.34, 1.00
}
OBSERVED_ULP = {}                      # (op, dtype name) -> largest error seen in this process

BUFFER_LIMIT = 256 << 20               # no single buffer above this
GUARD_BYTES = 64                       # a multiple of 16: offset 0 keeps the payload 16-byte aligned
CODE = {"float32": _lib.F32, "float64": _lib.F64, "int64": _lib.I64, "uint8": _lib.U8}
FLOATS = ("float32", "float64")
ALL_DTYPES = ("float32", "float64", "int64", "uint8")
OFFSETS3 = [(0, 0, 0), (1, 0, 0), (0, 2, 0), (0, 0, 3), (1, 2, 3)]      # (a, b, out): each pointer unaligned in turn
OFFSETS2 = [(0, 0), (1, 0), (0, 3), (2, 1)]


def lib():
    return _lib.get()


def device_limits():
    """The launch caps of the kernels, from the device's CU count (tnn::stream_grid: 8 blocks per CU of 256 threads).  The
    CPU twin reports no CUs: the MI355X's 256 are used there so that the same cases run."""
    cus = _lib.device_props()["cus"] or 256
    cap = 8 * cus
    return {"cus": cus, "block_cap": cap, "pass_scalar": cap * 256}


def sentinel(dt):
    dt = np.dtype(dt)
    if dt.kind == "f":
        return dt.type(-123456.0)
    if dt == np.uint8:
        return dt.type(0xA5)
    return dt.type(-0x5A5A5A5A5A5A5A5A)


class Dev(object):
    """`n` elements on the device inside a larger allocation: [guard | off elements | payload | guard], all pre-filled
    with the sentinel; `data` (if given) is copied into the payload."""

    def __init__(self, data=None, n=None, dtype=None, off=0):
        if data is not None:
            data = np.ascontiguousarray(data)
            n, dtype = data.size, data.dtype
        self.dt = np.dtype(dtype)
        self.n, self.off = int(n), int(off)
        self.g = GUARD_BYTES // self.dt.itemsize
        total = 2 * self.g + self.off + self.n
        assert total * self.dt.itemsize <= BUFFER_LIMIT + 4 * GUARD_BYTES, "buffer of %d bytes" % (total * self.dt.itemsize)
        self.image = np.full(total, sentinel(self.dt), self.dt)
        if data is not None:
            self.image[self.g + self.off:self.g + self.off + self.n] = data.ravel()
        self.buf = da.DeviceArray._new((total * self.dt.itemsize,), np.bool_)
        assert self.buf._ptr % 16 == 0, "allocator returned a base that is not 16-byte aligned"
        lib().memcpy_h2d(self.buf._ptr, self.image.ctypes.data, self.image.nbytes)
        self.ptr = self.buf._ptr + (self.g + self.off) * self.dt.itemsize      # whole elements only

    def at(self, elem):
        """Pointer `elem` elements into the payload (the start of a strided view); must stay inside it."""
        assert 0 <= elem < max(self.n, 1)
        return self.ptr + elem * self.dt.itemsize

    def read(self):
        """(payload, index of the first changed guard element or None)."""
        got = np.empty_like(self.image)
        lib().memcpy_d2h(got.ctypes.data, self.buf._ptr, got.nbytes)
        lo, hi = self.g + self.off, self.g + self.off + self.n
        guards = np.concatenate([got[:lo], got[hi:]])
        bad = np.flatnonzero(_bits(guards) != _bits(np.full(guards.size, sentinel(self.dt), self.dt)))
        first = None
        if bad.size:
            first = int(bad[0]) - lo if bad[0] < lo else int(bad[0]) - lo + self.n
        return got[lo:hi].copy(), first


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _signed_zero_free(a):
    """-0.0 -> +0.0 (for max/min results: which zero wins a +0/-0 tie is unspecified by IEEE 754's maximum, and numpy's own
    scalar and vector loops disagree about it, so the reference has no single answer there)."""
    a = a.copy()
    a[a == 0] = 0
    return a


class Report(object):
    def __init__(self, family, dtype):
        self.family, self.dtype, self.fails, self.checks = family, dtype, [], 0

    def _fail(self, label, text):
        self.fails.append("%s/%s: %s" % (self.family, label, text))

    def guard(self, label, first_bad):
        self.checks += 1
        if first_bad is not None:
            self._fail(label, "guard element changed at payload index %d (write outside the output range)" % first_bad)

    def bits(self, label, got, ref, zero_sign=True):
        """Bit equality in the output dtype; any NaN equals any NaN (payloads excepted)."""
        self.checks += 1
        got, ref = np.asarray(got).ravel(), np.asarray(ref).ravel()
        if got.size != ref.size:
            return self._fail(label, "size %d, expected %d" % (got.size, ref.size))
        if got.dtype != ref.dtype:
            return self._fail(label, "reference dtype %s, output dtype %s" % (ref.dtype, got.dtype))
        if not zero_sign:
            got, ref = _signed_zero_free(got), _signed_zero_free(ref)
        same = _bits(got) == _bits(ref)
        if got.dtype.kind == "f":
            same |= np.isnan(got) & np.isnan(ref)
        if not same.all():
            bad = np.flatnonzero(~same)
            with np.errstate(all="ignore"):
                err = np.nanmax(np.abs(got[bad].astype(np.float64) - ref[bad].astype(np.float64))) if got.dtype.kind == "f" \
                    else np.max(np.abs(got[bad].astype(np.float64) - ref[bad].astype(np.float64)))
            self._fail(label, "%d of %d differ, max err %.6g, first bad index %d (got %r, expected %r)"
                       % (bad.size, got.size, err, bad[0], got[bad[0]], ref[bad[0]]))

    def ulps(self, label, got, ref_hi, gate, key=None, at=None):
        """|got - ref_hi| in ulps of got's dtype at the rounded reference; inf, NaN and exact zeros (with their sign) must
        match exactly.  `ref_hi` is the higher-precision reference before rounding.  Records the maximum under `key`.
        `at`: magnitudes at which the ulp is taken where they exceed the result's (an intermediate that was rounded)."""
        self.checks += 1
        got = np.asarray(got).ravel()
        ref_hi = np.asarray(ref_hi).ravel()
        with np.errstate(all="ignore"):
            ref_r = ref_hi.astype(got.dtype)
            special = ~np.isfinite(ref_r) | (ref_hi == 0)
            ok = np.ones(got.size, bool)
            s = special
            ok[s] = (np.isnan(got[s]) & np.isnan(ref_r[s])) | (_bits(got[s]) == _bits(ref_r[s]))
            f = ~special
            err = np.zeros(got.size)
            hi_t = ref_hi.dtype.type
            err[f] = (np.abs(got[f].astype(ref_hi.dtype) - ref_hi[f]) / np.spacing(np.abs(ref_r[f]) if at is None else np.maximum(np.abs(ref_r[f]), np.abs(np.asarray(at).ravel()[f]).astype(got.dtype))).astype(ref_hi.dtype)).astype(np.float64)
            err[f & ~np.isfinite(got)] = np.inf
            del hi_t
        worst = float(err.max()) if got.size else 0.0
        if key is not None and math.isfinite(worst):
            OBSERVED_ULP[key] = max(OBSERVED_ULP.get(key, 0.0), worst)
        ok &= err <= gate
        if not ok.all():
            bad = np.flatnonzero(~ok)
            self._fail(label, "%d of %d outside %g ulp, max err %.4g ulp, first bad index %d (got %r, expected %r)"
                       % (bad.size, got.size, gate, worst, bad[0], got[bad[0]], ref_r[bad[0]]))

    def raises(self, label, fn):
        self.checks += 1
        try:
            fn()
        except _lib.TnnError:
            return
        self._fail(label, "did not raise")

    def finish(self):
        _dump_observed()
        da.trim_cache()
        assert self.checks > 0, "%s/%s ran no check" % (self.family, self.dtype)
        assert not self.fails, "%d of %d checks failed:\n%s" % (len(self.fails), self.checks, "\n".join(self.fails))


def _dump_observed():
    """TNN_SWEEP_ULP_OUT=<file>: the observed maxima of this process, rewritten after every family (the source of
    profiles/kernel_sweep_ulp.txt)."""
    path = os.environ.get("TNN_SWEEP_ULP_OUT")
    if not path:
        return
    with open(path, "w") as f:
        f.write("# backend %s\n# op dtype observed_max_ulp gate\n" % _lib.backend_name())
        for (op, dt), v in sorted(OBSERVED_ULP.items()):
            f.write("%s %s %.4f %d\n" % (op, dt, v, ULP_GATES[(op, dt)]))


# ---------------------------------------------------------------------------------------------------------- inputs
def specials(dt):
    fi = np.finfo(dt)
    return np.array([0.0, -0.0, np.inf, -np.inf, np.nan, fi.max, -fi.max, fi.tiny, -fi.tiny, fi.smallest_subnormal,
                     -fi.smallest_subnormal, fi.tiny / 4, 1.0, -1.0, 0.5, 3.0], dtype=dt)


def mixed(rs, n, dt, with_specials=True, scale=1.0):
    """n random values with the special values (signed zeros, infinities, NaN, extremes, denormals) sprinkled in."""
    x = (rs.standard_normal(n) * scale).astype(dt)
    if with_specials and n:
        sp = specials(dt)
        k = min(n, sp.size) if n < 64 else sp.size
        pos = rs.permutation(n)[:k]
        x[pos] = rs.permutation(sp)[:k]
    return x


def flat_sizes(dt):
    lim = device_limits()
    vec = 16 // np.dtype(dt).itemsize
    one_pass = lim["pass_scalar"] * vec                 # elements one pass of the 16-byte kernel covers
    return [1, 2, 3, 4, 5, 7, 255, 256, 257, 1023, 1025], [one_pass - 1, one_pass, one_pass + 1, 2 * one_pass + 3]


def np_ignore(fn):
    def wrapped(*a, **kw):
        with np.errstate(all="ignore"):
            return fn(*a, **kw)
    return wrapped


def _label(op, shape, offs):
    return "%s/%s/%s" % (op, "x".join(map(str, shape)) if isinstance(shape, (tuple, list)) else shape,
                         ",".join(map(str, offs)))


def run_map(rep, op, ins, offs, call, ref, mode="bits", out_dtype=None, key=None, gate=None, zero_sign=True, shape=None):
    """One launch: `ins` host arrays go up at offsets offs[:-1], the output (ref's size) at offs[-1];
    call(pointers..., out pointer); the payload is compared with `ref` and the guards are checked."""
    ref = np.asarray(ref)
    devs = [Dev(x, off=o) for x, o in zip(ins, offs)]
    out = Dev(n=ref.size, dtype=out_dtype or (ref.dtype if mode == "bits" else ins[0].dtype), off=offs[-1])
    label = _label(op, shape if shape is not None else ref.size, offs)
    try:
        call(*([d.ptr for d in devs] + [out.ptr]))
    except _lib.TnnError as exc:                 # a refused call is a failure of this case, not the end of the sweep
        rep.checks += 1
        return rep._fail(label, "raised %s" % exc)
    got, bad = out.read()
    rep.guard(label, bad)
    if mode == "bits":
        rep.bits(label, got, ref, zero_sign=zero_sign)
    else:
        rep.ulps(label, got, ref, gate, key)
    return got


# ---------------------------------------------------------------------------------------------------- family: flat
UNARY_EXACT = [("neg", _lib.NEG, np.negative), ("sqrt", _lib.SQRT, np.sqrt), ("square", _lib.SQUARE, np.square),
               ("abs", _lib.ABS, np.abs), ("recip", _lib.RECIP, lambda x: x.dtype.type(1) / x), ("copy", _lib.COPY, np.copy)]
BINARY_EXACT = [("add", _lib.ADD, np.add), ("sub", _lib.SUB, np.subtract), ("mul", _lib.MUL, np.multiply),
                ("div", _lib.DIV, np.true_divide), ("maximum", _lib.MAX, np.maximum), ("minimum", _lib.MIN, np.minimum)]


def _hi(x):
    """The reference precision of the measured class: float64 numpy."""
    return np.asarray(x, np.float64)


def libm_inputs(op, rs, n, dt):
    """Dense random inputs over the finite-result domain plus the edges of each libm operation."""
    f32 = np.dtype(dt) == np.float32
    fi = np.finfo(dt)
    den = [fi.smallest_subnormal, fi.tiny / 4, fi.tiny * 0.75]
    if op == "exp":
        top, bot = (88.7, -87.3) if f32 else (709.0, -708.0)
        x = rs.uniform(-20, 20, n)
        edges = [0.0, -0.0, 1.0, -1.0, top, top - 0.5, top + 2.0, bot, bot - 1.5, bot - 10.0, bot - 16.0, bot - 40.0,
                 np.inf, -np.inf, np.nan] + den
    elif op == "log":
        x = np.exp(rs.uniform(-30, 30, n))
        edges = [0.0, -0.0, 1.0, -1.0, -fi.tiny, fi.max, fi.tiny, np.inf, -np.inf, np.nan, 1.0 + fi.eps, 1.0 - fi.eps / 2] + den
    elif op == "tanh":
        x = rs.standard_normal(n) * 2
        edges = [0.0, -0.0, 1e-5, -1e-5, 20.0, -20.0, 0.5, 9.0, np.inf, -np.inf, np.nan] + den + [-v for v in den]
    else:                                   # sigmoid: 1 / (1 + exp(-x)) stays normal for |x| below the exp overflow
        top = 80.0 if f32 else 700.0
        x = rs.standard_normal(n) * 3
        edges = [0.0, -0.0, 20.0, -20.0, top, -top, np.inf, -np.inf, np.nan] + den
    x = x.astype(dt)
    k = min(n, len(edges))
    x[rs.permutation(n)[:k]] = np.array(edges, dt)[:k] if n < len(edges) else np.array(edges, dt)
    return x


LIBM_UNARY = [("exp", _lib.EXP, lambda x: np.exp(_hi(x))), ("log", _lib.LOG, lambda x: np.log(_hi(x))),
              ("tanh", _lib.TANH, lambda x: np.tanh(_hi(x))),
              ("sigmoid", _lib.SIGMOID, lambda x: 1.0 / (1.0 + np.exp(-_hi(x))))]


def pow_inputs(rs, n, dt):
    """bases and exponents of the general pow: positive bases with real exponents, negative bases with integer and
    with fractional exponents (NaN), zeros, 0**0, ones and infinities."""
    a = np.exp(rs.uniform(-3, 3, n))
    b = rs.uniform(-3, 3, n)
    neg = rs.rand(n) < 0.25
    a[neg] = -a[neg]
    b[neg] = rs.randint(-4, 5, neg.sum())
    edges = [(0.0, 0.0), (-0.0, 0.0), (-2.0, 0.5), (-2.0, 2.5), (-2.0, 3.0), (-2.0, -3.0), (0.0, 2.0), (-0.0, 3.0), (0.0, -1.0),
             (-0.0, -1.0), (1.0, np.nan), (np.nan, 0.0), (np.nan, 1.0), (np.inf, 2.0), (np.inf, -2.0), (-np.inf, 3.0), (2.0, np.inf),
             (0.5, np.inf), (2.0, -np.inf), (10.0, 30.0), (10.0, -30.0)]
    k = min(n, len(edges))
    pos = rs.permutation(n)[:k]
    for p, (x, y) in zip(pos, edges):
        a[p], b[p] = x, y
    return a.astype(dt), b.astype(dt)


def family_flat(dtype):
    rep = Report("flat", dtype)
    dt = np.dtype(dtype)
    code = CODE[dtype]
    L = lib()
    rs = np.random.RandomState(101)
    small, large = flat_sizes(dt)
    pow_gate, pow_key = ULP_GATES[("pow", dtype)], ("pow", dtype)

    for n in small + large:
        big = n in large
        offs3 = OFFSETS3 if not big else [(0, 0, 0), (1, 2, 3)]
        offs2 = OFFSETS2 if not big else [(0, 0), (2, 1)]
        a, b = mixed(rs, n, dt), mixed(rs, n, dt)
        shape = (ctypes.c_int64 * 1)(n)
        dense = (ctypes.c_int64 * 1)(1)
        # dense binary through tnn_ewise_binary (flat2_kernel)
        for name, op, fn in (BINARY_EXACT if not big else BINARY_EXACT[:1] + BINARY_EXACT[3:5]):
            for offs in offs3:
                run_map(rep, "binary_" + name, [a, b], offs,
                        lambda pa, pb, po, op=op: L.ewise_binary(op, pa, dense, pb, dense, po, 1, shape, code),
                        np_ignore(fn)(a, b), zero_sign=name not in ("maximum", "minimum"))
        pa_, pb_ = pow_inputs(rs, n, dt)
        for offs in offs3[:2] if big else offs3:
            run_map(rep, "binary_pow", [pa_, pb_], offs,
                    lambda pa, pb, po: L.ewise_binary(_lib.POW, pa, dense, pb, dense, po, 1, shape, code),
                    np_ignore(np.power)(_hi(pa_), _hi(pb_)), mode="ulps", key=pow_key, gate=pow_gate)
        # unary (flat1_kernel)
        for name, op, fn in (UNARY_EXACT if not big else UNARY_EXACT[:2]):
            for offs in offs2:
                run_map(rep, "unary_" + name, [a], offs, lambda pa, po, op=op: L.ewise_unary(op, pa, po, n, code),
                        np_ignore(fn)(a))
        for name, op, fn in (LIBM_UNARY if not big else LIBM_UNARY[:1]):
            x = libm_inputs(name, rs, n, dt)
            for offs in offs2:
                run_map(rep, "unary_" + name, [x], offs, lambda pa, po, op=op: L.ewise_unary(op, pa, po, n, code),
                        np_ignore(fn)(x), mode="ulps", key=(name, dtype), gate=ULP_GATES[(name, dtype)])
        # array-with-scalar, scalar on either side
        for name, op, fn in (BINARY_EXACT if not big else BINARY_EXACT[1:2]):
            for s in ((1.5, -0.75, np.nan, np.inf, 0.0) if name in ("maximum", "minimum") else (1.5, -0.75)):
                for lhs in (0, 1):
                    for offs in offs2[1:3] if not big else offs2[:1]:
                        sv = dt.type(s)
                        ref = np_ignore(fn)(np.full(n, sv, dt), a) if lhs else np_ignore(fn)(a, np.full(n, sv, dt))
                        run_map(rep, "scalar_%s_%s_%s" % (name, "lhs" if lhs else "rhs", s), [a], offs,
                                lambda pa, po, op=op, s=s, lhs=lhs: L.ewise_scalar(op, pa, float(s), lhs, po, n, code),
                                ref, zero_sign=name not in ("maximum", "minimum"))
        if not big:
            nonneg = np.abs(mixed(rs, n, dt))      # (x ** 0.5 is the square root: defined alike by both sides for x >= +0 only)
            nonneg[np.signbit(nonneg)] = 0
            for s, x, ref in ((2.0, a, np_ignore(np.square)(a)), (0.5, nonneg, np_ignore(np.sqrt)(nonneg)), (1.0, a, a.copy())):
                for offs in offs2:
                    run_map(rep, "scalar_pow_rhs_%s" % s, [x], offs,
                            lambda pa, po, s=s: L.ewise_scalar(_lib.POW, pa, s, 0, po, n, code), ref)
            for s in (3.0, -1.0, 0.0, 2.5):
                for offs in offs2[:2]:
                    run_map(rep, "scalar_pow_rhs_%s" % s, [pa_], offs,
                            lambda pa, po, s=s: L.ewise_scalar(_lib.POW, pa, s, 0, po, n, code),
                            np_ignore(np.power)(_hi(pa_), s), mode="ulps", key=pow_key, gate=pow_gate)
            for s in (2.0, -2.0):
                run_map(rep, "scalar_pow_lhs_%s" % s, [pb_], offs2[1],
                        lambda pa, po, s=s: L.ewise_scalar(_lib.POW, pa, s, 1, po, n, code),
                        np_ignore(np.power)(s, _hi(pb_)), mode="ulps", key=pow_key, gate=pow_gate)
        # clip / clip_bwd: all four bound combinations, values exactly on the bounds
        lo, hi = -0.5, 0.75
        x = a.copy()
        if n >= 2:
            x[0], x[n - 1] = lo, hi
        for has_lo, has_hi in (itertools.product((0, 1), (0, 1)) if not big else [(1, 1)]):
            ref = x.copy()
            with np.errstate(all="ignore"):
                if has_lo:
                    ref[x < lo] = lo
                if has_hi:
                    ref[ref > hi] = hi
                keep = (np.ones(n, bool) if not has_lo else x >= lo) & (np.ones(n, bool) if not has_hi else x <= hi)
            for offs in offs2[:3] if not big else offs2[:1]:
                run_map(rep, "clip_%d%d" % (has_lo, has_hi), [x], offs,
                        lambda pa, po: L.clip(pa, has_lo, lo, has_hi, hi, po, n, code), ref)
            for offs in offs3[:4] if not big else offs3[:1]:
                run_map(rep, "clip_bwd_%d%d" % (has_lo, has_hi), [b, x], offs,
                        lambda pg, px, po: L.clip_bwd(pg, px, has_lo, lo, has_hi, hi, po, n, code),
                        np.where(keep, b, dt.type(0)))
        # masks
        y = a.copy()
        if n >= 4:
            y[:4] = np.array([0.0, -0.0, -np.nan, -2.0], dt)
            y[2] = np.copysign(np.nan, -1.0)
        msk = (rs.rand(n) < 0.5).astype(np.uint8)
        for offs in offs3 if not big else offs3[-1:]:
            run_map(rep, "mul_signmask", [b, y], offs, lambda pg, py, po: L.mul_signmask(pg, py, po, n, code),
                    np.where(np.signbit(y), dt.type(0), b))
            run_map(rep, "mul_mask", [b, msk], offs, lambda pg, pm, po: L.mul_mask(pg, pm, po, n, code),
                    np.where(msk != 0, b, dt.type(0)))
        # axpy (in place): float64 (longdouble for f64) arithmetic rounded once.  The kernel may round alpha * x before it
        # adds (two roundings) or contract to an FMA (one): half an ulp of the product plus half an ulp of the sum, i.e.
        # 1 ulp at the larger of the two magnitudes.
        ya = mixed(rs, n, dt)
        xa = mixed(rs, n, dt)
        for v in (ya, xa):
            v[np.abs(v) == np.finfo(dt).max] = 2.0         # (no overflow edge: an FMA and two roundings may part there)
        alpha = -0.37109375
        hi_t = np.float64 if dt == np.float32 else np.longdouble
        with np.errstate(all="ignore"):
            ref_hi = ya.astype(hi_t) + hi_t(alpha) * xa.astype(hi_t)
        for offs in offs2 if not big else offs2[-1:]:
            dy, dx = Dev(ya, off=offs[0]), Dev(xa, off=offs[1])
            L.axpy(dy.ptr, alpha, dx.ptr, n, code)
            got, bad = dy.read()
            rep.guard(_label("axpy", n, offs), bad)
            rep.ulps(_label("axpy", n, offs), got, ref_hi, 1.0, at=np_ignore(np.multiply)(dt.type(alpha), xa))
    rep.finish()


def family_fill(dtype):
    rep = Report("fill", dtype)
    dt = np.dtype(dtype)
    lim = device_limits()
    for n in [1, 2, 3, 5, 255, 257, 1025, lim["pass_scalar"] + 1, 2 * lim["pass_scalar"] + 3]:
        for value in (0.0, 1.0) + ((-7.0, 2.5) if dt.kind == "f" else (-7.0, 3.0) if dt.kind == "i" else (2.0,)):
            for off in (0, 1, 3):
                out = Dev(n=n, dtype=dt, off=off)
                lib().fill(out.ptr, float(value), n, CODE[dtype])
                got, bad = out.read()
                label = _label("fill_%s" % value, n, (off,))
                rep.guard(label, bad)
                rep.bits(label, got, np.full(n, (value != 0) if dt == np.uint8 else value).astype(dt))
    rep.finish()


# ------------------------------------------------------------------------------------------------- family: strided
COMPARES = [("gt", _lib.GT, np.greater), ("ge", _lib.GE, np.greater_equal), ("lt", _lib.LT, np.less),
            ("le", _lib.LE, np.less_equal), ("eq", _lib.EQ, np.equal), ("ne", _lib.NE, np.not_equal)]


def _elem_strides(view):
    return [s // view.dtype.itemsize for s in view.strides]


def strided_shapes():
    lim = device_limits()
    over_gx = lim["block_cap"] * 256 + 5                      # more columns than the capped grid.x covers in one step
    small = [((7, 9), (1, 9)), ((7, 9), (7, 1)), ((7, 9), (1, 1)), ((7, 1), (1, 9)), ((1, 300), (5, 1)), ((300, 7), (300, 7)),
             # 3- to 6-D that do not collapse, size-1 axes in every position
             ((3, 1, 5), (1, 4, 5)), ((1, 4, 5), (3, 1, 5)), ((3, 4, 1), (1, 4, 5)), ((3, 1, 5, 6), (1, 4, 5, 1)),
             ((1, 4, 1, 6), (3, 1, 5, 1)), ((2, 3, 1, 4, 5), (1, 3, 6, 1, 5)), ((1, 3, 2, 1, 5), (2, 1, 2, 4, 1)),
             ((2, 1, 3, 1, 4, 3), (1, 5, 3, 2, 1, 3)), ((1, 2, 1, 3, 1, 4), (3, 1, 2, 1, 5, 1)),
             # shapes that collapse to 1-D / 2-D
             ((2, 3, 4, 5), (2, 3, 4, 5)), ((4, 5, 6), (1, 1, 6)), ((4, 5, 6), (4, 1, 1)), ((4, 5, 6), (1, 1, 1)), ((1, 1, 37), (1, 1, 37)),
             ((2, 3, 4, 5, 2, 3), (2, 3, 4, 5, 2, 3)), ((6, 1, 5), (4, 1)),
             # zero-size
             ((0, 5), (1, 5)), ((3, 0, 4), (3, 1, 4)), ((0,), (0,))]
    large = [((1, 3), (1, 3)), ((65535, 3), (1, 3)), ((65536, 3), (65536, 1)), ((70001, 3), (1, 3)), ((70001, 1), (1, 3)),
             ((2, over_gx), (2, 1)), ((2, over_gx), (1, over_gx))]
    return small, large


def family_strided(dtype):
    rep = Report("strided", dtype)
    dt = np.dtype(dtype)
    code = CODE[dtype]
    L = lib()
    rs = np.random.RandomState(202)
    small, large = strided_shapes()

    def one(name, fn, sa, sb, a, b, av, bv, offs, call, out_dtype, zero_sign=True, a_at=0, b_at=0):
        shape = np.broadcast_shapes(av.shape, bv.shape)
        nd = len(shape)
        cs = (ctypes.c_int64 * max(nd, 1))(*shape)
        st_a = (ctypes.c_int64 * max(nd, 1))(*_elem_strides(np.broadcast_to(av, shape)))
        st_b = (ctypes.c_int64 * max(nd, 1))(*_elem_strides(np.broadcast_to(bv, shape)))
        ref = np_ignore(fn)(av, bv)
        da_, db_ = Dev(a, off=offs[0]), Dev(b, off=offs[1])
        out = Dev(n=ref.size, dtype=out_dtype, off=offs[2])
        call(da_.at(a_at) if a.size else da_.ptr, st_a, db_.at(b_at) if b.size else db_.ptr, st_b, out.ptr, nd, cs)
        got, bad = out.read()
        label = _label(name, "%s_%s" % ("x".join(map(str, sa)), "x".join(map(str, sb))), offs)
        rep.guard(label, bad)
        rep.bits(label, got, ref.astype(out_dtype), zero_sign=zero_sign)

    for group, shapes in (("small", small), ("large", large)):
        for sa, sb in shapes:
            a = mixed(rs, int(np.prod(sa)), dt).reshape(sa)
            b = mixed(rs, int(np.prod(sb)), dt).reshape(sb)
            if a.size and b.size and a.shape == b.shape:
                b.flat[::3] = a.flat[::3]                         # equal elements for eq / ne / ge / le
            ops = BINARY_EXACT if group == "small" else [BINARY_EXACT[0], BINARY_EXACT[4]]
            cmps = COMPARES if group == "small" else COMPARES[1:2]
            offsets = [(0, 0, 0), (1, 2, 3)] if group == "small" else [(0, 1, 0)]
            for offs in offsets:
                for name, op, fn in ops:
                    one("binary_" + name, fn, sa, sb, a, b, a, b, offs,
                        lambda pa, s1, pb, s2, po, nd, cs, op=op: L.ewise_binary(op, pa, s1, pb, s2, po, nd, cs, code), dt,
                        zero_sign=name not in ("maximum", "minimum"))
                for name, op, fn in cmps:
                    one("compare_" + name, fn, sa, sb, a, b, a, b, offs,
                        lambda pa, s1, pb, s2, po, nd, cs, op=op: L.ewise_compare(op, pa, s1, pb, s2, po, nd, cs, code), np.uint8)
    # stepped (non-dense, non-broadcast) views of larger operands
    a = mixed(rs, 12 * 20, dt).reshape(12, 20)
    b = mixed(rs, 6 * 7 * 3, dt).reshape(6, 7, 3)
    av, bv = a[1::2, 2:16:2], b[:, :, 1]
    one("binary_sub_stepped", np.subtract, av.shape, bv.shape, a, b, av, bv, (1, 0, 2),
        lambda pa, s1, pb, s2, po, nd, cs: L.ewise_binary(_lib.SUB, pa, s1, pb, s2, po, nd, cs, code), dt, a_at=22, b_at=1)
    one("compare_lt_stepped", np.less, av.shape, bv.shape, a, b, av, bv, (0, 3, 1),
        lambda pa, s1, pb, s2, po, nd, cs: L.ewise_compare(_lib.LT, pa, s1, pb, s2, po, nd, cs, code), np.uint8, a_at=22, b_at=1)
    # a 7-D shape is refused
    seven = (ctypes.c_int64 * 7)(*([2] * 7))
    st7 = (ctypes.c_int64 * 7)(*[2 ** (6 - k) for k in range(7)])
    x7 = Dev(mixed(rs, 128, dt))
    o7 = Dev(n=128, dtype=dt)
    rep.raises("binary_add/7-D", lambda: L.ewise_binary(_lib.ADD, x7.ptr, st7, x7.ptr, st7, o7.ptr, 7, seven, code))
    rep.raises("compare_gt/7-D", lambda: L.ewise_compare(_lib.GT, x7.ptr, st7, x7.ptr, st7, o7.ptr, 7, seven, code))
    rep.guard("7-D", o7.read()[1])
    # compare with a scalar (map_kernel)
    lim = device_limits()
    for n in (1, 3, 257, 1025, lim["pass_scalar"] + 1, 2 * lim["pass_scalar"] + 3):
        x = mixed(rs, n, dt)
        x[::5] = 0.25
        for name, op, fn in (COMPARES if n < 10000 else COMPARES[:1]):
            for s in (0.25, np.nan) if n < 10000 else (0.25,):
                for offs in ((0, 0), (1, 3)):
                    run_map(rep, "compare_scalar_%s_%s" % (name, s), [x], offs,
                            lambda pa, po, op=op, s=s: L.compare_scalar(op, pa, float(s), po, n, code),
                            np_ignore(fn)(x, dt.type(s)).astype(np.uint8), out_dtype=np.uint8)
    rep.finish()


# ---------------------------------------------------------------------------------------------- family: reductions
def reduce_cases(dt):
    """(outer, red, inner) — every threshold of reduce_typed once with small partners, plus the combinations that
    select another kernel form; anything above the buffer limit is dropped."""
    lim = device_limits()
    cap = lim["block_cap"]
    cases = []
    reds, outers = [1, 63, 64, 65, 8191, 8192], [1, 2, 63, 64, 65, 5000]
    for red in reds:
        cases += [(o, red, 1) for o in (1, 2, 64)]
    for outer in outers:
        cases += [(outer, r, 1) for r in (1, 63, 64)]
    cases += [(63, 8191, 1), (63, 8192, 1), (65, 8192, 1), (5000, 65, 1)]
    very_long = 1024 * 256 * 16 + 4096 + 7                 # row_split: more 4096-element pieces than the 1024 blocks it may use
    cases += [(1, very_long, 1), (2, very_long, 1)]
    # inner > 1
    reds, inners = [1, 255, 256, 257, 5000], [2, 63, 64, 65, 1000]
    for red in reds:
        cases += [(1, red, 65), (5, red, 2)]
    for inner in inners:
        cases += [(1, 257, inner), (5, 255, inner), (5, 5000, inner)]
    for inner in (2, 65):
        strips = (inner + 63) // 64
        thr = (cap // 4 + strips - 1) // strips                # first outer with strips * outer >= block_cap / 4: not sliced
        cases += [(thr - 1, 256, inner), (thr, 256, inner), (thr - 1, 5000, inner), (thr, 257, inner)]
    cases += [(65535, 1, 2), (65536, 5, 12), (70000, 4, 3), (70000, 1, 64), (65536, 255, 2), (65535, 257, 2)]
    out, seen = [], set()
    for c in cases:
        if c not in seen and c[0] * c[1] * c[2] * np.dtype(dt).itemsize <= BUFFER_LIMIT:
            seen.add(c)
            out.append(c)
    return out


def cancelling(rs, outer, red, inner, dt):
    """Values of magnitude 1e4 paired with their negatives and shuffled along the reduced axis, plus a small remainder:
    the exact sum is tiny next to sum(|x|), which a float32 accumulator cannot deliver."""
    half = red // 2
    h = 1e4 * (1.0 + rs.rand(half))
    v = np.concatenate([h, -h, rs.standard_normal(red - 2 * half) * 1e-3])
    v = v[rs.permutation(red)].astype(dt)                 # rounded once, so each pair still cancels exactly
    scale = np.exp2(rs.randint(-2, 3, (outer, 1, inner))).astype(dt)      # powers of two: exact
    return np.ascontiguousarray(v[None, :, None] * scale)


def family_reduce(dtype):
    rep = Report("reduce", dtype)
    dt = np.dtype(dtype)
    code = CODE[dtype]
    L = lib()
    rs = np.random.RandomState(303)
    eps52 = 2.0 ** -52
    for outer, red, inner in reduce_cases(dt):
        x = cancelling(rs, outer, red, inner, dt)
        shape = "%dx%dx%d" % (outer, red, inner)
        dx = Dev(x)
        # sum: float64 accumulation in any order, rounded once
        S = np.sum(x, axis=1, dtype=np.longdouble)
        absS = np.sum(np.abs(x), axis=1, dtype=np.longdouble)
        runs = []
        for rep_i in range(2):
            out = Dev(n=outer * inner, dtype=dt, off=rep_i)
            try:
                L.reduce(_lib.RSUM, dx.ptr, out.ptr, outer, red, inner, code)
            except _lib.TnnError as exc:
                rep.checks += 1
                rep._fail(_label("sum", shape, (0, rep_i)), "raised %s" % exc)
            got, bad = out.read()
            rep.guard(_label("sum", shape, (0, rep_i)), bad)
            runs.append(got)
        rep.checks += 1
        got = runs[0].reshape(outer, inner)
        allowed = red * eps52 * absS + np.spacing(np.abs(S).astype(dt)).astype(np.longdouble)
        err = np.abs(got.astype(np.longdouble) - S)
        if not (err <= allowed).all():
            bad = np.flatnonzero(~(err <= allowed).ravel())
            rep._fail(_label("sum", shape, (0, 0)), "%d of %d outside the bound, max err %.6g (allowed there %.6g), first bad index %d"
                      % (bad.size, err.size, float(err.max()), float(allowed.ravel()[np.argmax(err)]), bad[0]))
        rep.checks += 1
        if not np.array_equal(_bits(runs[0]), _bits(runs[1])):
            rep._fail(_label("sum", shape, (0, 0)), "two runs differ in %d elements (not deterministic)"
                      % int((_bits(runs[0]) != _bits(runs[1])).sum()))
        # max / min: exact; then with one NaN at the start, in the middle and at the end of the reduced axis
        for name, rop, fn in (("max", _lib.RMAX, np.max), ("min", _lib.RMIN, np.min)):
            run_map(rep, name, [], (1,), lambda po, rop=rop: L.reduce(rop, dx.ptr, po, outer, red, inner, code),
                    fn(x, axis=1), shape=shape, zero_sign=False)
        xn = x.copy()
        o0, i0 = outer // 2, inner // 2
        for k, pos in enumerate(sorted(set([0, red // 2, red - 1]))):
            oo, ii = (o0 + k) % outer, (i0 + k) % inner
            xn[oo, pos, ii] = np.nan
        if inner > 1 or outer > 1:
            xn[0, :, 0] = x[0, :, 0]
            xn[0, red - 1, 0] = np.inf if red > 1 else x[0, 0, 0]
        dn = Dev(xn)
        for name, rop, fn in (("max_nan", _lib.RMAX, np.max), ("min_nan", _lib.RMIN, np.min)):
            run_map(rep, name, [], (0,), np_ignore(lambda po, rop=rop: L.reduce(rop, dn.ptr, po, outer, red, inner, code)),
                    np_ignore(fn)(xn, axis=1), shape=shape, zero_sign=False)
        del x, xn, dx, dn
    # signed zeros, infinities and extremes through max / min
    for outer, red, inner in [(3, 40, 1), (3, 200, 1), (2, 9000, 1), (3, 300, 5)]:
        x = mixed(rs, outer * red * inner, dt).reshape(outer, red, inner)
        x[np.isnan(x)] = 0.5
        dx = Dev(x)
        for name, rop, fn in (("max_specials", _lib.RMAX, np.max), ("min_specials", _lib.RMIN, np.min)):
            run_map(rep, name, [], (2,), lambda po, rop=rop: L.reduce(rop, dx.ptr, po, outer, red, inner, code),
                    fn(x, axis=1), shape="%dx%dx%d" % (outer, red, inner), zero_sign=False)
    # an empty reduced axis: the sum is 0
    unread = Dev(n=4, dtype=dt)
    run_map(rep, "sum_empty", [], (1,), lambda po: L.reduce(_lib.RSUM, unread.ptr, po, 3, 0, 2, code),
            np.zeros(6, dt), shape="3x0x2")
    # the host grouping of DeviceArray.sum / max / min: non-adjacent axes, keepdims, outer above the grid's y extent
    for shp, axes in [((7, 5, 9), [None, 0, 1, 2, -1, (0, 1), (1, 2), (0, 2), (0, 1, 2)]), ((70000, 4, 3), [1, (0, 2)]),
                      ((3, 4, 5, 6), [(0, 2), (1, 3), (0, 3)])]:
        x = cancelling(rs, 1, int(np.prod(shp)), 1, dt).reshape(shp)
        X = da.asarray(x, dtype=dt)
        for axis in axes:
            for keep in (False, True):
                label = "host/%s/axis=%s,keepdims=%s" % ("x".join(map(str, shp)), axis, keep)
                n_red = x.size // max(1, np.sum(x, axis=axis).size)
                S = np.sum(x, axis=axis, keepdims=keep, dtype=np.longdouble)
                absS = np.sum(np.abs(x), axis=axis, keepdims=keep, dtype=np.longdouble)
                try:
                    got = np.asarray(X.sum(axis=axis, keepdims=keep))
                    gmax, gmin = np.asarray(X.max(axis=axis, keepdims=keep)), np.asarray(X.min(axis=axis, keepdims=keep))
                except _lib.TnnError as exc:
                    rep.checks += 1
                    rep._fail(label, "raised %s" % exc)
                    continue
                rep.checks += 1
                allowed = n_red * eps52 * absS + np.spacing(np.abs(S).astype(dt)).astype(np.longdouble)
                if isinstance(axis, tuple) and tuple(axis) != tuple(range(axis[0], axis[0] + len(axis))):
                    # non-adjacent axes are reduced one after the other: every partial sum (fewer than n_red of them, none
                    # above sum|x|) is rounded to the dtype before the next pass adds it
                    allowed = allowed + n_red * np.spacing(absS.astype(dt)).astype(np.longdouble)
                if got.shape != S.shape or got.dtype != dt:
                    rep._fail(label, "shape %s dtype %s, expected %s %s" % (got.shape, got.dtype, S.shape, dt))
                elif not (np.abs(got.astype(np.longdouble) - S) <= allowed).all():
                    err = np.abs(got.astype(np.longdouble) - S)
                    rep._fail(label, "sum: max err %.6g, first bad index %d" % (float(err.max()), np.flatnonzero(~(err <= allowed).ravel())[0]))
                rep.bits(label + "/max", gmax, np.max(x, axis=axis, keepdims=keep), zero_sign=False)
                rep.bits(label + "/min", gmin, np.min(x, axis=axis, keepdims=keep), zero_sign=False)
    rep.finish()


# -------------------------------------------------------------------------------------------------- family: argmax
def family_argmax(dtype):
    rep = Report("argmax", dtype)
    dt = np.dtype(dtype)
    code = CODE[dtype]
    L = lib()
    rs = np.random.RandomState(404)
    lim = device_limits()
    many_rows = lim["block_cap"] * 4 + 3                    # more rows than the capped grid has waves

    def run(name, x, off=0):
        rows, cols = x.shape
        dx = Dev(x, off=off)
        run_map(rep, name, [], (off,), lambda po: L.argmax_rows(dx.ptr, po, rows, cols, code),
                np_ignore(np.argmax)(x, axis=1).astype(np.int64), shape="%dx%d" % (rows, cols), out_dtype=np.int64)

    for cols in (1, 2, 63, 64, 65, 129, 100000):
        for rows in (1, 5):
            run("random", rs.standard_normal((rows, cols)).astype(dt), off=rows % 4)
        # ties, -inf rows and NaN, one row per pattern
        pats = []
        for k in sorted(set(k for k in (0, 1, cols // 2, max(cols - 65, 0), cols - 1) if k < cols)):
            base = rs.standard_normal(cols).astype(dt)
            base[np.argmax(base)] = 0
            for k2 in (k + 64, k + 1, cols - 1):
                if k2 < cols:
                    r = np.minimum(base, dt.type(2.0))
                    r[k], r[k2] = 5.0, 5.0                    # equal maxima: the first wins
                    pats.append(r)
            for nan_at in ([k], [k, cols - 1], [cols - 1, k]):
                r = base.copy()
                r[min(cols - 1, 3)] = np.inf
                r[nan_at] = np.nan                               # the first NaN wins over everything
                pats.append(r)
        k63 = min(63, cols - 1)
        r = np.full(cols, -1.0, dt); r[k63] = 7.0; pats.append(r.copy())
        if cols > 64:
            r[64] = 7.0; pats.append(r.copy())                   # k and k+1 across the 64-lane boundary
        pats.append(np.full(cols, -np.inf, dt))
        r = np.full(cols, -np.inf, dt); r[cols - 1] = -np.finfo(dt).max; pats.append(r)
        r = np.full(cols, np.nan, dt); pats.append(r)
        pats.append(np.zeros(cols, dt))
        run("patterns", np.stack(pats), off=1)
    run("many_rows", rs.standard_normal((many_rows, 65)).astype(dt))
    run("many_rows_short", rs.randint(0, 3, (many_rows, 5)).astype(dt), off=2)
    # np.argmax on every axis through the host (transposes for axes other than the last)
    x = rs.randint(-3, 4, (6, 70, 5)).astype(dt)
    x[2, 5, 1] = np.nan
    X = da.asarray(x, dtype=dt)
    for axis in (None, 0, 1, 2, -1):
        rep.bits("host/6x70x5/axis=%s" % axis, np.asarray(np.argmax(X, axis=axis)).astype(np.int64),
                 np.asarray(np.argmax(x, axis=axis)).astype(np.int64))
    rep.finish()


# ------------------------------------------------------------------------------------ family: strided copy / scatter
def any_values(rs, n, dtype):
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return mixed(rs, n, dt)
    if dt == np.uint8:
        return rs.randint(0, 2, n).astype(dt)
    return rs.randint(-2 ** 62, 2 ** 62, n).astype(dt)


def family_copy(dtype):
    rep = Report("copy", dtype)
    dt = np.dtype(dtype)
    code = CODE[dtype]
    L = lib()
    rs = np.random.RandomState(505)

    def gather(name, base, view, start, offs):
        """out (dense, view's shape) = base read through view's strides"""
        nd = view.ndim
        cs = (ctypes.c_int64 * max(nd, 1))(*view.shape)
        st = (ctypes.c_int64 * max(nd, 1))(*_elem_strides(view))
        src = Dev(base, off=offs[0])
        run_map(rep, name, [], (offs[1],),
                lambda po: L.strided_copy(src.at(start) if base.size else src.ptr, st, po, nd, cs, code),
                np.ascontiguousarray(view), shape="x".join(map(str, view.shape)))

    def scatter(name, base, view, start, offs):
        """dest through view's strides = dense values; everything the view does not address keeps its contents"""
        nd = view.ndim
        cs = (ctypes.c_int64 * max(nd, 1))(*view.shape)
        st = (ctypes.c_int64 * max(nd, 1))(*_elem_strides(view))
        vals = any_values(rs, view.size, dt).reshape(view.shape)
        expect = base.copy()
        ev = np.lib.stride_tricks.as_strided(expect.ravel()[start:], view.shape, view.strides) if view.size else None
        if ev is not None:
            ev[...] = vals
        src, dst = Dev(vals, off=offs[0]), Dev(base, off=offs[1])
        L.strided_scatter(src.ptr, dst.at(start) if base.size else dst.ptr, st, nd, cs, code)
        got, bad = dst.read()
        label = _label(name, "x".join(map(str, view.shape)), offs)
        rep.guard(label, bad)
        rep.bits(label, got, expect.ravel())

    sizes = (1, 63, 64, 65, 129, 1000)
    for R, C in itertools.product(sizes, sizes):
        x = any_values(rs, R * C, dt).reshape(R, C)
        gather("transpose", x, x.T, 0, (0, 0) if (R + C) % 2 else (1, 3))
        if R in (1, 65, 1000) and C in (63, 64, 129):
            scatter("scatter_transpose", x, x.T, 0, (2, 1))
    R = 64 * 65536                                               # grid.y of the tiled transpose would pass 65535
    x = any_values(rs, R * 2, dt).reshape(R, 2)
    gather("transpose_tall", x, x.T, 0, (0, 0))
    x = any_values(rs, 3 * 4 * 5 * 6, dt).reshape(3, 4, 5, 6)
    for perm in itertools.permutations(range(4)):
        gather("permute%s" % "".join(map(str, perm)), x, x.transpose(perm), 0, (0, 1))
        scatter("scatter_permute%s" % "".join(map(str, perm)), x, x.transpose(perm), 0, (1, 0))
    x6 = any_values(rs, 2 * 3 * 4 * 2 * 3 * 5, dt).reshape(2, 3, 4, 2, 3, 5)
    gather("permute6", x6, x6.transpose(5, 0, 3, 1, 4, 2), 0, (0, 0))
    scatter("scatter_permute6", x6, x6.transpose(5, 0, 3, 1, 4, 2), 0, (0, 2))
    row = any_values(rs, 7, dt).reshape(1, 7)
    gather("broadcast_rows", row, np.broadcast_to(row, (5, 7)), 0, (1, 0))
    col = any_values(rs, 6, dt).reshape(6, 1)
    gather("broadcast_cols", col, np.broadcast_to(col, (6, 300)), 0, (0, 1))
    gather("broadcast_3d", col, np.broadcast_to(col.reshape(1, 6, 1), (4, 6, 5)), 0, (0, 0))
    m = any_values(rs, 40 * 31, dt).reshape(40, 31)
    for name, view, start in (("step_rows", m[::2], 0), ("step_both", m[1::3, 2::5], 33), ("window", m[5:9, 7:20], 5 * 31 + 7),
                              ("column", m[:, 4], 4), ("step_T", m[::4, 1::2].T, 1)):
        gather(name, m, view, start, (0, 3))
        scatter("scatter_" + name, m, view, start, (3, 0))
    c3 = any_values(rs, 9 * 8 * 7, dt).reshape(9, 8, 7)
    gather("step_3d", c3, c3[1::2, :, ::3], 56, (1, 1))
    scatter("scatter_step_3d", c3, c3[1::2, :, ::3], 56, (0, 0))
    gather("dense", c3, c3, 0, (1, 2))
    gather("zero_size", c3, c3[:0], 0, (0, 0))
    seven = (ctypes.c_int64 * 7)(*([2] * 7))
    st7 = (ctypes.c_int64 * 7)(*[2 ** (6 - k) for k in range(7)])
    x7, o7 = Dev(any_values(rs, 128, dt)), Dev(n=128, dtype=dt)
    rep.raises("strided_copy/7-D", lambda: L.strided_copy(x7.ptr, st7, o7.ptr, 7, seven, code))
    rep.raises("strided_scatter/7-D", lambda: L.strided_scatter(x7.ptr, o7.ptr, st7, 7, seven, code))
    rep.finish()


# -------------------------------------------------------------------------------------- family: row gather / scatter
def family_rows(dtype):
    rep = Report("rows", dtype)
    dt = np.dtype(dtype)
    code = CODE[dtype]
    L = lib()
    rs = np.random.RandomState(606)
    row_bytes = [4, 12, 16, 20, 24, 3136]
    row_elems = sorted(set(b // dt.itemsize for b in row_bytes if b % dt.itemsize == 0)) + [64 * 256 + 5, 64 * 256 + 16]

    def gather(src_rows, re, idx, offs):
        src = any_values(rs, src_rows * re, dt).reshape(src_rows, re)
        dsrc, didx = Dev(src, off=offs[0]), Dev(idx)
        run_map(rep, "gather", [], (offs[1],),
                lambda po: L.gather_rows(dsrc.ptr, didx.ptr, po, idx.size, re, src_rows, code), src[idx],
                shape="%dx%d_from_%d" % (idx.size, re, src_rows))

    def scatter(dst_rows, re, idx, offs):
        vals = any_values(rs, idx.size * re, dt).reshape(idx.size, re)
        old = any_values(rs, dst_rows * re, dt).reshape(dst_rows, re)
        expect = old.copy()
        expect[idx] = vals
        dsrc, didx, ddst = Dev(vals, off=offs[0]), Dev(idx), Dev(old, off=offs[1])
        L.scatter_rows(dsrc.ptr, didx.ptr, ddst.ptr, idx.size, re, dst_rows, code)
        got, bad = ddst.read()
        label = _label("scatter", "%dx%d_into_%d" % (idx.size, re, dst_rows), offs)
        rep.guard(label, bad)
        rep.bits(label, got, expect.ravel())                     # rows that no index names keep their contents

    for re in row_elems:
        idx = np.concatenate([rs.randint(-37, 37, 46), [0, 36, -1, -37]]).astype(np.int64)     # negative and duplicate
        uniq = rs.permutation(37)[:20].astype(np.int64)
        uniq[::3] -= 37                                           # negative, still unique
        for offs in ((0, 0), (1, 0), (0, 1), (3, 2)):
            gather(37, re, idx, offs)
            scatter(37, re, uniq, offs)
    for n_idx in (1, 65535, 65536, 70001):
        for re in sorted(set([max(1, 12 // dt.itemsize), 16 // dt.itemsize if dt.itemsize <= 16 else 1, 32 // dt.itemsize])):
            rows = n_idx + 5
            gather(97, re, rs.randint(-97, 97, n_idx).astype(np.int64), (0, 0))
            gather(97, re, rs.randint(-97, 97, n_idx).astype(np.int64), (1, 0))
            u = rs.permutation(rows)[:n_idx].astype(np.int64)
            u[::2] -= rows
            scatter(rows, re, u, (0, 0))
    # out-of-range indices never reach the device: the host layer refuses them
    X = da.asarray(any_values(rs, 10 * 3, dt).reshape(10, 3), dtype=np.bool_ if dt == np.uint8 else dt)
    for bad_idx in (np.array([0, 10]), np.array([-11, 2])):
        rep.checks += 1
        try:
            X[bad_idx]
        except IndexError:
            pass
        else:
            rep._fail("host/getitem/%s" % bad_idx.tolist(), "an out-of-range row index did not raise IndexError")
    rep.finish()


# ------------------------------------------------------------------------------------------- family: cast / one_hot
def cast_inputs(rs, n, src, dst):
    src, dst = np.dtype(src), np.dtype(dst)
    if src.kind == "f":
        if dst == np.int64:                                     # finite and inside the int64 range: nothing else is defined
            x = (rs.standard_normal(n) * 1000).astype(src)
            edges = [-0.5, -1.5, -2.9, 2.9, 0.5, -0.0, 0.0, -1e-30, 1e-30, 2.0 ** 53 + 2, -2.0 ** 62, 2.0 ** 62, 16777217.0, -0.99999]
        else:
            x = mixed(rs, n, src)
            edges = [1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, 1 + 2.0 ** -24 + 2.0 ** -50, 1 - 2.0 ** -25, 1e39, -1e39,
                     3.4028235677973366e38, 3.4028235e38, 1e-46, 7.1e-46, 2.0 ** -150, -2.0 ** -149 * 1.5, np.nan, -0.0,
                     5e-324, 1e-310]
        with np.errstate(all="ignore"):
            edges = np.array(edges, np.float64).astype(src)
    elif src == np.int64:
        x = rs.randint(-2 ** 62, 2 ** 62, n).astype(src)
        x[::2] = rs.randint(-1000, 1000, x[::2].size)
        edges = np.array([2 ** 24 + 1, 2 ** 24 + 3, -(2 ** 24 + 1), 2 ** 53 + 1, 2 ** 53 + 3, 2 ** 53 + 2 ** 29 + 1, -(2 ** 53 + 2 ** 29 + 1),
                          2 ** 62 + 2 ** 38 + 1, 2 ** 63 - 1, -2 ** 63, 2 ** 63 - 2 ** 39 - 1, 0, -1, 1, 2 ** 40 + 2 ** 15, 2 ** 40 + 2 ** 16 + 1],
                         np.int64)
    else:
        return rs.randint(0, 2, n).astype(src)
    k = min(n, edges.size)
    x[rs.permutation(n)[:k]] = edges[:k] if n < edges.size else edges
    return x


def family_cast(dtype):
    """`dtype` is the source type; every target type."""
    rep = Report("cast", dtype)
    rs = np.random.RandomState(707)
    L = lib()
    lim = device_limits()
    for dst in ALL_DTYPES:
        for n in (1, 2, 3, 5, 257, 1025, lim["pass_scalar"] + 3):
            x = cast_inputs(rs, n, dtype, dst)
            with np.errstate(all="ignore"):
                ref = (x != 0).astype(np.uint8) if dst == "uint8" else x.astype(dst)
            for offs in ((0, 0), (1, 3)):
                run_map(rep, "to_%s" % dst, [x], offs, lambda pa, po: L.cast(pa, CODE[dtype], po, CODE[dst], n), ref)
    rep.finish()


def family_one_hot(dtype):
    rep = Report("one_hot", dtype)
    dt = np.dtype(dtype)
    rs = np.random.RandomState(808)
    L = lib()
    lim = device_limits()
    for classes in (1, 10, 1000):
        for n in (1, 7, 300, lim["pass_scalar"] // 1000 + 13):
            labels = rs.randint(0, classes, n).astype(np.int64)
            labels[0], labels[-1] = classes - 1, 0
            for offs in ((0, 0), (1, 3)):
                run_map(rep, "classes%d" % classes, [labels], offs, lambda pl, po: L.one_hot(pl, po, n, classes, CODE[dtype]),
                        np.eye(classes, dtype=dt)[labels], shape="%dx%d" % (n, classes))
    rep.finish()


# ------------------------------------------------------------------------------------------------ family: bias_act
def family_bias_act(dtype):
    rep = Report("bias_act", dtype)
    dt = np.dtype(dtype)
    rs = np.random.RandomState(909)
    L = lib()
    hi_t = np.float64 if dt == np.float32 else np.longdouble
    lim = device_limits()
    shapes = list(itertools.product((1, 7, 128), (1, 3, 4, 5, 8, 257, 1000))) + [(3, lim["block_cap"] * 256 * 4 + 8), (70001, 4), (70001, 3)]
    for M, N in shapes:
        x, b = mixed(rs, M * N, dt).reshape(M, N), mixed(rs, N, dt)
        for v in (x, b):
            v[np.abs(v) == np.finfo(dt).max] = -3.0            # (no overflow edge, as for axpy)
        with np.errstate(all="ignore"):
            z = x.astype(hi_t) + b.astype(hi_t)[None, :]
            refs = {_lib.ACT_NONE: z, _lib.ACT_RELU: np.where(z < 0, hi_t(0), z)}
        for act in (_lib.ACT_NONE, _lib.ACT_RELU):
            for offs in ([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)] if M * N < 100000 else [(0, 0, 0), (0, 0, 2)]):
                dx, db = Dev(x, off=offs[0]), Dev(b, off=offs[1])
                out = Dev(n=M * N, dtype=dt, off=offs[2])
                L.bias_act(dx.ptr, db.ptr, act, out.ptr, M, N, CODE[dtype])
                got, bad = out.read()
                label = _label("act%d" % act, "%dx%d" % (M, N), offs)
                rep.guard(label, bad)
                # sum rounded once; ReLU of a sum that rounds to -0.0 may give either zero: compared as values
                g = got.copy()
                g[g == 0] = 0
                r = refs[act].ravel().copy()
                with np.errstate(all="ignore"):
                    r[r.astype(dt) == 0] = 0
                rep.ulps(label, g, r, 1.0)
    rep.finish()


# --------------------------------------------------------------------------------------------------------- registry
FAMILIES = {
    "flat": (family_flat, FLOATS),
    "fill": (family_fill, ALL_DTYPES),
    "strided": (family_strided, FLOATS),
    "reduce": (family_reduce, FLOATS),
    "argmax": (family_argmax, FLOATS),
    "copy": (family_copy, ALL_DTYPES),
    "rows": (family_rows, ALL_DTYPES),
    "cast": (family_cast, ALL_DTYPES),
    "one_hot": (family_one_hot, FLOATS),
    "bias_act": (family_bias_act, FLOATS),
}
CASES = sorted("%s-%s" % (family, dtype) for family, (_, dtypes) in FAMILIES.items() for dtype in dtypes)


def run_case(case):
    family, dtype = case.rsplit("-", 1)
    FAMILIES[family][0](dtype)
