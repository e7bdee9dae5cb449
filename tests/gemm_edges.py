"""Sweep of the fp32 / f64 GEMM entry points (tnn_gemm, tnn_gemm_bias_act, tnn_gemm_mask, tnn_gemm_tn_colsum of
csrc/tnn_gemm.hip) against exact references at their dispatch edges.  Backend-agnostic, like kernel_sweep.py:
test_gpu_gemm_edges.py runs the families through libtnn_hip.so on the MI355X, test_gemm_edges_twin.py through the CPU twin.

Every call goes through the C-ABI with raw pointers.  A 2-D operand is `rows x cols` elements inside a larger allocation
(Mat): leading dimension `cols + pad`, a whole-element offset from a 16-byte-aligned base, 64-byte guards on both sides.
  * inputs: guards and pad columns hold NaN, so an out-of-range element that reaches an accumulator poisons the result
    even where the other operand holds a zero;
  * outputs: guards and pad columns hold the sentinel and must be bit-unchanged; the payload is pre-filled with NaN whenever
    the epilogue must not read it (beta == 0, bias_act, mask, colsum) and must come back finite.

Input kinds (what each is compared with):
  1 small integers in [-7, 7]: every partial sum in any order is exact (49 K <= 2^24), so the result is compared bit for
    bit with numpy float64 cast to the dtype (zeros as values).  Under relu_sign = 1 the sign bit is the contract: the
    expected value is -0.0 where z < 0 and |z| elsewhere, compared with its zero signs.
  2 selection products: one operand with full-mantissa values (and max/8, tiny, a subnormal), the other with exactly one
    +-2^e per column (row) at a random k, first and last k forced.  Exact: bit for bit.
  3 Gaussian x Gaussian: |err| <= gamma_n (|alpha| |A||B| + |beta| |C0| + |bias|), gamma_n = n u / (1 - n u),
    n = K + splits + 2 — a derived bound, not a measured one.  The observed maxima go to TNN_SWEEP_ERR_OUT.
  4 specials on integer inputs: one NaN in A poisons exactly its row, one in B exactly its column, ReLU keeps it, the mask
    selects (a masked element is 0 even where the product is NaN), the column sum takes it in exactly its column.

One entry of CASES per family; a label reads `family/entry/layout/MxNxK/variant[/branch]`, where `branch` is the kernel the
host rules of tnn_gemm.hip pick for that call on the HIP library (mirrored here for the label only; nothing asserts it).
"""

import os

import numpy as np

from kernel_sweep import CODE, Report, _bits, device_limits, lib, sentinel
from tinynn_autograd_amd import _lib
from tinynn_autograd_amd import device_array as da

GUARD_BYTES = 64
LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]
LNAME = {(0, 0): "NN", (0, 1): "NT", (1, 0): "TN", (1, 1): "TT"}
ENV_KNOBS = ("TNN_GEMM_CFG", "TNN_GEMM_SPLITK", "TNN_GEMM_SMALL", "TNN_GEMM_GROUP_M")
TILE = {0: (128, 128), 1: (64, 128), 2: (64, 64), 3: (128, 64)}
OBSERVED_ERR = {}                      # (family, entry) -> (largest err / (u * bound) of kind 3, the n of its gate)

# operand -> (offset in elements, pad columns) per variant; Y follows C, the bias B and db C
VARIANTS = {
    "dense": {},
    "padded4": {"pad": {"A": 4, "B": 4, "C": 4, "Y": 4}},
    "A+1": {"off": {"A": 1}},
    "B+1": {"off": {"B": 1, "bias": 1}},
    "C+1": {"off": {"C": 1, "Y": 2, "db": 1}},
    "ld_odd": {"pad": {"A": 1, "B": 1, "C": 3, "Y": 3}},
    "A+1/ld_odd": {"off": {"A": 1}, "pad": {"A": 1, "B": 1, "C": 3, "Y": 3}},
}
ALL_VARIANTS = ["dense", "padded4", "A+1", "B+1", "C+1", "ld_odd"]
BIG_VARIANTS = ["dense", "padded4", "A+1/ld_odd"]


class Mat(object):
    """rows x cols elements on the device: [guard | off elements | rows x (cols + pad) | guard].  Everything outside the
    logical elements holds `outside` (NaN for an input, the sentinel for an output)."""

    def __init__(self, rows, cols, dtype, pad=0, off=0, data=None, fill=None, output=False):
        self.dt = np.dtype(dtype)
        self.rows, self.cols = int(rows), int(cols)
        self.ld = max(self.cols + int(pad), 1)
        self.g = GUARD_BYTES // self.dt.itemsize
        self.lo = self.g + int(off)
        self.n = self.rows * self.ld
        total = self.lo + self.n + self.g
        self.image = np.full(total, sentinel(self.dt) if output else np.nan, self.dt)
        if data is not None:
            self._view(self.image)[...] = np.asarray(data, self.dt).reshape(self.rows, self.cols)
        elif fill is not None:
            self._view(self.image)[...] = fill
        self.buf = da.DeviceArray._new((total * self.dt.itemsize,), np.bool_)
        assert self.buf._ptr % 16 == 0, "allocator returned a base that is not 16-byte aligned"
        lib().memcpy_h2d(self.buf._ptr, self.image.ctypes.data, self.image.nbytes)
        self.ptr = self.buf._ptr + self.lo * self.dt.itemsize

    def _view(self, img):
        return img[self.lo:self.lo + self.n].reshape(self.rows, self.ld)[:, :self.cols]

    def read(self):
        """(the logical elements, index relative to the operand's first element of the first changed element outside
        them — guard or pad column — or None)."""
        got = np.empty_like(self.image)
        lib().memcpy_d2h(got.ctypes.data, self.buf._ptr, got.nbytes)
        payload = self._view(got).copy()
        self._view(got)[...] = self._view(self.image)
        bad = np.flatnonzero(_bits(got) != _bits(self.image))
        return payload, (int(bad[0]) - self.lo if bad.size else None)


# ------------------------------------------------------------------------------------------------- host-rule mirror
def eff_splits(K, s):
    """launch_cfg: the split count after its clamps (BK = 32)."""
    ktiles = (K + 31) // 32
    s = max(1, min(s, ktiles))
    per = max(1, -(-ktiles // s))
    return -(-ktiles // per) if ktiles else 1


def branch(tA, tB, M, N, K, var, cus, forced=None):
    """Label only: the kernel gemm_f32 picks (use_small_path / use_mid_path / the tile and split rules)."""
    v = VARIANTS[var]
    off, pad = v.get("off", {}), v.get("pad", {})

    def vec(name, contiguous):
        return off.get(name, 0) % 4 == 0 and (contiguous + pad.get(name, 0)) % 4 == 0 and contiguous % 4 == 0
    va, vb = vec("A", M if tA else K), vec("B", K if tB else N)
    vtag = "VEC" if va and vb else "guarded"
    if forced is not None:
        c, s = forced
        return "tiled cfg%d %s splits=%d" % (c, vtag, eff_splits(K, s))
    akc, bkc = not tA, bool(tB)
    mid_ok = (not akc or vec("A", K)) and (not bkc or vec("B", K))
    flop = 2.0 * M * N * K
    if flop <= 4.2e8 and -(-M // 16) * -(-N // 16) <= 8192:
        if flop >= 1.5e8 and -(-M // 32) * -(-N // 32) >= 192 and mid_ok:
            return "mid"
        chunks = -(-K // 16)
        return "small %dw%s" % (4 if chunks <= 16 else 8 if chunks <= 48 else 16, " FAST" if mid_ok and (not tA or tB) else "")
    t3, t2 = -(-M // 128) * -(-N // 64), -(-M // 64) * -(-N // 64)
    t1 = -(-M // 64) * -(-N // 128)
    cfg = 3 if t3 >= cus // 2 else 2
    if cfg == 3 and not tA and M <= 1024 and cus // 2 <= t1 <= 2 * cus:
        cfg = 1
    tiles = {3: t3, 2: t2, 1: t1}[cfg]
    s = 1
    if tiles < cus:
        s = max(1, min(-(-cus // tiles), K // 256, 16))
    return "tiled cfg%d %s splits=%d" % (cfg, vtag, eff_splits(K, s))


def natural_splits(tA, tB, M, N, K, var, cus):
    b = branch(tA, tB, M, N, K, var, cus)
    return int(b.rsplit("=", 1)[1]) if "splits=" in b else 1


# ---------------------------------------------------------------------------------------------------------- epilogues
AXPBY = [("gemm", a, b) for a in (1.0, -2.0, 0.5) for b in (0.0, 1.0, -0.5)]
BIAS = [("bias", _lib.ACT_NONE, 0), ("bias", _lib.ACT_RELU, 0), ("bias", _lib.ACT_RELU, 1)]


def entry_name(spec):
    if spec[0] == "gemm":
        return "gemm(a=%g,b=%g)" % spec[1:3]
    if spec[0] == "bias":
        return "bias_act(%s%s)" % ("relu" if spec[1] == _lib.ACT_RELU else "none", ",sign" if spec[2] else "")
    if spec[0] == "mask":
        return "mask"
    return "tn_colsum(%s)" % ("db" if spec[1] else "no db")


def family_entry(spec):
    return {"gemm": "tnn_gemm", "bias": "tnn_gemm_bias_act", "mask": "tnn_gemm_mask", "colsum": "tnn_gemm_tn_colsum"}[spec[0]]


MASK_SOURCES = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, np.copysign(np.nan, -1.0)])


def epilogue_ref(spec, P, ops):
    """The epilogue of `spec` on the product P, in P's precision.  ops: C0 / bias / Y as given to the call."""
    hi = P.dtype.type
    with np.errstate(all="ignore"):
        if spec[0] == "gemm":
            r = hi(spec[1]) * P
            if spec[2] != 0.0:
                r = r + hi(spec[2]) * ops["C0"].astype(hi)
            return r
        if spec[0] == "bias":
            z = P + ops["bias"].astype(hi)[None, :]
            if spec[1] != _lib.ACT_RELU:
                return z
            return np.where(z < 0, hi(-0.0), np.abs(z)) if spec[2] else np.where(z < 0, hi(0), z)
        if spec[0] == "mask":
            return np.where(np.signbit(ops["Y"]), hi(0), P)
        return P


def product(tA, tB, A, B, hi=np.float64):
    opA, opB = (A.T if tA else A), (B.T if tB else B)
    with np.errstate(all="ignore"):
        return np.matmul(opA.astype(hi), opB.astype(hi))


class Sweep(object):
    def __init__(self, family, dtype, seed, env=None):
        self.rep = Report(family, dtype)
        self.family, self.dt = family, np.dtype(dtype)
        self.rs = np.random.RandomState(seed)
        self.cus = device_limits()["cus"]
        self.env = env
        self.forced = None
        self._count = {}
        for k in ENV_KNOBS:
            self._setenv(k, None)

    # ---- environment (the tuning overrides; the test hands in pytest's monkeypatch, which restores them)
    def _setenv(self, key, value):
        if self.env is None:
            assert value is None and key not in os.environ, "%s needs the caller's monkeypatch" % key
        elif value is None:
            self.env.delenv(key, raising=False)
        else:
            self.env.setenv(key, str(value))

    def force(self, cfg, splits):
        self.forced = None if cfg is None else (cfg, splits)
        self._setenv("TNN_GEMM_CFG", cfg)
        self._setenv("TNN_GEMM_SPLITK", splits if cfg is not None else None)

    # ---- rotation: every variant and every epilogue comes round per layout
    def _next(self, key, seq):
        # plain round-robin per key; the epilogues shift by one every full turn so that they do not stay in step with the
        # variants (which would pair each variant with the same few epilogues for ever)
        c = self._count.get(key, 0)
        self._count[key] = c + 1
        return seq[(c + c // len(seq)) % len(seq)] if key[0] == "spec" else seq[c % len(seq)]

    def variant(self, lay, variants):
        return self._next(("var", lay, tuple(variants)), variants)

    def specs(self, lay, n):
        """n epilogues for one product: the groups alpha/beta, bias/activation and mask (and column sum for TN) in turn."""
        groups = [AXPBY, BIAS, [("mask",)] + ([("colsum", True), ("colsum", False)] if lay == (1, 0) else [])]
        out = []
        for _ in range(n):
            gi = self._next(("group", lay), [0, 1, 2])
            out.append(self._next(("spec", lay, gi), groups[gi]))
        return out

    def label(self, spec, lay, M, N, K, var, extra=""):
        if self.dt == np.float32:
            br = branch(lay[0], lay[1], M, N, K, var, self.cus, self.forced)
        else:
            br = "f64"
        return "%s/%s/%dx%dx%d/%s/%s%s" % (entry_name(spec), LNAME[lay], M, N, K, var, br, extra)

    # ---- one call
    def operands(self, spec, M, N, kind):
        """The epilogue's host-side operands for `spec`: integer (kind 1, 2, 4) or Gaussian (kind 3)."""
        rs, dt = self.rs, self.dt
        draw = (lambda *s: rs.randint(-7, 8, s).astype(dt)) if kind != 3 else (lambda *s: rs.standard_normal(s).astype(dt))
        ops = {}
        if spec[0] == "gemm" and spec[2] != 0.0:
            ops["C0"] = draw(M, N)
        if spec[0] == "bias":
            ops["bias"] = draw(N)
        if spec[0] == "mask":
            ops["Y"] = MASK_SOURCES[rs.randint(0, MASK_SOURCES.size, (M, N))].astype(dt)
        return ops

    def call(self, label, spec, lay, M, N, K, A, B, var, ops):
        """Uploads, calls, checks the guards.  Returns (C, db or None), or None when the call was refused (a failure)."""
        v = VARIANTS[var]
        off, pad = v.get("off", {}), v.get("pad", {})
        dt, code, L = self.dt, CODE[self.dt.name], lib()
        tA, tB = lay
        with_db = spec[0] == "colsum" and spec[1]
        dA = Mat(A.shape[0], A.shape[1], dt, pad.get("A", 0), off.get("A", 0), data=A)
        # (the column sum needs a dense G: ldg == N)
        dB = Mat(B.shape[0], B.shape[1], dt, 0 if with_db else pad.get("B", 0), off.get("B", 0), data=B)
        reads_c = "C0" in ops
        dC = Mat(M, N, dt, pad.get("C", 0), off.get("C", 0), output=True, data=ops.get("C0"), fill=None if reads_c else np.nan)
        keep = [dA, dB, dC]
        db = None
        try:
            if spec[0] == "gemm":
                L.gemm(tA, tB, M, N, K, float(spec[1]), dA.ptr, dA.ld, dB.ptr, dB.ld, float(spec[2]), dC.ptr, dC.ld, code)
            elif spec[0] == "bias":
                dbias = Mat(1, N, dt, 0, off.get("bias", 0), data=ops["bias"])
                keep.append(dbias)
                L.gemm_bias_act(tA, tB, M, N, K, dA.ptr, dA.ld, dB.ptr, dB.ld, dbias.ptr, spec[1], spec[2], dC.ptr, dC.ld, code)
            elif spec[0] == "mask":
                dY = Mat(M, N, dt, pad.get("Y", 0), off.get("Y", 0), data=ops["Y"])
                keep.append(dY)
                L.gemm_mask(tA, tB, M, N, K, dA.ptr, dA.ld, dB.ptr, dB.ld, dY.ptr, dY.ld, dC.ptr, dC.ld, code)
            else:
                assert lay == (1, 0)
                if with_db:
                    db = Mat(1, N, dt, 0, off.get("db", 0), output=True, fill=np.nan)
                L.gemm_tn_colsum(M, N, K, dA.ptr, dA.ld, dB.ptr, dB.ld, dC.ptr, dC.ld, db.ptr if with_db else None, code)
        except _lib.TnnError as exc:
            self.rep.checks += 1
            self.rep._fail(label, "raised %s" % exc)
            return None
        got, bad = dC.read()
        self.rep.guard(label, bad)
        got_db = None
        if with_db:
            got_db, bad = db.read()
            self.rep.guard(label + " db", bad)
            got_db = got_db.ravel()
        del keep
        return got, got_db

    def exact(self, label, spec, got, ref_hi, got_db=None, db_hi=None):
        with np.errstate(all="ignore"):
            self.rep.bits(label, got, ref_hi.astype(self.dt), zero_sign=spec[0] == "bias" and bool(spec[2]))
            if got_db is not None:
                self.rep.bits(label + " db", got_db, db_hi.astype(self.dt), zero_sign=False)

    # ---- kind 1
    def integers(self, lay, M, N, K, var, spec, extra=""):
        tA, tB = lay
        rs, dt = self.rs, self.dt
        A = rs.randint(-7, 8, (K, M) if tA else (M, K)).astype(dt)
        B = rs.randint(-7, 8, (N, K) if tB else (K, N)).astype(dt)
        ops = self.operands(spec, M, N, 1)
        label = self.label(spec, lay, M, N, K, var, extra)
        out = self.call(label, spec, lay, M, N, K, A, B, var, ops)
        if out is not None:
            self.exact(label, spec, out[0], epilogue_ref(spec, product(tA, tB, A, B), ops), out[1], B.astype(np.float64).sum(axis=0))

    # ---- kind 2
    def _full(self, rows, cols):
        fi = np.finfo(self.dt)
        x = self.rs.standard_normal((rows, cols)).astype(self.dt)
        x[x == 0] = 1
        ext = np.array([fi.max / 8, fi.tiny, fi.tiny * 0.375, -fi.max / 8], self.dt)     # (0.375 tiny: a subnormal whose half is exact)
        k = min(x.size, ext.size)
        x.ravel()[self.rs.permutation(x.size)[:k]] = ext[:k]
        return x

    def _select(self, K, n):
        """K x n: one nonzero +-2^e per column, e in {-1, 0, 1}; the last and the first k forced."""
        ks = self.rs.randint(0, K, n)
        ks[0] = K - 1
        if n > 1:
            ks[1] = 0
        S = np.zeros((K, n), self.dt)
        S[ks, np.arange(n)] = self.rs.choice([-1.0, 1.0], n) * 2.0 ** self.rs.randint(-1, 2, n)
        return S

    def selection(self, lay, M, N, K, var, extra=""):
        """Both orientations: the selection matrix as op(B), then as op(A)."""
        tA, tB = lay
        if K == 0:
            return
        for orient in (0, 1):
            if orient == 0:
                F, S = self._full(M, K), self._select(K, N)
                A, B = (F.T.copy() if tA else F), (S.T.copy() if tB else S)
            else:
                S, F = self._select(K, M), self._full(K, N)
                A, B = (S if tA else S.T.copy()), (F.T.copy() if tB else F)
            choices = [("gemm", 1.0, 0.0), ("mask",)] + ([("colsum", False)] if lay == (1, 0) else [])
            spec = self._next(("sel", lay), choices)
            ops = self.operands(spec, M, N, 2)
            label = self.label(spec, lay, M, N, K, var, "/select-%s%s" % ("AB"[1 - orient], extra))
            out = self.call(label, spec, lay, M, N, K, A, B, var, ops)
            if out is not None:
                self.exact(label, spec, out[0], epilogue_ref(spec, product(tA, tB, A, B), ops))

    # ---- kind 3
    def _bounded(self, label, key, got, ref, bound, n, relu=None):
        """|got - ref| <= gamma_n bound; relu = (z, sign mode): compared only where |z| exceeds the gate, elsewhere a zero of
        either sign or a value within twice the gate is accepted."""
        self.rep.checks += 1
        u = 2.0 ** -24 if self.dt == np.float32 else 2.0 ** -53
        hi = ref.dtype.type
        gate = hi(n * u / (1 - n * u)) * bound
        g = got.astype(hi)
        ok = np.isfinite(g)
        if relu is None:
            err = np.abs(g - ref)
            ok &= err <= gate
            measured = np.ones(g.shape, bool)
        else:
            z, sign = relu
            measured = np.abs(z) > gate
            err = np.abs((np.abs(g) if sign else g) - ref)
            ok &= np.where(measured, err <= gate, np.abs(g) <= 2 * gate)
            if sign:
                ok &= ~measured | (np.signbit(got) == (z < 0))
        m = measured & (bound > 0) & np.isfinite(g)
        ratio = float(np.max(err[m] / (hi(u) * bound[m]))) if m.any() else 0.0
        old = OBSERVED_ERR.get(key, (0.0, 0))
        OBSERVED_ERR[key] = (max(old[0], ratio), max(old[1], n))
        if not ok.all():
            bad = np.flatnonzero(~ok.ravel())
            self.rep._fail(label, "%d of %d outside gamma_%d x bound, max err / (u bound) %.4g, first bad index %d (got %r, expected %r)"
                           % (bad.size, g.size, n, ratio, bad[0], got.ravel()[bad[0]], float(ref.ravel()[bad[0]])))

    def gaussian(self, lay, M, N, K, var, splits=1):
        tA, tB = lay
        rs, dt = self.rs, self.dt
        hi = np.float64 if dt == np.float32 else np.longdouble
        n = K + splits + 2
        A = rs.standard_normal((K, M) if tA else (M, K)).astype(dt)
        B = rs.standard_normal((N, K) if tB else (K, N)).astype(dt)
        P, absP = product(tA, tB, A, B, hi), product(tA, tB, np.abs(A), np.abs(B), hi)
        todo = [("gemm", -2.0, -0.5), ("gemm", 1.0, 0.0)] + BIAS + [("mask",)] + ([("colsum", True)] if lay == (1, 0) else [])
        for spec in todo:
            ops = self.operands(spec, M, N, 3)
            label = self.label(spec, lay, M, N, K, var, "/gauss")
            out = self.call(label, spec, lay, M, N, K, A, B, var, ops)
            if out is None:
                continue
            key = (self.family, family_entry(spec))
            ref = epilogue_ref(spec, P, ops)
            relu = None
            if spec[0] == "gemm":
                bound = abs(hi(spec[1])) * absP + (abs(hi(spec[2])) * np.abs(ops["C0"].astype(hi)) if spec[2] else 0)
            elif spec[0] == "bias":
                bound = absP + np.abs(ops["bias"].astype(hi))[None, :]
                if spec[1] == _lib.ACT_RELU:
                    relu = (P + ops["bias"].astype(hi)[None, :], bool(spec[2]))
            else:
                bound = absP
            self._bounded(label, key, out[0], ref, bound, n, relu)
            if out[1] is not None:
                self._bounded(label + " db", (self.family, "tnn_gemm_tn_colsum db"), out[1], B.astype(hi).sum(axis=0),
                              np.abs(B.astype(hi)).sum(axis=0), K + 2)

    # ---- kind 4
    def specials(self, lay, M, N, K, var):
        tA, tB = lay
        rs, dt = self.rs, self.dt
        if K == 0:
            return
        A = rs.randint(-7, 8, (K, M) if tA else (M, K)).astype(dt)
        B = rs.randint(-7, 8, (N, K) if tB else (K, N)).astype(dt)
        i0, k0, k1, j1 = rs.randint(M), rs.randint(K), rs.randint(K), rs.randint(N)
        An, Bn = A.copy(), B.copy()
        An[(k0, i0) if tA else (i0, k0)] = np.nan
        Bn[(j1, k1) if tB else (k1, j1)] = np.nan
        plain = ("gemm", 1.0, 0.0)
        clean = self.call(self.label(plain, lay, M, N, K, var, "/clean"), plain, lay, M, N, K, A, B, var, {})
        if clean is None:
            return
        for name, a, b, sl in (("nanA[%d,%d]" % (i0, k0), An, B, (i0, slice(None))), ("nanB[%d,%d]" % (k1, j1), A, Bn, (slice(None), j1))):
            label = self.label(plain, lay, M, N, K, var, "/" + name)
            out = self.call(label, plain, lay, M, N, K, a, b, var, {})
            if out is not None:
                ref = clean[0].copy()
                ref[sl] = np.nan
                self.rep.bits(label, out[0], ref)
        P = product(tA, tB, An, B)
        for spec in [("bias", _lib.ACT_RELU, 0), ("bias", _lib.ACT_RELU, 1), ("mask",)]:
            ops = self.operands(spec, M, N, 4)
            label = self.label(spec, lay, M, N, K, var, "/nanA[%d,%d]" % (i0, k0))
            out = self.call(label, spec, lay, M, N, K, An, B, var, ops)
            if out is not None:
                self.exact(label, spec, out[0], epilogue_ref(spec, P, ops))
        if lay == (1, 0):
            spec = ("colsum", True)
            label = self.label(spec, lay, M, N, K, var, "/nanG[%d,%d]" % (k1, j1))
            out = self.call(label, spec, lay, M, N, K, A, Bn, var, {})
            if out is not None:
                with np.errstate(all="ignore"):
                    self.exact(label, spec, out[0], product(tA, tB, A, Bn), out[1], Bn.astype(np.float64).sum(axis=0))

    def finish(self):
        _dump_observed()
        self.force(None, None)
        self.rep.finish()


def _dump_observed():
    """TNN_SWEEP_ERR_OUT=<file>: the kind-3 maxima of this process, rewritten after every family (the source of
    profiles/gemm_edges_err.txt)."""
    path = os.environ.get("TNN_SWEEP_ERR_OUT")
    if not path:
        return
    with open(path, "w") as f:
        f.write("# backend %s\n# family entry observed_max_err_over_u_bound largest_n (gate: gamma_n = n u / (1 - n u), i.e. about n)\n"
                % _lib.backend_name())
        for (fam, entry), (v, n) in sorted(OBSERVED_ERR.items()):
            f.write("%s %s %.4f %d\n" % (fam, entry, v, n))


# ----------------------------------------------------------------------------------------------------------- families
def family_small(dtype, env):
    """Natural dispatch, the 16 x 16 latency kernel: the 4 / 8 / 16-wave switch at 16 and 48 chunks, K % 4 and K % 16 tails,
    FAST and guarded loaders.  (128, 10) is the one grid pick_xcd_cut can cut."""
    sw = Sweep("small", dtype, 1101, env)
    shapes = [(1, 1), (16, 16), (17, 33), (33, 15), (15, 17), (128, 10)]
    for K in (0, 1, 3, 4, 15, 16, 17, 64, 255, 256, 257, 260, 768, 769, 772):
        for M, N in shapes:
            for lay in LAYOUTS:
                variants = ALL_VARIANTS if K in (17, 260) else [sw.variant(lay, ALL_VARIANTS)]
                for var in variants:
                    for spec in sw.specs(lay, 3 if len(variants) == 1 else 2):
                        sw.integers(lay, M, N, K, var, spec)
                sw.selection(lay, M, N, K, sw.variant(lay, ALL_VARIANTS))
    for lay in LAYOUTS:
        for (M, N, K), var in (((17, 33, 260), "dense"), ((33, 15, 769), "A+1"), ((128, 10, 64), "padded4")):
            sw.specials(lay, M, N, K, var)
        sw.gaussian(lay, 33, 15, 772, "dense")
        sw.gaussian(lay, 17, 33, 257, "ld_odd")
    sw.finish()


def family_mid(dtype, env):
    """Natural dispatch around use_mid_path (flop >= 1.5e8, >= 192 tiles of 32 x 32, mid_ok): (448, 448, 376) just inside,
    (417, 449, 380) ragged tiles, (416, 448, 404) 182 tiles -> small kernel, (448, 448, 378) K % 4 != 0 -> only TN stays mid."""
    sw = Sweep("mid", dtype, 1202, env)
    variants = ["dense", "padded4", "A+1"]
    for M, N, K in ((448, 448, 376), (417, 449, 380), (416, 448, 404), (448, 448, 378)):
        for lay in LAYOUTS:
            for var in variants:
                for spec in sw.specs(lay, 2 if lay == (1, 0) else 1):
                    sw.integers(lay, M, N, K, var, spec)
            sw.selection(lay, M, N, K, sw.variant(lay, variants))
    for lay in LAYOUTS:
        sw.integers(lay, 448, 448, 376, "dense", ("colsum", True) if lay == (1, 0) else ("mask",))
        sw.specials(lay, 417, 449, 380, "dense")
        sw.gaussian(lay, 448, 448, 376, "padded4")
    sw.finish()


def family_tiled_forced(dtype, env):
    """The LDS-tiled kernel at small shapes: TNN_GEMM_CFG routes any shape to it, TNN_GEMM_SPLITK picks the split.  Every tile
    configuration x layout x VEC value; partial raster group and a tile count that is no multiple of 8 ((9 BM + 1, BN + 1, 8));
    split-K with every epilogue in splitk_reduce_kernel."""
    sw = Sweep("tiled-forced", dtype, 1303, env)
    everything = [("gemm", -2.0, 1.0), ("gemm", 0.5, -0.5), ("bias", _lib.ACT_RELU, 1), ("bias", _lib.ACT_NONE, 0), ("mask",)]
    for c in (0, 1, 2, 3):
        BM, BN = TILE[c]
        shapes = [(1, 1, 1), (BM + 1, BN - 1, 33), (2 * BM, 2 * BN, 64), (BM + 4, BN + 4, 100), (9 * BM + 1, BN + 1, 8)]
        shapes += [(BM + 1, BN - 1, K) for K in (0, 31, 32, 257)]
        split_runs = [(s, (BM + 4, BN + 4, 100)) for s in (1, 2, 3, 16)] + [(4, (BM + 1, BN - 1, 257))]
        for lay in LAYOUTS:
            sw.force(c, 1)
            for M, N, K in shapes:
                for var in BIG_VARIANTS:
                    for spec in sw.specs(lay, 1):
                        sw.integers(lay, M, N, K, var, spec)
            # the staged 16-byte store of interior tiles with every epilogue (splits == 1 applies it there)
            for spec in everything:
                sw.integers(lay, 2 * BM, 2 * BN, 64, "padded4", spec)
            for s, (M, N, K) in split_runs:
                sw.force(c, s)
                for spec in everything + ([("colsum", True)] if lay == (1, 0) else []):
                    sw.integers(lay, M, N, K, "ld_odd" if spec[0] == "colsum" else sw.variant(lay, ["padded4", "A+1/ld_odd", "ld_odd"]), spec)
                sw.selection(lay, M, N, K, sw.variant(lay, BIG_VARIANTS))
            for i, (M, N, K) in enumerate(shapes):
                sw.force(c, (1, 2, 3)[i % 3])
                sw.selection(lay, M, N, K, sw.variant(lay, BIG_VARIANTS))
            sw.force(c, 3)
            sw.specials(lay, BM + 4, BN + 4, 100, "A+1/ld_odd")
            sw.force(c, 1)
            sw.specials(lay, 2 * BM, 2 * BN, 64, "dense")
        lay = LAYOUTS[c]
        sw.force(c, 3)
        sw.gaussian(lay, BM + 4, BN + 4, 100, "padded4", eff_splits(100, 3))
        sw.force(c, 1)
        sw.gaussian(LAYOUTS[(c + 1) % 4], BM + 1, BN - 1, 257, "A+1/ld_odd", 1)
    sw.finish()


def natural_shapes(cus):
    """The smallest shapes at which gemm_f32's own rules pick each tiled branch (256 CUs: the shapes of the MI355X)."""
    half = cus // 2
    tm3 = max(9, -(-half // 16))                      # cfg 3: >= cus / 2 tiles of 128 x 64, more than 1024 rows
    tm1 = -(-half // 8)                               # cfg 1: cus / 2 tiles of 64 x 128 in at most 1024 rows
    out = [("cfg2 split-K", (520, 520, 800), LAYOUTS), ("cfg3", (128 * (tm3 - 1) + 1, 961, 220), LAYOUTS),
           ("flop switch, small side", (520, 520, 776), LAYOUTS), ("flop switch, tiled side", (520, 520, 777), LAYOUTS)]
    if 64 * tm1 <= 1024:
        out.append(("cfg1", (64 * tm1, 1024, 208), [(0, 0), (0, 1)]))
    return out


def family_tiled_natural(dtype, env):
    """No overrides: (520, 520, 800) cfg 2 with 3-way split-K, (1025, 961, 220) cfg 3, (1024, 1024, 208) NN / NT cfg 1, and the
    flop switch at (520, 520, 776 | 777) — the shapes for 256 CUs; natural_shapes derives them from the device's count."""
    sw = Sweep("tiled-natural", dtype, 1404, env)
    for what, (M, N, K), lays in natural_shapes(sw.cus):
        for lay in lays:
            for var in ("dense", "padded4"):
                specs = sw.specs(lay, 1)
                if what == "cfg3" and lay == (1, 0) and var == "dense":
                    specs = [("colsum", True)]            # the column sum as a separate tnn_reduce launch
                for spec in specs:
                    sw.integers(lay, M, N, K, var, spec)
    for what, (M, N, K), lays in natural_shapes(sw.cus):
        if what in ("cfg2 split-K", "cfg3", "cfg1"):
            lay = lays[1] if what == "cfg1" else (1, 0)
            sw.gaussian(lay, M, N, K, "dense", natural_splits(lay[0], lay[1], M, N, K, "dense", sw.cus))
    sw.finish()


def family_f64(dtype, env):
    """gemm_f64_kernel (64 x 64 tiles, K step 16) and the tall product whose row-tile count exceeds a grid's y limit."""
    sw = Sweep("f64", dtype, 1505, env)
    sizes = (1, 63, 64, 65, 129)
    for K in (0, 1, 15, 16, 17, 33, 100):
        for M in sizes:
            for N in sizes:
                for lay in LAYOUTS:
                    var = sw.variant(lay, ALL_VARIANTS)
                    for spec in sw.specs(lay, 1):
                        sw.integers(lay, M, N, K, var, spec)
                    sw.selection(lay, M, N, K, var)
    for lay in LAYOUTS:
        sw.specials(lay, 65, 129, 33, "ld_odd")
        sw.specials(lay, 63, 1, 17, "C+1")
        sw.gaussian(lay, 129, 65, 100, "padded4")
    tall = 64 * 65535 + 1                             # 65536 row tiles
    for lay in ((0, 0), (1, 0)):
        sw.integers(lay, tall, 1, 1, "dense", ("gemm", 1.0, 0.0), "/tall")
    sw.finish()


FAMILIES = {
    "small-float32": family_small,
    "mid-float32": family_mid,
    "tiled-forced-float32": family_tiled_forced,
    "tiled-natural-float32": family_tiled_natural,
    "float64": family_f64,
}
CASES = sorted(FAMILIES)


def run_case(case, env=None):
    """`env`: pytest's monkeypatch (the tuning overrides are set and cleared through it and restored by it)."""
    FAMILIES[case](case.rsplit("-", 1)[1] if "-" in case else case, env)
