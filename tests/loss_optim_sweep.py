"""Sweep of the loss and optimizer kernels (the second half of csrc/tnn_fused.hip, csrc/tnn_nll_rows.h, tnn_adam_tick)
against np.longdouble at their dispatch edges.  Backend-agnostic, like kernel_sweep.py, whose Dev / Report / guard
machinery it reuses: test_gpu_loss_optim_sweep.py runs the families through libtnn_hip.so on the MI355X,
test_loss_optim_sweep_twin.py through the CPU twin.

Every call goes through the C-ABI with raw pointers into Dev allocations (sentinel guards on both sides, whole-element
base offsets 0..3).  After a call the output guards must be unchanged, the read-only operands bit-identical to what
was uploaded, and an output passed as NULL must simply not be written.

Tolerances are error models evaluated on the reference, never fitted to what a kernel gives.

Softmax NLL (the whole-batch form, core/losses.py:24-32).  With x = M - z >= 0, eps = the dtype's machine epsilon:
  * a same-precision exp(z - M) carries relative error <= (x/2 + 2) eps: the argument is rounded (|x| eps/2 absolute,
    which is relative in the exponential), exp itself is within one ulp, one cast.  Splitting the argument as
    (z - m_r) + (m_r - M), as the row kernel does, rounds two smaller arguments and multiplies: the same total.
  * beta_S = eps (sum e (x/2 + 2) / S + 4), beta_q,r = eps (sum_k e y (x/2 + 2) / q_r + 4): the weighted element
    errors plus the six half-ulp steps of a float shuffle tree and the cast of the sum.
  * dz = p - t: |p| (beta_k + beta_S + 3 eps) + |t| (beta_k + beta_q,r + 3 eps)   (a quotient / product, the
    difference and the store, each at most one eps of a term not larger than |p| + |t|).
  * loss: (m / m_global) (beta_S + mean_r beta_q,r + 2 eps (|log S| + mean_r |log q_r|)
    + eps (ceil(log2 m) / 2 + 1) mean_r |log S - log q_r|).  The last term is the sum over the m rows in the dtype, which
    the first form of this model had missed (the literal f32 chain reached 0.54 of that bound at 960 x 15, from the row sum
    alone): a binary tree over m terms takes ceil(log2 m) half-ulp steps of partial sums that never exceed the total, and
    the division by m and the store one more eps.
  * stats[0] is a maximum of inputs: bit-exact.  stats[1] within beta_S S.
On the CPU twin every case also evaluates the same formulas literally in the dtype with numpy and requires that chain to
stay within HALF of every bound: the model is checked against the reference alone before any kernel is judged by it.
That criterion decides the input domain.  The argument rounding alone reaches half an ulp of x, up to x/2 eps just above
a power of two, while half the bound of such an element is about (x/4 + 5.5) eps: no same-precision chain can keep half
of the bound to spare everywhere above 16 (it fails from 16 to about 18 and from 32 to about 52).  So the bulk of the logits lies within 16 of the maximum (sigma <= 1.5 at
levels from -100 to 300; the loss knows no level, a kernel might), and about 3 % of the elements of every case are
placed 56 to 60 below it, one of them exactly at the cap and one 30 below.

lse_merge is the same sum with shard pairs {M_i, S_i} in place of elements: x_i = M - M_i and the bound
eps (sum S_i e^-x_i (x_i/2 + 2) / S + 4) S.

MSE, SGD, Momentum / RMSProp / Adagrad / Adadelta, Adam keep the reference's operation order (core/optimizer.py:67-164).
Their oracle is a running-error arithmetic (class RE): a longdouble value plus a first-order bound through + - * / sqrt
that evaluates the same order.  Every operation is charged one FULL eps of its result (half would be the IEEE rounding;
the other half covers FMA contraction and the few reassociations), plus the smallest normal number as an absolute term:
a result in the denormal range may be flushed (g * g for |g| = tiny is).  The square root propagates its operand's
bound exactly (sqrt(a + d) - sqrt(a), not d / 2 sqrt(a)), so a zero second moment needs no special case.
Hyperparameters enter rounded exactly as the entry points round them ((T)lr, T(1) - (T)b1, (T)(1 / (1 - b1^t)) ...):
those are single IEEE operations and are reproduced bit for bit, not bounded.  State carries over three steps inside the
oracle, bound included.  The MSE loss is a float64 sum of the squares of the dtype-rounded differences: within
(n 2^-52 + eps) sum e^2 / m of it.

TNN_LOSS_SWEEP_OUT=<file> writes, for every (family, dtype, entry), the largest observed error as a fraction of its
bound (profiles/loss_optim_sweep.txt).  A record only: nothing reads it back.
"""

import os

import numpy as np

from kernel_sweep import BUFFER_LIMIT, CODE, FLOATS, Dev, Report, _bits, device_limits, lib, mixed
from tinynn_autograd_amd import _lib

LD = np.longdouble
OBSERVED = {}                          # (family, dtype name, entry) -> largest err / bound seen in this process
MAX_SPREAD = 60                        # M - z <= 60 everywhere: every form's f32 exp stays normal (the flush starts near 87)
B1, B2 = 0.9, 0.999


def on_twin():
    return _lib.backend_name() != "hip-gfx950"


def _dump():
    path = os.environ.get("TNN_LOSS_SWEEP_OUT")
    if not path:
        return
    with open(path, "w") as f:
        f.write("# backend %s\n# family dtype entry max_error_as_fraction_of_bound\n" % _lib.backend_name())
        for (family, dt, entry), v in sorted(OBSERVED.items()):
            f.write("%s %s %s %.4f\n" % (family, dt, entry, v))


def finish(rep):
    _dump()
    rep.finish()


def within(rep, label, entry, got, ref, tol, scale=1.0):
    """|got - ref| <= tol element-wise (ref and tol in longdouble); `scale` < 1 asks for a fraction of the bound.  Records
    the largest err / tol under (family, dtype, entry)."""
    rep.checks += 1
    got = np.asarray(got).ravel()
    ref, tol = np.asarray(ref, LD).ravel(), np.asarray(tol, LD).ravel()
    if got.size != ref.size:
        return rep._fail(label, "%s: size %d, expected %d" % (entry, got.size, ref.size))
    with np.errstate(all="ignore"):
        err = np.abs(got.astype(LD) - ref)
        err[~np.isfinite(got)] = np.inf
        frac = np.where(err == 0, LD(0), err / tol)            # a zero bound admits only a zero error
    worst = float(frac.max()) if frac.size else 0.0
    key = (rep.family, rep.dtype, entry)
    if np.isfinite(worst):
        OBSERVED[key] = max(OBSERVED.get(key, 0.0), worst)
    ok = frac <= scale
    if not ok.all():
        bad = np.flatnonzero(~ok)
        k = int(np.argmax(frac))
        rep._fail(label, "%s: %d of %d outside %g x the bound, worst %.4g x at index %d (got %r, expected %.12g, bound %.4g), "
                  "first bad index %d" % (entry, bad.size, got.size, scale, worst, k, got[k], float(ref[k]), float(tol[k]), bad[0]))


def same_bits(rep, label, what, dev, data):
    """A read-only operand (or an output that must not be written) still holds `data`, and its guards the sentinel."""
    got, bad = dev.read()
    rep.guard(label + "/" + what, bad)
    rep.bits(label + "/" + what + " unchanged", got, np.asarray(data).ravel())


def powers_are(rep, label, dev, p1, p2):
    """The powers block {b1^t, b2^t, ticket, pad}: the pair bit-equal to the float64 products, the self-advance ticket word
    (and the pad) all-zero bits."""
    got, bad = dev.read()
    rep.guard(label + "/pows", bad)
    rep.bits(label + "/pows[0:2]", got[:2], np.array([p1, p2]))
    rep.checks += 1
    if _bits(got[2:]).any():
        rep._fail(label, "ticket word of the powers block is %r after the launch, not zero" % _bits(got[2:]).tolist())


def call(rep, label, fn, *args):
    """A call that must succeed; a refusal is a failure of this case and not the end of the sweep."""
    try:
        fn(*args)
        return True
    except _lib.TnnError as exc:
        rep.checks += 1
        rep._fail(label, "raised %s" % exc)
        return False


def ptr(dev):
    return None if dev is None else dev.ptr


# ------------------------------------------------------------------------------------------------------ softmax NLL
def nll_inputs(rs, m, c, T, onehot, scale=3.0, shift=0.0):
    """Logits with spread exactly at the cap where there is room (one element at M - 60), labels one-hot or dense
    non-negative with a few exact zeros."""
    T = np.dtype(T).type
    z = (rs.standard_normal((m, c)) * scale + shift).astype(T)
    n = m * c
    top = z.max()
    if n >= 3:
        deep = rs.permutation(n)[:max(2, n // 32)]
        deep = deep[z.flat[deep] != top]
        z.flat[deep] = (top - rs.uniform(56, MAX_SPREAD, deep.size)).astype(T)
        if deep.size:
            z.flat[deep[0]] = top - T(MAX_SPREAD + 40)          # clipped to the floor below
        if deep.size > 1:
            z.flat[deep[1]] = top - T(MAX_SPREAD // 2)
    floor = T(top - T(MAX_SPREAD))
    if LD(top) - LD(floor) > MAX_SPREAD:
        floor = np.nextafter(floor, T(np.inf))
    z = np.maximum(z, floor)
    assert (LD(top) - z.astype(LD)).max() <= MAX_SPREAD
    if onehot:
        y = np.zeros((m, c), T)
        y[np.arange(m), rs.randint(0, c, m)] = 1
        if n >= 3:
            r, k = np.unravel_index(np.argmin(z), z.shape)      # one label sits on the lowest logit
            y[r] = 0
            y[r, k] = 1
    else:
        y = rs.rand(m, c).astype(T)
        if c >= 2:
            rows = rs.permutation(m)[:max(1, m // 7)]
            y[rows, rs.randint(0, c, rows.size)] = 0            # never a whole row
    return z, y


class NllRef(object):
    """The longdouble reference of one (z, y, m_global) and the bounds of the error model."""

    def __init__(self, z, y, mg):
        T = z.dtype.type
        eps = LD(np.finfo(T).eps)
        m = z.shape[0]
        zl, yl = z.astype(LD), y.astype(LD)
        self.T, self.z, self.y, self.mg = T, z, y, mg
        self.M = zl.max()
        x = self.M - zl
        e = np.exp(-x)
        self.S = e.sum()
        ey = e * yl
        q = ey.sum(axis=1)
        logS, logq = np.log(self.S), np.log(q)
        self.loss = (logS - logq).sum() / mg
        p, t = e / self.S, ey / q[:, None] / mg
        self.dz = p - t
        w = x / 2 + 2
        beta_k = eps * w
        beta_S = eps * ((e * w).sum() / self.S + 4)
        beta_q = eps * ((ey * w).sum(axis=1) / q + 4)
        self.tol_dz = np.abs(p) * (beta_k + beta_S + 3 * eps) + np.abs(t) * (beta_k + beta_q[:, None] + 3 * eps)
        tree = eps * (np.ceil(np.log2(max(m, 2))) / 2 + 1) * np.abs(logS - logq).mean()
        self.tol_loss = (LD(m) / mg) * (beta_S + beta_q.mean() + 2 * eps * (np.abs(logS) + np.abs(logq).mean()) + tree)
        self.tol_S = beta_S * self.S
        self.stats = np.array([self.M, self.S]).astype(T)       # what a caller of the two-launch form passes on

    def literal(self, rep, label):
        """The same formulas evaluated literally in the dtype by numpy: within half of every bound."""
        T, z, y = self.T, self.z, self.y
        with np.errstate(all="ignore"):
            M = z.max()
            e = np.exp(z - M)
            S = e.sum()
            ey = e * y
            q = ey.sum(axis=1)
            loss = (np.log(S) - np.log(q)).sum() / T(self.mg)
            dz = e / S - ey / q[:, None] / T(self.mg)
        for v in (M, S, loss, dz):
            assert np.asarray(v).dtype == z.dtype
        rep.bits(label + "/literal M", np.array([M]), np.array([self.M]).astype(T))
        within(rep, label, "literal_chain_S", np.array([S]), self.S, self.tol_S, scale=0.5)
        within(rep, label, "literal_chain_loss", np.array([loss]), self.loss, self.tol_loss, scale=0.5)
        within(rep, label, "literal_chain_dz", dz, self.dz, self.tol_dz, scale=0.5)


def nll_ref(rep, label, z, y, mg):
    ref = NllRef(z, y, mg)
    if on_twin():
        ref.literal(rep, label)
    return ref


def nll_run(rep, entry, ref, offs=(0, 0, 0), null=(), pows=None, label=None):
    """One launch of `entry` ("fused", "tick" or "fwd_bwd") on ref's inputs; returns the raw outputs for bit comparisons.
    `null` names the outputs passed as NULL ("stats", "loss", "dz")."""
    L = lib()
    T, z, y, mg = ref.T, ref.z, ref.y, ref.mg
    m, c = z.shape
    code = CODE[np.dtype(T).name]
    label = label or "%s/%dx%d/mg%d/%s/null=%s" % (entry, m, c, mg, ",".join(map(str, offs)), "+".join(sorted(null)) or "-")
    dz_, dy_ = Dev(z, off=offs[0]), Dev(y, off=offs[1])
    d_dz = None if "dz" in null else Dev(n=m * c, dtype=T, off=offs[2])
    d_loss = None if "loss" in null else Dev(n=1, dtype=T, off=offs[2] % 2)
    d_stats = Dev(ref.stats, off=offs[0] % 2) if entry == "fwd_bwd" else None if "stats" in null else Dev(n=2, dtype=T, off=offs[1] % 2)
    if entry == "fused":
        ok = call(rep, label, L.softmax_nll_fused, dz_.ptr, dy_.ptr, m, c, ptr(d_stats), ptr(d_loss), ptr(d_dz), code)
    elif entry == "tick":
        ok = call(rep, label, L.softmax_nll_fused_tick, dz_.ptr, dy_.ptr, m, c, mg, 0, ptr(d_stats), ptr(d_loss), ptr(d_dz), code,
                  ptr(pows), B1, B2)
    else:
        ok = call(rep, label, L.softmax_nll_fwd_bwd, dz_.ptr, dy_.ptr, m, c, mg, d_stats.ptr, ptr(d_loss), ptr(d_dz), code)
    out = {}
    if not ok:
        return out
    same_bits(rep, label, "z", dz_, z)
    same_bits(rep, label, "y", dy_, y)
    if entry == "fwd_bwd":
        same_bits(rep, label, "stats", d_stats, ref.stats)
    elif d_stats is not None:
        got, bad = d_stats.read()
        rep.guard(label + "/stats", bad)
        rep.bits(label + "/stats[0]", got[:1], ref.stats[:1])
        within(rep, label, entry + "_stats1", got[1:], ref.S, ref.tol_S)
        out["stats"] = got
    if d_loss is not None:
        got, bad = d_loss.read()
        rep.guard(label + "/loss", bad)
        within(rep, label, entry + "_loss", got, ref.loss, ref.tol_loss)
        out["loss"] = got
    if d_dz is not None:
        got, bad = d_dz.read()
        rep.guard(label + "/dz", bad)
        within(rep, label, entry + "_dz", got, ref.dz, ref.tol_dz)
        out["dz"] = got
    return out


SCALES = [(1.5, 0.0), (0.5, -7.5), (1.0, 30.0), (1.0, 300.0), (1.5, -100.0)]      # (sigma, level): the loss knows no level


def _nll_case(rep, rs, k, m, c, T, mg_factor=1):
    scale, shift = SCALES[k % 5]
    z, y = nll_inputs(rs, m, c, T, onehot=k % 2 == 0, scale=scale, shift=shift)
    return nll_ref(rep, "%dx%d" % (m, c), z, y, m * mg_factor)


def family_nll_rows(dtype):
    """tnn_softmax_nll_fused, rows form (c <= 16, m <= 1024): 1, 2, 3, 15, 16 waves with a partly dead last wave, every
    class count, and for f32 the LDS-staged path (m > 128, m c <= 10240, m c % 4 == 0, 16-byte bases) with each of its
    exits."""
    rep = Report("nll_rows", dtype)
    rs = np.random.RandomState(1101)
    k = 0
    for m in (1, 63, 64, 65, 128, 129, 192, 960, 1023, 1024):
        for c in (1, 2, 10, 15, 16):
            ref = _nll_case(rep, rs, k, m, c, dtype)
            nll_run(rep, "fused", ref, offs=(0, 0, 0) if k % 3 else (k % 4, (k + 1) % 4, (k + 2) % 4))
            if (m, c) in ((1, 1), (65, 10)):
                for null in (("dz",), ("loss",), ("stats",), ("dz", "loss", "stats")):
                    nll_run(rep, "fused", ref, null=null)
            k += 1
    # the staged path and each exit: m c % 4 != 0, too big, an aligned shape at base offset 1 (z, y, dz in turn), dz = NULL
    for m, c in ((129, 4), (256, 10), (1024, 10), (129, 3), (1024, 16)):
        ref = _nll_case(rep, rs, k, m, c, dtype)
        k += 1
        nll_run(rep, "fused", ref)
        if (m, c) == (256, 10):
            for offs in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
                nll_run(rep, "fused", ref, offs=offs)
        if (m, c) in ((256, 10), (129, 3)):
            for null in (("dz",), ("loss",), ("stats",), ("dz", "stats"), ("dz", "loss", "stats")):
                nll_run(rep, "fused", ref, null=null)
    finish(rep)


def family_nll_elem(dtype):
    """tnn_softmax_nll_fused, element-parallel form (c > 16: 256 threads below 512 elements, 1024 from there, up to 4096 f32 /
    2048 f64 elements) and the fall-through to the multi-launch form above it (with the temporary stats buffer)."""
    rep = Report("nll_elem", dtype)
    rs = np.random.RandomState(1102)
    shapes = [(1, 17), (30, 17), (31, 17), (240, 17), (241, 17), (120, 17), (121, 17), (1, 4096), (64, 64), (37, 100), (1025, 10)]
    for k, (m, c) in enumerate(shapes):
        ref = _nll_case(rep, rs, k, m, c, dtype)
        nll_run(rep, "fused", ref)
        nll_run(rep, "fused", ref, offs=(1, 2, 3))
        if (m, c) in ((30, 17), (37, 100), (241, 17), (1025, 10)):
            for null in (("stats",), ("dz",), ("loss",), ("dz", "stats"), ("loss", "stats")):
                nll_run(rep, "fused", ref, null=null)
    finish(rep)


def family_nll_tick(dtype):
    """tnn_softmax_nll_fused_tick called directly: with a powers pointer the pair is advanced exactly once and the outputs are
    the bits of the call without it; what does not fit one workgroup is refused with nothing written."""
    rep = Report("nll_tick", dtype)
    rs = np.random.RandomState(1103)
    L = lib()
    code = CODE[dtype]
    p0 = np.array([B1 * B1, B2 * B2 * B2, 0.0, 0.0])
    for k, (m, c) in enumerate([(1, 1), (128, 10), (256, 10), (1024, 16), (30, 17), (20, 100), (120, 17)]):
        ref = _nll_case(rep, rs, k, m, c, dtype)
        plain = nll_run(rep, "tick", ref)
        pows = Dev(p0)
        ticked = nll_run(rep, "tick", ref, pows=pows, label="tick/%dx%d/pows" % (m, c))
        powers_are(rep, "tick/%dx%d advanced once" % (m, c), pows, p0[0] * B1, p0[1] * B2)
        for name in sorted(plain):
            if name in ticked:
                rep.bits("tick/%dx%d/%s with and without pows" % (m, c, name), ticked[name], plain[name])
    refusals = [("1025x10", 1025, 10, 1025, code), ("m_global != m", 8, 10, 16, code), ("m = 0", 0, 10, 0, code),
                ("integer dtype", 8, 10, 8, _lib.I64)]
    if dtype == "float32":
        refusals.append(("241x17", 241, 17, 241, code))
    else:
        refusals.append(("121x17", 121, 17, 121, code))
    for what, m, c, mg, cd in refusals:
        n = max(m * c, 80)
        zz, yy = rs.standard_normal(n).astype(dtype), rs.rand(n).astype(dtype)
        dz_, dy_, pows = Dev(zz), Dev(yy), Dev(p0)
        outs = [Dev(n=2, dtype=dtype), Dev(n=1, dtype=dtype), Dev(n=n, dtype=dtype)]
        rep.raises("tick refuses " + what, lambda: L.softmax_nll_fused_tick(dz_.ptr, dy_.ptr, m, c, mg, 0, outs[0].ptr, outs[1].ptr,
                                                                          outs[2].ptr, cd, pows.ptr, B1, B2))
        for name, d in zip(("stats", "loss", "dz"), outs):
            same_bits(rep, "tick refuses " + what, name, d, np.full(d.n, d.image[0], d.dt))
        same_bits(rep, "tick refuses " + what, "pows", pows, p0)
    finish(rep)


def family_nll_stats(dtype):
    """tnn_softmax_nll_stats: one block up to 2048 elements, block pairs merged above, the grid capped at 1024 blocks."""
    rep = Report("nll_stats", dtype)
    rs = np.random.RandomState(1104)
    L = lib()
    T = np.dtype(dtype).type
    eps = LD(np.finfo(T).eps)
    for k, n in enumerate((1, 2047, 2048, 2049, 1024 * 2048 + 5)):
        scale, shift = SCALES[k % 5]
        z, _ = nll_inputs(rs, n, 1, dtype, onehot=True, scale=scale, shift=shift)
        zl = z.astype(LD).ravel()
        M = zl.max()
        x = M - zl
        e = np.exp(-x)
        S = e.sum()
        tol_S = eps * ((e * (x / 2 + 2)).sum() / S + 4) * S
        if on_twin():
            with np.errstate(all="ignore"):
                lit = np.exp(z - z.max()).sum()
            within(rep, "stats/%d" % n, "literal_chain_S", np.array([lit]), S, tol_S, scale=0.5)
        for off, (m, c) in ((0, (n, 1)), (1, (1, n))):
            label = "stats/%dx%d/%d" % (m, c, off)
            dz_, out = Dev(z, off=off), Dev(n=2, dtype=dtype, off=off)
            if not call(rep, label, L.softmax_nll_stats, dz_.ptr, m, c, out.ptr, CODE[dtype]):
                continue
            same_bits(rep, label, "z", dz_, z)
            got, bad = out.read()
            rep.guard(label, bad)
            rep.bits(label + "/stats[0]", got[:1], np.array([M]).astype(T))
            within(rep, label, "stats1", got[1:], S, tol_S)
    finish(rep)


def family_lse_merge(dtype):
    """tnn_lse_merge: one wave over n_shards pairs, shards that saw nothing ({-inf, 0}) among them."""
    rep = Report("lse_merge", dtype)
    rs = np.random.RandomState(1105)
    L = lib()
    T = np.dtype(dtype).type
    eps = LD(np.finfo(T).eps)
    cases = [(n, "dense") for n in (1, 2, 63, 64, 65, 200)] + [(n, "some_empty") for n in (2, 65, 200)] + [(65, "one_live")]
    for n, kind in cases:
        Ms = (rs.standard_normal(n) * 8 + 3).astype(T)
        Ms = np.maximum(Ms, T(Ms.max() - T(MAX_SPREAD - 1)))
        Ss = (1 + rs.rand(n) * 2000).astype(T)
        if kind == "some_empty":
            dead = rs.permutation(n)[:max(1, n // 3)]
            Ms[dead], Ss[dead] = -np.inf, 0
        elif kind == "one_live":
            keep = rs.randint(n)
            dead = np.arange(n) != keep
            Ms[dead], Ss[dead] = -np.inf, 0
        both = np.stack([Ms, Ss], axis=1)
        live = np.isfinite(Ms)
        M = Ms[live].astype(LD).max()
        x = M - Ms[live].astype(LD)
        terms = Ss[live].astype(LD) * np.exp(-x)
        S = terms.sum()
        tol_S = eps * ((terms * (x / 2 + 2)).sum() / S + 4) * S
        if on_twin():
            with np.errstate(all="ignore"):
                lit = (Ss[live] * np.exp(Ms[live] - Ms[live].max())).sum()
            within(rep, "lse_merge/%d/%s" % (n, kind), "literal_chain_S", np.array([lit]), S, tol_S, scale=0.5)
        for off in (0, 1):
            label = "lse_merge/%d/%s/%d" % (n, kind, off)
            d_in, out = Dev(both, off=off), Dev(n=2, dtype=dtype, off=(off + 1) % 2)
            if not call(rep, label, L.lse_merge, d_in.ptr, n, out.ptr, CODE[dtype]):
                continue
            same_bits(rep, label, "stats_all", d_in, both)
            got, bad = out.read()
            rep.guard(label, bad)
            rep.bits(label + "/stats[0]", got[:1], np.array([M]).astype(T))
            within(rep, label, "stats1", got[1:], S, tol_S)
    rep.raises("lse_merge refuses 0 shards", lambda: L.lse_merge(d_in.ptr, 0, out.ptr, CODE[dtype]))
    finish(rep)


def family_nll_fwd_bwd(dtype):
    """tnn_softmax_nll_fwd_bwd alone, stats taken from the reference: one block up to 256 rows, block partials above, the grid
    capped at 1024 blocks; m_global = m and 3 m."""
    rep = Report("nll_fwd_bwd", dtype)
    rs = np.random.RandomState(1106)
    k = 0
    for m, c in ((1, 10), (255, 10), (256, 10), (257, 10), (1024 * 256 + 3, 2)):
        for factor in (1, 3):
            ref = _nll_case(rep, rs, k, m, c, dtype, mg_factor=factor)
            k += 1
            nll_run(rep, "fwd_bwd", ref, offs=(0, 0, 0) if factor == 1 else (1, 2, 3))
            # the one-block launch has only loss_out to write its loss to; the NULL-loss case therefore uses the multi-block one
            nll_run(rep, "fwd_bwd", ref, null=("dz",) if m <= 256 else ("loss",))
    finish(rep)


# ------------------------------------------------------------------------------------------- running-error arithmetic
class RE(object):
    """A longdouble value and a first-order bound of how far the evaluation in dtype T (unit roundoff `u` charged in
    full, `tiny` for a flushed denormal) can be from it."""

    __array_ufunc__ = None                 # a numpy scalar on the left defers to the reflected operators below

    def __init__(self, val, err, u, tiny):
        self.val, self.err, self.u, self.tiny = val, err, u, tiny

    @classmethod
    def exact(cls, x, T):
        fi = np.finfo(T)
        x = np.asarray(x)
        assert x.dtype == np.dtype(T)
        return cls(x.astype(LD), np.zeros(x.shape, LD), LD(fi.eps), LD(fi.tiny))

    def _lift(self, o):
        return o if isinstance(o, RE) else RE(LD(o), LD(0), self.u, self.tiny)

    def _op(self, val, prop):
        return RE(val, prop + self.u * np.abs(val) + self.tiny, self.u, self.tiny)

    def __neg__(self):
        return RE(-self.val, self.err, self.u, self.tiny)

    def __add__(self, o):
        o = self._lift(o)
        return self._op(self.val + o.val, self.err + o.err)

    def __sub__(self, o):
        o = self._lift(o)
        return self._op(self.val - o.val, self.err + o.err)

    def __mul__(self, o):
        o = self._lift(o)
        return self._op(self.val * o.val, np.abs(self.val) * o.err + np.abs(o.val) * self.err)

    __radd__, __rmul__ = __add__, __mul__

    def __truediv__(self, o):
        o = self._lift(o)
        val = self.val / o.val
        return self._op(val, (self.err + np.abs(val) * o.err) / np.abs(o.val))

    def __rtruediv__(self, o):
        return self._lift(o) / self

    def sqrt(self):
        val = np.sqrt(self.val)
        up = np.sqrt(self.val + self.err) - val
        down = val - np.sqrt(np.maximum(self.val - self.err, 0))
        return self._op(val, np.maximum(up, down))


def check_re(rep, label, entry, got, ref):
    within(rep, label, entry, got, ref.val, ref.err)


def grads(rs, n, T, against=None):
    """Gradients with zeros, +-tiny and, where a running moment is given, values of mixed sign against it, some placed so that
    b1 m + (1 - b1) g cancels."""
    T = np.dtype(T).type
    g = (rs.standard_normal(n) * 0.1).astype(T)
    tiny = np.finfo(T).tiny
    pos = rs.permutation(n)
    k = min(n, 4)
    g[pos[:k]] = np.array([0.0, tiny, -tiny, -0.0], T)[:k]
    if against is not None and n >= 8:
        k = pos[4:4 + max(1, n // 16)]
        g[k] = (-B1 / (1 - B1) * against[k].astype(np.float64)).astype(T)
    return g


# --------------------------------------------------------------------------------------------------------------- MSE
def family_mse(dtype):
    """tnn_mse_fwd_bwd / _tick: one block, a partly filled second block, the grid capped at 1024 blocks."""
    rep = Report("mse", dtype)
    rs = np.random.RandomState(1107)
    L = lib()
    T = np.dtype(dtype).type
    code = CODE[dtype]
    eps = LD(np.finfo(T).eps)
    p0 = np.array([B1, B2 * B2, 0.0, 0.0])
    for n in (1, 255, 256, 257, 1024 * 256 + 1):
        pred, y = mixed(rs, n, T, with_specials=False), mixed(rs, n, T, with_specials=False, scale=0.5)
        y[::5] = pred[::5]                                       # exact zeros of the difference
        e = RE.exact(pred, T) - RE.exact(y, T)
        e_t = (pred - y).astype(LD)                              # the difference as the dtype rounds it: one IEEE operation
        for mg in (1, 7):
            two_inv_m = T(2.0 * (1.0 / mg))                      # as the entry point rounds it
            dpred = LD(two_inv_m) * e
            loss = (e_t * e_t).sum() / mg
            tol_loss = (n * LD(2.0) ** -52 + eps) * loss
            for off, null, tick in ((0, (), False), (1, ("dpred",), False), (2, (), True), (3, ("loss",), False)):
                label = "mse/%d/mg%d/off%d/null=%s%s" % (n, mg, off, "+".join(null) or "-", "/tick" if tick else "")
                d_p, d_y = Dev(pred, off=off), Dev(y, off=(off + 1) % 4)
                d_d = None if "dpred" in null else Dev(n=n, dtype=T, off=(off + 2) % 4)
                d_l = None if "loss" in null else Dev(n=1, dtype=T, off=off % 2)
                d_l2, pows = (Dev(n=1, dtype=T, off=1), Dev(p0)) if tick else (None, None)
                if tick:
                    ok = call(rep, label, L.mse_fwd_bwd_tick, d_p.ptr, d_y.ptr, n, mg, d_l.ptr, d_l2.ptr, ptr(d_d), code, pows.ptr, B1, B2)
                else:
                    ok = call(rep, label, L.mse_fwd_bwd, d_p.ptr, d_y.ptr, n, mg, ptr(d_l), ptr(d_d), code)
                if not ok:
                    continue
                same_bits(rep, label, "pred", d_p, pred)
                same_bits(rep, label, "y", d_y, y)
                if d_d is not None:
                    got, bad = d_d.read()
                    rep.guard(label + "/dpred", bad)
                    check_re(rep, label, "dpred", got, dpred)
                if d_l is not None:
                    got, bad = d_l.read()
                    rep.guard(label + "/loss", bad)
                    within(rep, label, "loss", got, loss, tol_loss)
                if tick:
                    got2, bad = d_l2.read()
                    rep.guard(label + "/loss_out2", bad)
                    rep.bits(label + "/loss_out2 equals loss_out", got2, got)
                    powers_are(rep, label + " advanced once", pows, p0[0] * B1, p0[1] * B2)
    d_p, d_y, d_l2, d_d, pows = Dev(pred[:8]), Dev(y[:8]), Dev(n=1, dtype=T), Dev(n=8, dtype=T), Dev(p0)
    rep.raises("mse_tick refuses loss_out2 without loss_out",
               lambda: L.mse_fwd_bwd_tick(d_p.ptr, d_y.ptr, 8, 8, None, d_l2.ptr, d_d.ptr, code, pows.ptr, B1, B2))
    same_bits(rep, "mse_tick refusal", "loss_out2", d_l2, np.full(1, d_l2.image[0], T))
    same_bits(rep, "mse_tick refusal", "dpred", d_d, np.full(8, d_d.image[0], T))
    same_bits(rep, "mse_tick refusal", "pows", pows, p0)
    finish(rep)


# --------------------------------------------------------------------------------------------------- SGD, optim_step
def _optim_oracle(kind, T, g, s1, s2, lr, a, b, eps):
    """One step in the kernels' operation order; hyperparameters rounded as tnn_optim_step rounds them."""
    lr, a, b, eps = LD(T(lr)), T(a), LD(T(b)), LD(T(eps))
    one_m_a = LD(T(1) - a)                                       # a single operation in the dtype: reproduced, not bounded
    a = LD(a)
    if kind == _lib.OPT_MOMENTUM:
        s1 = a * s1 + g
        step = (-lr) * s1
    elif kind == _lib.OPT_RMSPROP:
        s1 = s1 + one_m_a * (g * g - s1)
        s2 = b * s2 + lr * g / (s1 + eps).sqrt()
        step = -s2
    elif kind == _lib.OPT_ADAGRAD:
        s1 = s1 + g * g
        step = -(lr / (s1 + eps).sqrt()) * g
    else:
        s1 = s1 + one_m_a * (g * g - s1)
        delta = g * ((s2 + eps).sqrt() / (s1 + eps).sqrt())
        step = (-lr) * delta
        s2 = s2 + one_m_a * (delta * delta - s2)
    return step, s1, s2


def family_optim(dtype):
    """tnn_sgd and tnn_optim_step (Momentum, RMSProp, Adagrad, Adadelta): p given, step_out given, both; three consecutive steps;
    one block, two, and one element more than a pass of the capped grid covers."""
    rep = Report("optim", dtype)
    rs = np.random.RandomState(1108)
    L = lib()
    T = np.dtype(dtype).type
    code = CODE[dtype]
    sizes = (1, 255, 257, device_limits()["pass_scalar"] + 1)
    lr = 0.0123
    for n in sizes:
        p0 = mixed(rs, n, T, with_specials=False)
        gs = [grads(rs, n, T) for _ in range(3)]
        # SGD: p = p + (-lr g)
        for off in (0, 1):
            d_p = Dev(p0, off=off)
            ref = RE.exact(p0, T)
            for t, g in enumerate(gs):
                label = "sgd/%d/off%d/step%d" % (n, off, t + 1)
                d_g = Dev(g, off=(off + 2) % 4)
                ref = ref + (-LD(T(lr))) * RE.exact(g, T)
                if not call(rep, label, L.sgd, d_p.ptr, d_g.ptr, n, lr, code):
                    break
                same_bits(rep, label, "g", d_g, g)
                got, bad = d_p.read()
                rep.guard(label, bad)
                check_re(rep, label, "sgd_p", got, ref)
        for kind, name, (a, b, eps) in ((_lib.OPT_MOMENTUM, "momentum", (0.9, 0.0, 0.0)), (_lib.OPT_RMSPROP, "rmsprop", (0.9, 0.5, 1e-8)),
                                        (_lib.OPT_ADAGRAD, "adagrad", (0.0, 0.0, 1e-8)), (_lib.OPT_ADADELTA, "adadelta", (0.9, 0.0, 1e-6))):
            two = kind in (_lib.OPT_RMSPROP, _lib.OPT_ADADELTA)
            s1_0 = np.abs(mixed(rs, n, T, with_specials=False, scale=0.01))
            s2_0 = np.abs(mixed(rs, n, T, with_specials=False, scale=0.01))
            s1_0[::7] = 0
            s2_0[::5] = 0
            modes = [("p", 0), ("step", 1), ("both", 2)]
            devs = {}
            for mode, off in modes:
                devs[mode] = {"p": Dev(p0, off=off) if mode != "step" else None, "s1": Dev(s1_0, off=(off + 1) % 4),
                              "s2": Dev(s2_0, off=(off + 3) % 4) if two else None,
                              "step": Dev(n=n, dtype=T, off=(off + 2) % 4) if mode != "p" else None}
            r_p, r_s1, r_s2 = RE.exact(p0, T), RE.exact(s1_0, T), RE.exact(s2_0, T)
            for t, g in enumerate(gs):
                r_step, r_s1, r_s2 = _optim_oracle(kind, T, RE.exact(g, T), r_s1, r_s2, lr, a, b, eps)
                r_p = r_p + r_step
                for mode, off in modes:
                    d = devs[mode]
                    if d is None:
                        continue
                    label = "%s/%d/%s/step%d" % (name, n, mode, t + 1)
                    d_g = Dev(g, off=off)
                    if not call(rep, label, L.optim_step, kind, ptr(d["p"]), d_g.ptr, d["s1"].ptr, ptr(d["s2"]), ptr(d["step"]), n,
                                lr, a, b, eps, code):
                        devs[mode] = None
                        continue
                    same_bits(rep, label, "g", d_g, g)
                    for what, ref in (("p", r_p), ("s1", r_s1), ("s2", r_s2), ("step", r_step)):
                        if d[what] is not None:
                            got, bad = d[what].read()
                            rep.guard(label + "/" + what, bad)
                            check_re(rep, label, "%s_%s" % (name, what), got, ref)
    # refusals: the second state vector of RMSProp / Adadelta, an unknown kind; nothing written
    g, s = grads(rs, 8, T), np.abs(mixed(rs, 8, T, with_specials=False))
    for what, kind, has_s2 in (("rmsprop without s2", _lib.OPT_RMSPROP, False), ("adadelta without s2", _lib.OPT_ADADELTA, False),
                               ("kind 4", 4, True), ("kind -1", -1, True)):
        d_p, d_g, d_s1, d_s2, d_st = Dev(s), Dev(g), Dev(s), Dev(s), Dev(n=8, dtype=T)
        rep.raises("optim_step refuses " + what, lambda: L.optim_step(kind, d_p.ptr, d_g.ptr, d_s1.ptr, d_s2.ptr if has_s2 else None,
                                                                       d_st.ptr, 8, lr, 0.9, 0.5, 1e-8, code))
        for nm, d in (("p", d_p), ("s1", d_s1), ("s2", d_s2)):
            same_bits(rep, "optim_step refuses " + what, nm, d, s)
        same_bits(rep, "optim_step refuses " + what, "step_out", d_st, np.full(8, d_st.image[0], T))
    finish(rep)


# -------------------------------------------------------------------------------------------------------------- Adam
def _adam_oracle(T, g, p, m, v, lr, eps, p1, p2):
    """core/optimizer.py:67-79 in the kernel's order; p1, p2 are the float64 powers of the step.  The bias corrections are
    float64 operations followed by one cast: reproduced bit for bit."""
    b1, b2 = T(B1), T(B2)
    c1, c2 = LD(T(1) - b1), LD(T(1) - b2)
    ic1, ic2 = LD(T(1.0 / (1.0 - p1))), LD(T(1.0 / (1.0 - p2)))
    m = m + c1 * (g - m)
    v = v + c2 * (g * g - v)
    step = (-LD(T(lr))) * (m * ic1) / ((v * ic2).sqrt() + LD(T(eps)))
    return step, p + step, m, v


class _AdamRun(object):
    """One device-side trajectory: its own p, m, v (and step_out) at one base offset, and its own powers."""

    def __init__(self, name, p0, m0, v0, off, step_out):
        T = p0.dtype
        self.name, self.off, self.alive = name, off, True
        self.p0 = p0
        self.p, self.m, self.v = Dev(p0, off=off), Dev(m0, off=off), Dev(v0, off=off)
        self.step = Dev(n=p0.size, dtype=T, off=off) if step_out else None
        self.pows = Dev(np.array([1.0, 1.0, 0.0, 0.0]))


def _adam_sizes(rep, rs, dtype, sizes, lr=1e-3, eps=1e-8):
    """Three steps at every n.  Trajectories: `aligned` (tnn_adam on steps 1 and 3, tnn_adam_ex with the scalar riding along on
    step 2: for f32 up to 2^20 elements the launch advances the powers itself, above that the prologue does), `offset1` (every
    base one element off: the scalar kernel behind the prologue, scalar on step 1), and at the sizes marked so `step_out`
    (advance = 0 against powers set by hand: p and the powers untouched)."""
    L = lib()
    T = np.dtype(dtype).type
    code = CODE[dtype]
    for n, which in sizes:
        p0, m0 = mixed(rs, n, T, with_specials=False), mixed(rs, n, T, with_specials=False, scale=0.05)
        v0 = np.abs(mixed(rs, n, T, with_specials=False, scale=0.01))
        v0[::9] = 0
        runs = [_AdamRun(w, p0, m0, v0, {"aligned": 0, "offset1": 1, "step_out": 0, "step_out_offset3": 3}[w], w.startswith("step_out"))
                for w in which]
        r_p, r_m, r_v = RE.exact(p0, T), RE.exact(m0, T), RE.exact(v0, T)
        p1 = p2 = 1.0
        m_now = m0
        for t in (1, 2, 3):
            g = grads(rs, n, T, against=m_now)
            p1, p2 = p1 * B1, p2 * B2                            # the sequential float64 products
            r_step, r_p, r_m, r_v = _adam_oracle(T, RE.exact(g, T), r_p, r_m, r_v, lr, eps, p1, p2)
            m_now = r_m.val.astype(T)
            src = np.array([1.25 + t], T)
            for run in runs:
                if not run.alive:
                    continue
                label = "adam/%d/%s/step%d" % (n, run.name, t)
                d_g = Dev(g, off=run.off)
                d_src, d_dst = Dev(src, off=run.off % 2), Dev(n=1, dtype=T, off=(run.off + 1) % 2)
                scalar = False
                if run.step is not None:                         # advance = 0: the powers are given, and stay
                    run.pows = Dev(np.array([p1, p2, 0.0, 0.0]))
                    scalar = t == 3
                    ok = call(rep, label, L.adam_ex, run.p.ptr, d_g.ptr, run.m.ptr, run.v.ptr, n, lr, B1, B2, eps, run.pows.ptr,
                              run.step.ptr, code, 0, d_src.ptr if scalar else None, d_dst.ptr if scalar else None)
                elif (run.name == "aligned" and t == 2) or (run.name == "offset1" and t == 1):
                    scalar = True
                    ok = call(rep, label, L.adam_ex, run.p.ptr, d_g.ptr, run.m.ptr, run.v.ptr, n, lr, B1, B2, eps, run.pows.ptr,
                              None, code, 1, d_src.ptr, d_dst.ptr)
                else:
                    ok = call(rep, label, L.adam, run.p.ptr, d_g.ptr, run.m.ptr, run.v.ptr, n, lr, B1, B2, eps, run.pows.ptr,
                              None, code)
                if not ok:
                    run.alive = False
                    continue
                same_bits(rep, label, "g", d_g, g)
                # powers: the sequential products, bit for bit; the self-advance ticket word back to zero
                powers_are(rep, label, run.pows, p1, p2)
                same_bits(rep, label, "scalar_src", d_src, src)
                same_bits(rep, label, "scalar_dst", d_dst, src if scalar else np.full(1, d_dst.image[0], T))
                for what, dev, ref in (("m", run.m, r_m), ("v", run.v, r_v)):
                    got, bad = dev.read()
                    rep.guard(label + "/" + what, bad)
                    check_re(rep, label, "adam_" + what, got, ref)
                if run.step is not None:
                    got, bad = run.step.read()
                    rep.guard(label + "/step_out", bad)
                    check_re(rep, label, "adam_step_out", got, r_step)
                    same_bits(rep, label, "p", run.p, run.p0)
                else:
                    got, bad = run.p.read()
                    rep.guard(label + "/p", bad)
                    check_re(rep, label, "adam_p", got, r_p)


def family_adam(dtype):
    """tnn_adam / tnn_adam_ex / tnn_adam_tick at the small sizes: below, at and above one float4, a float4 body with a tail, and
    (f32) more float4 work than the 128 workgroups of the self-advancing launch cover in one pass."""
    rep = Report("adam", dtype)
    rs = np.random.RandomState(1109)
    L = lib()
    T = np.dtype(dtype).type
    code = CODE[dtype]
    every = ("aligned", "offset1", "step_out", "step_out_offset3")
    sizes = [(n, every) for n in (1, 3, 4, 5, 1023)]
    if dtype == "float32":
        sizes.append((128 * 256 * 4 + 4, ("aligned", "offset1", "step_out")))
    _adam_sizes(rep, rs, dtype, sizes)
    # tnn_adam_tick: the pair times {b1, b2}, the other two words untouched
    pows = Dev(np.array([1.0, 1.0, 0.0, 0.0]))
    q1 = q2 = 1.0
    for t in range(4):
        if call(rep, "adam_tick/%d" % t, L.adam_tick, pows.ptr, B1, B2):
            q1, q2 = q1 * B1, q2 * B2
            powers_are(rep, "adam_tick/%d" % t, pows, q1, q2)
    rep.raises("adam_tick refuses NULL", lambda: L.adam_tick(None, B1, B2))
    # refusals: a scalar source without a destination (and the reverse), no powers
    x = np.abs(mixed(rs, 8, T, with_specials=False))
    for what, has_src, has_dst, has_pows in (("scalar_src without scalar_dst", True, False, True),
                                             ("scalar_dst without scalar_src", False, True, True), ("no pows", False, False, False)):
        d = [Dev(x) for _ in range(4)]
        d_src, d_dst, pows = Dev(x[:1]), Dev(n=1, dtype=T), Dev(np.array([B1, B2, 0.0, 0.0]))
        rep.raises("adam_ex refuses " + what,
                   lambda: L.adam_ex(d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, 8, 1e-3, B1, B2, 1e-8, pows.ptr if has_pows else None, None,
                                     code, 1, d_src.ptr if has_src else None, d_dst.ptr if has_dst else None))
        for name, dev in (("p", d[0]), ("m", d[2]), ("v", d[3])):
            same_bits(rep, "adam_ex refuses " + what, name, dev, x)
        same_bits(rep, "adam_ex refuses " + what, "scalar_dst", d_dst, np.full(1, d_dst.image[0], T))
        same_bits(rep, "adam_ex refuses " + what, "pows", pows, np.array([B1, B2, 0.0, 0.0]))
    finish(rep)


def family_adam_large(dtype):
    """f32 at the switch between the launch that advances the powers itself (n <= 2^20, 128 workgroups walking the arena) and the
    prologue launch in front of a full grid (2^20 + 5: float4 body with a tail), and the scalar kernel past one pass of its
    capped grid."""
    rep = Report("adam_large", dtype)
    rs = np.random.RandomState(1110)
    lim = device_limits()
    assert (2 ** 20 + 5) * 4 <= BUFFER_LIMIT
    _adam_sizes(rep, rs, dtype, [(2 ** 20, ("aligned", "offset1")), (2 ** 20 + 5, ("aligned", "offset1")),
                                 (lim["pass_scalar"] + 3, ("offset1",))])
    finish(rep)


# -------------------------------------------------------------------------------------------------------- host layer
def family_host(dtype):
    """ops.softmax_nll_ and SoftmaxCrossEntropyLoss(fused=True) on a transposed, non-contiguous logits view, one shape per kernel
    form, against the same oracle: the loss and t.grad."""
    import tinynn_autograd_amd as tn
    from tinynn_autograd_amd import device_array as da
    from tinynn_autograd_amd.core import ops
    from tinynn_autograd_amd.core.losses import SoftmaxCrossEntropyLoss
    from tinynn_autograd_amd.core.tensor import Tensor
    rep = Report("host", dtype)
    rs = np.random.RandomState(1111)
    T = np.dtype(dtype).type
    tn.set_default_float(T)
    try:
        # rows form, its staged path, element-parallel, multi-launch (rows above 1024; elements above the one-workgroup cap)
        for k, (m, c) in enumerate([(128, 10), (256, 10), (37, 100), (1025, 10), (241, 17)]):
            ref = _nll_case(rep, rs, k, m, c, dtype)
            for how in ("ops", "layer"):
                label = "host/%s/%dx%d" % (how, m, c)
                zt = da.asarray(np.ascontiguousarray(ref.z.T), dtype=T).T          # [m, c] view of a [c, m] buffer
                t = Tensor(zt, requires_grad=True)
                rep.checks += 1
                if t.values.shape != (m, c) or np.asarray(t.values).dtype != np.dtype(T):
                    rep._fail(label, "the logits view has shape %s dtype %s" % (t.values.shape, np.asarray(t.values).dtype))
                    continue
                try:
                    loss = ops.softmax_nll_(t, Tensor(ref.y)) if how == "ops" else SoftmaxCrossEntropyLoss(fused=True).loss(t, Tensor(ref.y))
                    loss.backward()
                    got_loss, got_grad = np.asarray(loss.values), np.asarray(t.grad)
                except _lib.TnnError as exc:
                    rep._fail(label, "raised %s" % exc)
                    continue
                rep.checks += 1
                if got_loss.dtype != np.dtype(T) or got_grad.dtype != np.dtype(T) or got_grad.shape != (m, c):
                    rep._fail(label, "loss %s, grad %s %s" % (got_loss.dtype, got_grad.dtype, got_grad.shape))
                    continue
                within(rep, label, "host_loss", got_loss, ref.loss, ref.tol_loss)
                within(rep, label, "host_grad", got_grad, ref.dz, ref.tol_dz)
    finally:
        tn.set_default_float(np.float32)
    finish(rep)


# --------------------------------------------------------------------------------------------------------- registry
FAMILIES = {
    "nll_rows": (family_nll_rows, FLOATS),
    "nll_elem": (family_nll_elem, FLOATS),
    "nll_tick": (family_nll_tick, FLOATS),
    "nll_stats": (family_nll_stats, FLOATS),
    "lse_merge": (family_lse_merge, FLOATS),
    "nll_fwd_bwd": (family_nll_fwd_bwd, FLOATS),
    "mse": (family_mse, FLOATS),
    "optim": (family_optim, FLOATS),
    "adam": (family_adam, FLOATS),
    "adam_large": (family_adam_large, ("float32",)),
    "host": (family_host, FLOATS),
}
CASES = sorted("%s-%s" % (family, dtype) for family, (_, dtypes) in FAMILIES.items() for dtype in dtypes)


def run_case(case):
    family, dtype = case.rsplit("-", 1)
    FAMILIES[family][0](dtype)
