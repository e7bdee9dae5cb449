"""Host planner of the device-resident optimizer step (numpy only, no device import): the state record, the decay runs, the
grid and workspace sizes, the learning-rate schedules and one AdamW step of csrc/tnn_ostep.hip in numpy.

State record (include/tnn_ostep.h)
    A device double[8], created as {1, 1, 0, lr0, 0, 1, 0, 0}: b1^t, b2^t, t (steps applied), lr (this step's learning rate),
    gnorm (global L2 norm of the last gradient before clipping), coef (the factor the gradient is multiplied by), skipped
    (steps skipped so far), skip (1 if THIS step is skipped).  Everything that changes from step to step is in it, so a
    captured graph replays the right step.

One step
    (a) sumsq   one float64 partial per workgroup            only with a max_norm or the non-finite guard
    (b) begin   norm, skip, coef = min(1, max_norm / (gnorm + 1e-6)), the tick, lr = schedule(t)
    (c) adamw   g' = g coef;  m += (1 - b1)(g' - m);  v += (1 - b2)(g' g' - v)
                p = p (1 - lr wd_run);  p += -lr (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps)
    (d) scale   g *= coef: (a) + (b) + (d) are a stand-alone clip_grad_norm
    A non-finite norm skips the step: nothing is written, t and the powers stay, `skipped` counts.

Routes
    native    csrc/tnn_ostep.hip.  Needs the entry points and float32 / float64 operands.  Capturable: nothing is read back.
    composed  the same maths on DeviceArray arithmetic with an uploaded 0 / wd vector and the norm READ BACK on the host.
              What runs under the CPU test twin and with `fused=False`.  Not capturable.
"""

import math

import numpy as np

THREADS = 256             # TNN_OSTEP_THREADS
VEC = 16                  # TNN_OSTEP_VEC: bytes per lane of a wide access
MAX_BLOCKS = 2048         # TNN_OSTEP_MAX_BLOCKS: most workgroups of a data launch
STATE_DOUBLES = 8         # TNN_OSTEP_STATE_DOUBLES
B1_POW, B2_POW, T, LR, GNORM, COEF, SKIPPED, SKIP = range(8)        # TNN_OSTEP_B1_POW .. TNN_OSTEP_SKIP
STATE_NAMES = ("b1_pow", "b2_pow", "t", "lr", "gnorm", "coef", "skipped", "skip")
SCHED_CONST, SCHED_COSINE, SCHED_LINEAR = 0, 1, 2                   # TNN_OSTEP_SCHED_*
CLIP_EPS = 1e-6           # torch's clip_grad_norm_: coef = max_norm / (gnorm + 1e-6), clamped to 1
ROUTES = ("native", "composed")

_FLOATS = (np.dtype(np.float32), np.dtype(np.float64))


# ------------------------------------------------------------------------------------------------ schedules
class Schedule(object):
    """base: the optimizer's lr.  value(t, base) is the float64 learning rate of step t (t = 1 is the first step)."""
    kind = SCHED_CONST
    warmup = 0
    total = 0
    min_lr = 0.0

    def value(self, t, base):
        return schedule_lr(self.kind, float(base), self.min_lr, self.warmup, self.total, t)

    def __repr__(self):
        return "%s(warmup=%d, total=%d, min_lr=%r)" % (type(self).__name__, self.warmup, self.total, self.min_lr)


class Constant(Schedule):
    """lr = base."""


class _Decaying(Schedule):
    def __init__(self, warmup, total, min_lr=0.0):
        warmup, total = int(warmup), int(total)
        if warmup < 0 or total < 0:
            raise ValueError("%s: warmup and total must be >= 0, got %d and %d" % (type(self).__name__, warmup, total))
        self.warmup, self.total, self.min_lr = warmup, total, float(min_lr)


class Cosine(_Decaying):
    """Linear warm-up lr = base t / warmup for t <= warmup, then
    lr = min_lr + 0.5 (base - min_lr)(1 + cos(pi min(1, (t - warmup) / (total - warmup)))): min_lr from `total` on."""
    kind = SCHED_COSINE


class Linear(_Decaying):
    """The same warm-up, then a straight line down to min_lr at `total`, constant afterwards."""
    kind = SCHED_LINEAR


def schedule_lr(kind, base, min_lr, warmup, total, t):
    """The schedule at step t in float64: the arithmetic of tnn_ostep_begin, operation for operation."""
    base, min_lr, warmup, total, t = float(base), float(min_lr), float(warmup), float(total), float(t)
    if kind == SCHED_CONST:
        return base
    if warmup > 0.0 and t <= warmup:
        return base * t / warmup
    frac = (t - warmup) / (total - warmup) if total > warmup else 1.0
    frac = min(frac, 1.0)
    if kind == SCHED_COSINE:
        return min_lr + 0.5 * (base - min_lr) * (1.0 + math.cos(math.pi * frac))
    if kind == SCHED_LINEAR:
        return min_lr + (base - min_lr) * (1.0 - frac)       # (exactly min_lr from `total` on)
    raise ValueError("unknown schedule kind %r" % (kind,))


# ------------------------------------------------------------------------------------------------ record, runs, geometry
def initial_state(lr0):
    """The record as the host creates it: {1, 1, 0, lr0, 0, 1, 0, 0}."""
    return np.array([1.0, 1.0, 0.0, float(lr0), 0.0, 1.0, 0.0, 0.0], dtype=np.float64)


def state_dict(state):
    state = np.asarray(state, dtype=np.float64).reshape(STATE_DOUBLES)
    return {name: float(state[i]) for i, name in enumerate(STATE_NAMES)}


def decay_runs(segments, flags):
    """segments: (offset, count) pairs in ascending, gap-free order from 0; flags: decay yes / no per segment.  Returns
    (starts int64 [R], flags int64 [R]): empty segments dropped, neighbours with the same flag merged; run r covers
    [starts[r], starts[r + 1]) and the last ends at the total.  No element at all: one run at 0, not decayed."""
    segments, flags = list(segments), list(flags)
    if len(segments) != len(flags):
        raise ValueError("decay_runs: %d segments, %d flags" % (len(segments), len(flags)))
    starts, out, at = [], [], 0
    for (offset, count), flag in zip(segments, flags):
        offset, count, flag = int(offset), int(count), 1 if flag else 0
        if count < 0 or offset != at:
            raise ValueError("decay_runs: segment (%d, %d) does not continue at %d" % (offset, count, at))
        if count == 0:
            continue
        if not out or out[-1] != flag:
            starts.append(offset)
            out.append(flag)
        at += count
    if not starts:
        starts, out = [0], [0]
    return np.array(starts, dtype=np.int64), np.array(out, dtype=np.int64)


def run_table(starts, flags):
    """The device table of tnn_ostep_adamw: int64 [2 R], the starts followed by the flags."""
    return np.concatenate([np.asarray(starts, dtype=np.int64), np.asarray(flags, dtype=np.int64)])


def decay_vector(n, runs, wd, dtype=np.float64):
    """[n] with wd where the element's run decays and 0 elsewhere (what the composed route uploads)."""
    starts, flags = runs
    ends = list(starts[1:]) + [n]
    out = np.zeros(n, dtype=dtype)
    for s, e, f in zip(starts, ends, flags):
        if f:
            out[int(s):int(e)] = wd
    return out


def grid(n):
    """Workgroups of a data launch over n elements (0: no launch): a function of n alone."""
    n = int(n)
    if n < 0:
        raise ValueError("ostep: n must be >= 0, got %d" % n)
    blocks = (n + 3) // 4
    return min((blocks + THREADS - 1) // THREADS, MAX_BLOCKS)


def workspace_bytes(n):
    """One double per workgroup of the sumsq launch (tnn_ostep_workspace)."""
    return grid(n) * 8


def clip_coef(gnorm, max_norm):
    """min(1, max_norm / (gnorm + 1e-6)) in float64; 1 without a max_norm."""
    if max_norm is None:
        return 1.0
    coef = float(max_norm) / (float(gnorm) + CLIP_EPS)        # (a NaN norm gives a NaN factor, as on the device)
    return 1.0 if coef > 1.0 else coef


# ------------------------------------------------------------------------------------------------ the plan
class OstepPlan(object):
    __slots__ = ("n", "dtype", "route", "need_norm", "max_norm", "guard", "grid", "workspace_bytes", "launches")

    def __repr__(self):
        return "OstepPlan(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.__slots__)


def plan_ostep(n, dtype=np.float32, max_norm=None, skip_nonfinite=True, native=True, float_ok=True, route=None):
    """The plan of one step over n elements.  native: the library has the entry points; route: force one, None picks."""
    if route is not None and route not in ROUTES:
        raise ValueError("route must be one of %s or None, got %r" % (ROUTES, route))
    if max_norm is not None and not float(max_norm) >= 0.0:
        raise ValueError("max_norm must be None or a number >= 0, got %r" % (max_norm,))
    dtype = np.dtype(dtype)
    can = bool(native) and bool(float_ok) and dtype in _FLOATS
    if route == "native" and not can:
        raise ValueError("the native optimizer-step route needs libtnn_hip.so and float32 / float64 operands, got dtype %s"
                         % dtype.name)
    plan = OstepPlan()
    plan.n, plan.dtype = int(n), dtype
    plan.route = route or ("native" if can else "composed")
    plan.max_norm = None if max_norm is None else float(max_norm)
    plan.guard = bool(skip_nonfinite)
    plan.need_norm = plan.max_norm is not None or plan.guard
    plan.grid = grid(plan.n)
    plan.workspace_bytes = workspace_bytes(plan.n) if plan.need_norm else 0
    plan.launches = (("sumsq",) if plan.need_norm and plan.n else ()) + ("begin",) + (("adamw",) if plan.n else ())
    return plan


# ------------------------------------------------------------------------------------------------ the reference step
class Hyper(object):
    """The hyper-parameters of one step, as the entry points take them."""

    def __init__(self, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.01, max_norm=None, schedule=None, guard=True):
        self.lr, self.b1, self.b2, self.eps, self.wd = float(lr), float(b1), float(b2), float(eps), float(wd)
        self.max_norm = None if max_norm is None else float(max_norm)
        self.schedule = schedule if schedule is not None else Constant()
        self.guard = bool(guard)

    def need_norm(self):
        return self.max_norm is not None or self.guard


def begin(state, g, hyper):
    """Launches (a) + (b) in numpy: the new record from the old one and the gradient (float64 throughout)."""
    if hyper.need_norm():
        g64 = np.asarray(g).astype(np.float64).ravel()
        with np.errstate(all="ignore"):
            gnorm = float(np.sqrt(np.sum(g64 * g64)))
    else:
        gnorm = 0.0
    return begin_from_norm(state, gnorm, hyper)


def begin_from_norm(state, gnorm, hyper):
    """Launch (b) in numpy: the new record from the old one and the norm (0.0 when none was taken)."""
    st = np.array(state, dtype=np.float64).reshape(STATE_DOUBLES)
    gnorm = float(gnorm)
    skip = hyper.guard and not math.isfinite(gnorm)
    coef = clip_coef(gnorm, hyper.max_norm)
    if not skip:
        st[T] += 1.0
        st[B1_POW] *= hyper.b1
        st[B2_POW] *= hyper.b2
    else:
        st[SKIPPED] += 1.0
    st[LR] = hyper.schedule.value(st[T], hyper.lr)
    st[GNORM], st[COEF], st[SKIP] = gnorm, coef, 1.0 if skip else 0.0
    return st


def reference(p, g, m, v, state, hyper, runs):
    """One whole step in numpy: returns (p, m, v, state) after it.  The record is float64; the update is evaluated in the
    operand dtype with one rounding per operation, where the kernel rounds (the two bias corrections are formed in float64 and
    applied as one multiplication each)."""
    p, g, m, v = (np.asarray(a) for a in (p, g, m, v))
    dt = p.dtype
    if dt not in _FLOATS or g.dtype != dt or m.dtype != dt or v.dtype != dt:
        raise ValueError("reference: p, g, m, v of one dtype, float32 or float64")
    st = begin(state, g, hyper)
    if st[SKIP] != 0.0:
        return p.copy(), m.copy(), v.copy(), st
    ty = dt.type
    coef, lr = ty(st[COEF]), ty(st[LR])
    one_m_b1, one_m_b2 = ty(1) - ty(hyper.b1), ty(1) - ty(hyper.b2)
    inv_c1, inv_c2 = ty(1.0 / (1.0 - st[B1_POW])), ty(1.0 / (1.0 - st[B2_POW]))
    wd = decay_vector(p.size, runs, hyper.wd, dt).reshape(p.shape)
    with np.errstate(all="ignore"):
        gc = g * coef
        m = m + one_m_b1 * (gc - m)
        v = v + one_m_b2 * (gc * gc - v)
        upd = -lr * (m * inv_c1) / (np.sqrt(v * inv_c2) + ty(hyper.eps))
        p = p * (ty(1) - lr * wd) + upd
    return p.astype(dt, copy=False), m.astype(dt, copy=False), v.astype(dt, copy=False), st
