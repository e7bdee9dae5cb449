"""Optimizers (reference: core/optimizer.py:6-164).

Same contract as the reference: `compute_step(grads, params)` flattens every gradient in layer order
(dict order "w", "b"), calls `_compute_step(flat)` and hands back per-parameter steps that the caller
ADDS to the parameters (core/model.py:59-61).  All state lives in HBM.

  * When the gradients are views into one flat arena (Model binds them that way) the flatten is a
    zero-copy view (core/optimizer.py:14-15 is a concatenate copy in the reference).
  * `Adam` / `SGD` compute the step with ONE fused kernel (tnn_adam with step_out / tnn_ewise_scalar)
    instead of 13 / 1 array expressions; `fused=False` evaluates the reference's literal expressions
    through DeviceArray arithmetic — the two are parity-tested against each other and the oracle.
  * Adam's epsilon is added OUTSIDE the square root, after bias correction (core/optimizer.py:77).
  * `AdamW` (not in the reference) adds decoupled weight decay, clipping by the global gradient norm, learning-rate schedules
    and a non-finite guard, with every per-step quantity in a device record (include/tnn_ostep.h, ostep.py): a whole step
    captures into a graph.  `weight_decay` of every OTHER optimizer stays stored and unused.
"""

import ctypes
import weakref

import numpy as np

from .. import _lib
from .. import device_array as da
from .. import ostep


class BaseOptimizer(object):

    def __init__(self, lr, weight_decay):
        self.lr = lr
        self.weight_decay = weight_decay      # stored, unused (the reference's use is commented out, :28-29) — except by AdamW
        self._last_flat_step = None

    def compute_step(self, grads, params):
        flat_grad = np.concatenate([np.ravel(g) for layer in grads for g in layer.values()])
        flat_step = self._compute_step(flat_grad)
        self._last_flat_step = flat_step
        steps, offset = [], 0
        for layer in params:
            restored = {}
            for key, p in layer.items():
                count = int(np.prod(p.shape))
                restored[key] = flat_step[offset:offset + count].reshape(p.shape)
                offset += count
            steps.append(restored)
        return steps

    def _compute_step(self, grad):
        raise NotImplementedError

    def apply_flat(self, params, grads):
        """Optional fast path for `Model.step` when parameters and gradients live in flat arenas: update `params`
        in place from `grads` in ONE pass (same maths as compute_step followed by `param += step`,
        core/model.py:56-61) and return True; return False to take the compute_step route."""
        return False


class SGD(BaseOptimizer):
    """step = -lr * g (core/optimizer.py:46-47)"""

    def __init__(self, lr, weight_decay=0.0):
        super().__init__(lr, weight_decay)

    def _compute_step(self, grad):
        return -self.lr * grad

    def apply_flat(self, params, grads):
        if not _flat_pair_ok(params, grads):
            return False
        _lib.get().sgd(params._ptr, grads._ptr, grads.size, self.lr, grads._code())
        return True


_TICKED = weakref.WeakSet()       # Adam instances whose powers a loss launch has advanced for a step that has not run yet


def take_capture_ticks():
    """End of a hipGraph capture (graph.py): the optimizers whose powers a loss launch INSIDE the captured function advances
    while the step that consumes the advance is NOT part of it.  Nothing has executed yet, so their `_ticked` flags are
    cleared here; the captured function sets them after every replay (the replay's loss launch has then really advanced the
    powers and the eager step that follows must not advance them again — exact, no extra launch in the graph).  A captured
    WHOLE step has consumed its tick: nothing to hand over."""
    # the capture is closed: the eager advances its own launches superseded are taken back NOW (nothing of the captured function
    # has executed, so the order "eager advance, roll back, replay advances" is what the device sees)
    for opt in _ROLLBACK:
        if opt._pows is not None:
            _lib.get().adam_tick(opt._pows._ptr, 1.0 / opt._b1, 1.0 / opt._b2)
    del _ROLLBACK[:]
    out = [opt for opt in list(_TICKED) if opt._ticked and opt._tick_captured and opt._pows is not None]
    for opt in out:
        opt._ticked = opt._tick_captured = False
        _TICKED.discard(opt)
    return out


_ROLLBACK = []                    # Adam instances whose pending EAGER advance was superseded inside the open capture


def settle_eager_ticks():
    """Start of a hipGraph capture (graph.py).  An advance that an EAGER loss launch has made and no step has consumed yet (a
    warm-up call of a loss-only function, ANOTHER model's pending loss) is NOT touched here: only an optimizer that ticks or
    steps again inside the captured function has its eager advance taken back — lazily, see `Adam._supersede_eager_tick` and
    `take_capture_ticks` — so capturing one model never perturbs the bias-correction powers of an unrelated one."""
    del _ROLLBACK[:]              # (left over from an aborted capture)


def _flat_pair_ok(params, grads):
    return (isinstance(params, da.DeviceArray) and isinstance(grads, da.DeviceArray) and params.shape == grads.shape
            and params.dtype == grads.dtype and params.dtype.kind == "f" and params.ndim == 1
            and not params._t and not grads._t and params._hv is None and grads._hv is None)


class Adam(BaseOptimizer):
    """reference: core/optimizer.py:50-79"""

    def __init__(self, lr=0.001, beta1=0.9, beta2=0.999, epsilon=1e-8, weight_decay=0.0, fused=True):
        super().__init__(lr, weight_decay)
        self._b1, self._b2, self._eps = beta1, beta2, epsilon
        self.fused = fused
        self._t = 0
        self._m = 0
        self._v = 0
        self._pows = None      # device double[4]: {b1^(t-1), b2^(t-1), ticket, pad}
        self._ticked = False   # the powers have ALREADY been advanced for the coming step (by the loss launch, see take_tick)
        self._tick_captured = False   # ... by a launch recorded into an open hipGraph capture (not executed yet)

    def _compute_step(self, grad):
        self._t += 1
        if self.fused and isinstance(grad, da.DeviceArray) and grad.dtype.kind == "f":
            return self._fused_step(grad._contig())
        self._m += (1.0 - self._b1) * (grad - self._m)
        self._v += (1.0 - self._b2) * (grad ** 2 - self._v)
        m_hat = self._m / (1 - self._b1 ** self._t)
        v_hat = self._v / (1 - self._b2 ** self._t)
        return -self.lr * m_hat / (v_hat ** 0.5 + self._eps)

    def _supersede_eager_tick(self):
        """Inside an open hipGraph capture with an EAGER advance of the powers still pending (a loss evaluated before the capture
        whose step never ran): the captured function must record its OWN advance — a replay cannot live on one that happened
        once, outside the graph — so the eager one is forgotten here and taken back when the capture closes
        (`take_capture_ticks`; 1 / b is not the exact inverse in float64: an ulp at most, on this optimizer only)."""
        if self._ticked and not self._tick_captured and _lib.capturing:
            self._ticked = False
            _ROLLBACK.append(self)

    def apply_flat(self, params, grads):
        if not (self.fused and _flat_pair_ok(params, grads)):
            return False
        self._t += 1
        self._ensure_state(grads)
        self._supersede_eager_tick()
        if self._ticked:                             # the loss launch advanced the powers for this step
            _lib.get().adam_ex(params._ptr, grads._ptr, self._m._ptr, self._v._ptr, grads.size, self.lr, self._b1, self._b2,
                               self._eps, self._pows._ptr, None, grads._code(), 0, None, None)
            self._ticked = False
        else:
            _lib.get().adam(params._ptr, grads._ptr, self._m._ptr, self._v._ptr, grads.size, self.lr, self._b1, self._b2,
                            self._eps, self._pows._ptr, None, grads._code())
        return True

    def take_tick(self):
        """For the loss launch of a training step (ops._softmax_head): (powers pointer, b1, b2) if that launch should advance
        the bias-correction powers for the coming step — once per optimizer step, however many losses are evaluated in
        between — else None.  The whole-step trainer does the same in its head launch; it is what lets the step's LAST launch
        carry the optimizer (apply_with_first_layer) without a launch or an arrival counter for the advance."""
        if self.fused and self._pows is not None:
            self._supersede_eager_tick()
        if not self.fused or self._pows is None or self._ticked:
            return None
        self._ticked = True
        self._tick_captured = bool(_lib.capturing)
        _TICKED.add(self)
        return self._pows._ptr, self._b1, self._b2

    def untick(self):
        """Take back an advance of the powers that no step has consumed (a loss-only hipGraph replayed twice in a row: its loss
        launch advances unconditionally).  The multiplication by 1 / b is not the exact inverse in float64 — an ulp at most,
        on this rare path only."""
        if self._ticked and self._pows is not None:
            _lib.get().adam_tick(self._pows._ptr, 1.0 / self._b1, 1.0 / self._b2)
        self._ticked = False

    def apply_with_first_layer(self, params, grads, rows, n_in, n_out, x, dz):
        """The backward of the model's FIRST Dense layer (deferred by Model, core/model.py) and the Adam step over the whole
        arena in ONE launch (tnn_dense_bwd_first_adam): dW = x^T dz and db = column sums of dz are written to the head of
        `grads` (the layer's arena views) and consumed in the same launch.  Returns False if this optimizer cannot."""
        if not (self.fused and _flat_pair_ok(params, grads)) or grads.dtype != np.float32:
            return False
        self._ensure_state(grads)
        self._supersede_eager_tick()
        lib = _lib.get()
        if not self._ticked:                         # no loss launch advanced the powers: a launch of its own
            lib.adam_tick(self._pows._ptr, self._b1, self._b2)
        self._t += 1
        self._ticked = False
        esz = grads.dtype.itemsize
        nw, nb = n_in * n_out, n_out
        rest = nw + nb
        pp, gp, mp, vp = params._ptr, grads._ptr, self._m._ptr, self._v._ptr
        lib.dense_bwd_first_adam(rows, n_in, n_out, x._ptr, dz._ptr, gp, gp + nw * esz, pp, mp, vp, pp + nw * esz,
                                 mp + nw * esz, vp + nw * esz, pp + rest * esz, gp + rest * esz, mp + rest * esz,
                                 vp + rest * esz, grads.size - rest, self.lr, self._b1, self._b2, self._eps,
                                 self._pows._ptr, grads._code())
        return True

    def _ensure_state(self, grad):
        if self._pows is None:
            self._m = da.zeros(grad.shape, grad.dtype)
            self._v = da.zeros(grad.shape, grad.dtype)
            self._pows = da.asarray(np.array([1.0, 1.0, 0.0, 0.0]), dtype=np.float64)

    def _fused_step(self, grad):
        lib = _lib.get()
        self._ensure_state(grad)
        step = da.empty(grad.shape, grad.dtype)
        self._supersede_eager_tick()
        if self._ticked:                             # see take_tick
            lib.adam_ex(None, grad._ptr, self._m._ptr, self._v._ptr, grad.size, self.lr, self._b1, self._b2,
                        self._eps, self._pows._ptr, step._ptr, grad._code(), 0, None, None)
            self._ticked = False
        else:
            lib.adam(None, grad._ptr, self._m._ptr, self._v._ptr, grad.size, self.lr, self._b1, self._b2,
                     self._eps, self._pows._ptr, step._ptr, grad._code())
        return step


class _FusedStateOptimizer(BaseOptimizer):
    """Momentum / RMSProp / Adagrad / Adadelta: the state vectors live in HBM next to the flat gradient and one
    kernel (tnn_optim_step) reads g + state, writes state + step.  `fused=False`, or a gradient that is not a float
    DeviceArray, takes the reference's array expressions instead (same maths through DeviceArray arithmetic)."""
    _kind = None
    _n_state = 1

    def __init__(self, lr, weight_decay=0.0, fused=True):
        super().__init__(lr, weight_decay)
        self.fused = fused
        self._state = None

    def _hyper(self):               # (a, b, eps) of tnn_optim_step
        raise NotImplementedError

    def _array_step(self, grad):
        raise NotImplementedError

    def _compute_step(self, grad):
        if not (self.fused and isinstance(grad, da.DeviceArray) and grad.dtype.kind == "f"):
            return self._array_step(grad)
        grad = grad._contig()
        step = da.empty(grad.shape, grad.dtype)
        self._launch(None, grad, step)
        return step

    def _launch(self, params, grad, step):
        if self._state is None:
            self._state = [da.zeros(grad.shape, grad.dtype) for _ in range(self._n_state)]
        a, b, eps = self._hyper()
        s2 = self._state[1]._ptr if self._n_state > 1 else None
        _lib.get().optim_step(self._kind, params._ptr if params is not None else None, grad._ptr,
                              self._state[0]._ptr, s2, step._ptr if step is not None else None, grad.size, self.lr,
                              a, b, eps, grad._code())

    def apply_flat(self, params, grads):
        if not (self.fused and _flat_pair_ok(params, grads)):
            return False
        self._launch(params, grads, None)
        return True


class Momentum(_FusedStateOptimizer):
    """acc = momentum * acc + g; step = -lr * acc (core/optimizer.py:111-124)"""
    _kind = _lib.OPT_MOMENTUM

    def __init__(self, lr, momentum=0.9, weight_decay=0.0, fused=True):
        super().__init__(lr, weight_decay, fused)
        self._momentum = momentum
        self._acc = 0

    def _hyper(self):
        return self._momentum, 0.0, 0.0

    def _array_step(self, grad):
        self._acc = self._momentum * self._acc + grad
        return -self.lr * self._acc


class RMSProp(_FusedStateOptimizer):
    """reference: core/optimizer.py:82-108"""
    _kind = _lib.OPT_RMSPROP
    _n_state = 2

    def __init__(self, lr=0.01, decay=0.99, momentum=0.0, epsilon=1e-8, weight_decay=0.0, fused=True):
        super().__init__(lr, weight_decay, fused)
        self._decay, self._momentum, self._eps = decay, momentum, epsilon
        self._ms = 0
        self._mom = 0

    def _hyper(self):
        return self._decay, self._momentum, self._eps

    def _array_step(self, grad):
        self._ms += (1 - self._decay) * (grad ** 2 - self._ms)
        self._mom = self._momentum * self._mom + self.lr * grad / (self._ms + self._eps) ** 0.5
        return -self._mom


class Adagrad(_FusedStateOptimizer):
    """reference: core/optimizer.py:127-142"""
    _kind = _lib.OPT_ADAGRAD

    def __init__(self, lr, weight_decay=0.0, epsilon=1e-8, fused=True):
        super().__init__(lr, weight_decay, fused)
        self._G = 0
        self._eps = epsilon

    def _hyper(self):
        return 0.0, 0.0, self._eps

    def _array_step(self, grad):
        self._G += grad ** 2
        return -(self.lr / (self._G + self._eps) ** 0.5) * grad


class Adadelta(_FusedStateOptimizer):
    """reference: core/optimizer.py:145-164"""
    _kind = _lib.OPT_ADADELTA
    _n_state = 2

    def __init__(self, lr=1.0, weight_decay=0.0, decay=0.9, epsilon=1e-8, fused=True):
        super().__init__(lr, weight_decay, fused)
        self._eps, self._decay = epsilon, decay
        self._Eg = 0
        self._delta = 0

    def _hyper(self):
        return self._decay, 0.0, self._eps

    def _array_step(self, grad):
        self._Eg += (1 - self._decay) * (grad ** 2 - self._Eg)
        std = (self._delta + self._eps) ** 0.5
        delta = grad * (std / (self._Eg + self._eps) ** 0.5)
        self._delta += (1 - self._decay) * (delta ** 2 - self._delta)
        return -self.lr * delta


def default_no_decay(layer_index, layer, name):
    """AdamW's default: a parameter is NOT decayed when the last component of its name starts with "b" or is "gamma" or
    "beta" — biases and norm gains / offsets ("b", "attn.bq", "ln1.gamma", "ln2.beta"); everything else is decayed."""
    last = name.rpartition(".")[2]
    return last.startswith("b") or last in ("gamma", "beta")


class AdamW(BaseOptimizer):
    """Adam with DECOUPLED weight decay, clipping by the global gradient norm, a learning-rate schedule and a non-finite guard,
    all resident on the device (include/tnn_ostep.h, the planner is ostep.py):

        g' = g coef,  coef = min(1, max_norm / (gnorm + 1e-6))          gnorm: the L2 norm over EVERY parameter's gradient
        m += (1 - b1)(g' - m);  v += (1 - b2)(g' g' - v)
        p  = p (1 - lr wd)  (decayed parameters only);  p += -lr (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps)

    which is torch.optim.AdamW behind torch.nn.utils.clip_grad_norm_.  t, the powers, lr, the norm, coef and the skip flag
    live in one 8-double record in HBM that the step's own launches advance: sum of squares (one double per workgroup),
    one small launch for the norm / tick / schedule, ONE update launch over the whole arena.  Nothing is read back, so a
    whole step captures into a graph (tn.capture) and every replay sees its own step count and learning rate.

    schedule     None (constant lr), ostep.Cosine(warmup, total, min_lr) or ostep.Linear(warmup, total, min_lr)
    no_decay     predicate (layer_index, layer, name) -> bool; default `default_no_decay`
    skip_nonfinite  a step whose gradient norm is inf / NaN changes nothing: p, m, v keep their bits, t stays, `skipped` counts
    fused=False  (and the CPU test twin) take the composed route: the same maths on DeviceArray arithmetic with an uploaded
                 0 / wd vector and the norm read back on the host.  Not capturable: it raises inside an open capture.

    Data parallel: Model.step all-reduces the gradient arena BEFORE the optimizer runs, so the norm is the global one on
    every rank and every rank takes the same decision, with no further communication.

    Derives from BaseOptimizer, not Adam, and has neither apply_with_first_layer nor take_tick on purpose: Model must not
    defer the first layer's backward into a launch that cannot see the global norm.

    Out of scope: the whole-step trainers (tnn_mlp.cpp), the bf16 master-weight path and the sharded optimizer, folding the
    update into GEMM epilogues, per-parameter norms, and decay for the other optimizers."""

    def __init__(self, lr=1e-3, beta1=0.9, beta2=0.999, epsilon=1e-8, weight_decay=0.01, max_norm=None, schedule=None,
                 no_decay=None, skip_nonfinite=True, fused=True):
        super().__init__(lr, weight_decay)
        self._os = ostep               # the planner: record layout, runs, schedules, the host form of launch (b)
        self._b1, self._b2, self._eps = beta1, beta2, epsilon
        if max_norm is not None and not float(max_norm) >= 0.0:
            raise ValueError("AdamW: max_norm must be None or a number >= 0, got %r" % (max_norm,))
        self.max_norm = None if max_norm is None else float(max_norm)
        if schedule is not None and not isinstance(schedule, ostep.Schedule):
            raise TypeError("AdamW: schedule must be None, ostep.Cosine(...) or ostep.Linear(...), got %r" % (schedule,))
        self.schedule = schedule if schedule is not None else ostep.Constant()
        self.no_decay = no_decay if no_decay is not None else default_no_decay
        self.skip_nonfinite = bool(skip_nonfinite)
        self.fused = fused
        self._runs = None          # (starts, flags) of the bound layout
        self._layout_n = None
        self._m = self._v = None
        self._rec = None           # native: the device record
        self._ws = None            # native: one double per workgroup of the norm launch
        self._runs_dev = None      # native: the run table, uploaded once per layout
        self._wd_vec = None        # composed: wd where decayed, 0 elsewhere
        self._host_rec = None      # composed: the record on the host
        self.route = None          # the route the last step took

    # ------------------------------------------------------------------ layout
    def bind_layout(self, segments):
        """segments: (offset, count, layer_index, layer, name) in arena order (Model binds them).  Decides which parameters
        decay and merges neighbours into runs; the device table is uploaded at the next step."""
        segments = list(segments)
        flags = [not self.no_decay(li, layer, name) for _o, _c, li, layer, name in segments]
        self._runs = self._os.decay_runs([(o, c) for o, c, _li, _l, _n in segments], flags)
        self._layout_n = sum(int(c) for _o, c, _li, _l, _n in segments)
        self._runs_dev = self._wd_vec = None

    def has_layout(self):
        return self._runs is not None

    def decay_runs(self):
        """(starts, flags) of the bound layout, or None."""
        return self._runs

    def _layout_for(self, n):
        if self._runs is None or self._layout_n != n:
            if self._runs is not None:
                raise ValueError("AdamW: the bound layout covers %d elements, the step %d" % (self._layout_n, n))
            # no layout was bound (the optimizer used without a Model): one run, decayed — torch's default
            self._runs = self._os.decay_runs([(0, n)], [True])
            self._layout_n = n
        return self._runs

    def _hyper(self):
        return self._os.Hyper(lr=self.lr, b1=self._b1, b2=self._b2, eps=self._eps, wd=self.weight_decay,
                              max_norm=self.max_norm, schedule=self.schedule, guard=self.skip_nonfinite)

    # ------------------------------------------------------------------ the step
    def apply_flat(self, params, grads):
        if not _flat_pair_ok(params, grads):
            return False
        self._step(params, grads, None)
        return True

    def compute_step(self, grads, params):
        """The reference's contract with the parameters flattened too (decay needs them): per-parameter steps that the caller
        ADDS.  Without a bound layout the names come from `params` itself (the layer object passed to no_decay is None)."""
        flat_grad = np.concatenate([np.ravel(g) for layer in grads for g in layer.values()])
        flat_par = np.concatenate([np.ravel(p.values) for layer in params for p in layer.values()])
        if self._runs is None:
            segs, off = [], 0
            for li, layer in enumerate(params):
                for key, p in layer.items():
                    count = int(np.prod(p.shape))
                    segs.append((off, count, li, None, key))
                    off += count
            self.bind_layout(segs)
        if not (isinstance(flat_grad, da.DeviceArray) and isinstance(flat_par, da.DeviceArray)
                and flat_grad.dtype == flat_par.dtype and flat_grad.dtype.kind == "f"):
            raise TypeError("AdamW: float32 / float64 device parameters and gradients of one dtype are needed")
        # zeros, not empty: a skipped (non-finite) step writes NOTHING to step_out, and the caller adds it to the parameters
        flat_step = da.zeros(flat_grad.shape, flat_grad.dtype)
        self._step(flat_par._contig(), flat_grad._contig(), flat_step)
        self._last_flat_step = flat_step
        steps, offset = [], 0
        for layer in params:
            restored = {}
            for key, p in layer.items():
                count = int(np.prod(p.shape))
                restored[key] = flat_step[offset:offset + count].reshape(p.shape)
                offset += count
            steps.append(restored)
        return steps

    def _step(self, p, g, step_out):
        n = g.size
        starts, flags = self._layout_for(n)
        lib = _lib.get()
        plan = self._os.plan_ostep(n, g.dtype, self.max_norm, self.skip_nonfinite, native=lib.has_ostep,
                                   route=None if self.fused else "composed")
        if self.route is not None and plan.route != self.route:
            raise RuntimeError("AdamW: the route changed from %s to %s between steps" % (self.route, plan.route))
        self.route = plan.route
        if self._m is None:
            self._m = da.zeros(g.shape, g.dtype)
            self._v = da.zeros(g.shape, g.dtype)
        if self._m.size != n or self._m.dtype != g.dtype or p.size != n or p.dtype != g.dtype:
            raise ValueError("AdamW: the state covers %d %s elements, the step %d %s (parameters %d %s)"
                             % (self._m.size, self._m.dtype.name, n, g.dtype.name, p.size, p.dtype.name))
        if plan.route == "composed":
            return self._composed_step(p, g, step_out, plan)
        if self._rec is None:
            self._rec = da.asarray(self._os.initial_state(self.lr), dtype=np.float64)
            self._ws = da.empty((max(plan.grid, 1),), np.float64)
        if self._runs_dev is None:
            self._runs_dev = da.asarray(self._os.run_table(starts, flags), dtype=np.int64)
        code, sch = g._code(), self.schedule
        ws = None
        if plan.need_norm and n:
            lib.ostep_sumsq(g._ptr, n, self._ws._ptr, self._ws.nbytes, code)
            ws = self._ws._ptr
        lib.ostep_begin(self._rec._ptr, ws, n, -1.0 if self.max_norm is None else self.max_norm, int(self.skip_nonfinite),
                        self._b1, self._b2, sch.kind, self.lr, sch.min_lr, sch.warmup, sch.total)
        lib.ostep_adamw(p._ptr, g._ptr, self._m._ptr, self._v._ptr, step_out._ptr if step_out is not None else None, n,
                        self._rec._ptr, self._runs_dev._ptr, len(starts), self._b1, self._b2, self._eps, self.weight_decay, code)

    def _composed_step(self, p, g, step_out, plan):
        if _lib.capturing:
            raise RuntimeError("AdamW (composed route) reads the gradient norm back to the host, which a graph capture "
                               "cannot do; use fused=True on libtnn_hip.so")
        os_ = self._os
        if self._host_rec is None:
            self._host_rec = os_.initial_state(self.lr)
        gnorm = 0.0
        if plan.need_norm and plan.n:
            g64 = g.astype(np.float64)
            gnorm = float(np.sqrt(float((g64 * g64).sum())))                 # the read-back
        st = self._host_rec = os_.begin_from_norm(self._host_rec, gnorm, self._hyper())
        if st[os_.SKIP] != 0.0:
            if step_out is not None:
                step_out.fill(0.0)
            return
        ty = g.dtype.type
        if self._wd_vec is None:
            self._wd_vec = da.asarray(os_.decay_vector(plan.n, self._runs, self.weight_decay, g.dtype), dtype=g.dtype)
        coef, lr = float(ty(st[os_.COEF])), float(ty(st[os_.LR]))
        one_m_b1, one_m_b2 = float(ty(1) - ty(self._b1)), float(ty(1) - ty(self._b2))
        inv_c1, inv_c2 = float(ty(1.0 / (1.0 - st[os_.B1_POW]))), float(ty(1.0 / (1.0 - st[os_.B2_POW])))
        gc = g * coef
        self._m += one_m_b1 * (gc - self._m)
        self._v += one_m_b2 * (gc * gc - self._v)
        upd = (-lr) * (self._m * inv_c1) / (da.sqrt(self._v * inv_c2) + float(ty(self._eps)))
        new_p = p * (1.0 - self._wd_vec * lr) + upd
        if step_out is not None:
            step_out[...] = new_p - p
        else:
            p[...] = new_p

    # ------------------------------------------------------------------ the record
    def state(self):
        """The record as a dict (ostep.STATE_NAMES).  The only read-back of this optimizer: it synchronises."""
        if self._rec is not None:
            return self._os.state_dict(np.asarray(self._rec))
        return self._os.state_dict(self._host_rec if self._host_rec is not None else self._os.initial_state(self.lr))

    def last_norm(self):
        return self.state()["gnorm"]

    def lr_now(self):
        return self.state()["lr"]
