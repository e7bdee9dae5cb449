"""Host planner of the gated activations (numpy only, no device import): from the geometry of one call to ONE plan, in the
style of rope.py and norm.py, plus the numpy evaluation of the expressions.

    contract    every operand is viewed as [M, F] through a ROW stride in elements (ld >= F), unit stride along F.
                forward   a = act(gate),  y = a * up            (no up: y = a — a plain activation)
                backward  dup = dy * a,   dgate = (dy * up) * act'(gate)       (no up: dgate = dy * act'(gate))
                The halves of a packed projection z [M, 2 F] are gate = z[:, :F] and up = z[:, F:], read in place with
                ld = 2 F; dgate and dup may likewise be the halves of one dz [M, 2 F].
    acts        "silu"       g * sig(g),  sig = 1 / (1 + exp(-g)) in the overflow-free form of include/tnn_gated.h;
                             act' = sig * (1 + g * (1 - sig)).  With up this is SwiGLU.
                "gelu_tanh"  the tanh form of GELU (norm.py), with up: GEGLU.
                "gelu"       the exact (erf) form.  There is no erf among the generic elementwise operations, so — as for
                             norm.gelu_route — only the native route has it.

Routes
    native    csrc/tnn_gated.hip: ONE tnn_gated_fwd / tnn_gated_bwd launch.  Needs the entry points and float32 / float64.
    composed  the existing elementwise operations (sigmoid or tanh, products, sums) on slices: what runs under the CPU test
              twin and the second, independent implementation the GPU tests compare the kernel with.

Wide or element accesses (include/tnn_gated.h states the rule; `wide_access` is its one Python copy): every used base address
VEC-byte aligned, every used row stride and F multiples of V = VEC / itemsize.

Out of scope: bf16, fusing the gate into a GEMM epilogue, the whole-step trainers, separate w_gate / w_up parameters.
"""

import numpy as np

VEC = 16                  # TNN_GATED_VEC
THREADS = 256             # TNN_GATED_THREADS
MAX_BLOCKS = 2048         # TNN_GATED_MAX_BLOCKS
ACTS = ("silu", "gelu_tanh", "gelu")          # TNN_GATED_SILU, TNN_GATED_GELU_TANH, TNN_GATED_GELU_ERF: the index is the code
ROUTES = ("native", "composed")
FWD_OPERANDS = ("gate", "up", "y")                                  # the order of tnn_gated_fwd's strides
BWD_OPERANDS = ("gate", "up", "dy", "dgate", "dup")                 # ... and of tnn_gated_bwd's
MAX_ELEMENTS = 2 ** 31
_GELU_C, _GELU_A = 0.79788456080286535588, 0.044715


def check_act(act, what="gated"):
    if act not in ACTS:
        raise ValueError("%s: act must be one of %s, got %r" % (what, ACTS, act))
    return act


def gated_hidden(width):
    """The default hidden width of a gated feed-forward block: 8 E / 3 rounded up to a multiple of 8 — three [E, hidden]
    matrices then hold about what the two [E, 4 E] matrices of the plain block do."""
    return -(-(8 * int(width)) // 24) * 8


def wide_access(F, itemsize, lds, addresses):
    """include/tnn_gated.h's rule: True when the kernels take 16-byte accesses.  lds / addresses: those that are used."""
    v = VEC // int(itemsize)
    return int(F) % v == 0 and all(int(s) % v == 0 for s in lds) and all(int(a) % VEC == 0 for a in addresses)


def choose_blocks(items):
    """The library's choice of workgroups for `items` work items (blocks == 0)."""
    return max(1, min(-(-int(items) // THREADS), MAX_BLOCKS))


def outputs_apart(dgate, dup, ld_dgate, ld_dup, M, F, itemsize):
    """include/tnn_gated.h's rule for dgate and dup (byte addresses): disjoint address ranges, or equal row strides and
    F <= ((dup - dgate) mod ld) <= ld - F in elements — the interleaved rows of one array."""
    n_g, n_u = ((M - 1) * ld_dgate + F) * itemsize, ((M - 1) * ld_dup + F) * itemsize
    if dgate + n_g <= dup or dup + n_u <= dgate:
        return True
    if ld_dgate != ld_dup or (dup - dgate) % itemsize:
        return False
    return F <= ((dup - dgate) // itemsize) % ld_dgate <= ld_dgate - F


class GatedPlan(object):
    __slots__ = ("M", "F", "act", "backward", "has_up", "operands", "lds", "blocks", "wide", "chunks", "items", "grid", "route")

    def act_code(self):
        return ACTS.index(self.act)

    def strides(self):
        """The row strides in the order of the entry point's `strides` array (F for an operand that is absent)."""
        return tuple(self.lds.get(name, self.F) for name in (BWD_OPERANDS if self.backward else FWD_OPERANDS))

    def empty(self):
        return self.M == 0

    def __repr__(self):
        return "GatedPlan(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.__slots__)


def plan_gated(M, F, act="silu", backward=False, has_up=True, need_dgate=True, need_dup=True, lds=None, addresses=None,
               blocks=0, itemsize=4, native=True, float_ok=True, route=None):
    """The plan of ONE tnn_gated_fwd (backward=False: operands gate, up, y) or tnn_gated_bwd (gate, up, dy, dgate, dup) call.
    has_up False: the plain activation, no `up` and no `dup`.  need_dgate / need_dup: the outputs of a backward call.
    lds: {operand: row stride in elements}, F where it says nothing.  addresses: {operand: byte address}; an operand it does
    not name is a fresh array — aligned, and disjoint from everything.  blocks: 0 (the library's choice) or 1 .. MAX_BLOCKS.
    Every check of include/tnn_gated.h runs here, before any launch."""
    what = "gated_bwd" if backward else "gated"
    check_act(act, what)
    M, F, itemsize = int(M), int(F), int(itemsize)
    if F < 1:
        raise ValueError("%s: F must be >= 1, got %d" % (what, F))
    if M < 0:
        raise ValueError("%s: M must be >= 0, got %d" % (what, M))
    if M * F >= MAX_ELEMENTS:
        raise ValueError("%s: M %d x F %d is 2^31 elements or more" % (what, M, F))
    p = GatedPlan()
    p.M, p.F, p.act, p.backward, p.has_up = M, F, act, bool(backward), bool(has_up)
    p.blocks = int(blocks)
    if not 0 <= p.blocks <= MAX_BLOCKS:
        raise ValueError("%s: blocks must be 0 (the library's choice) or 1 .. %d, got %d" % (what, MAX_BLOCKS, p.blocks))
    if backward:
        if not has_up and need_dup:
            raise ValueError("%s: the plain activation (no up) has no dup" % what)
        if not (need_dgate or need_dup):
            raise ValueError("%s: neither dgate nor dup is asked for" % what)
        used = ["gate"] + (["up"] if has_up else []) + ["dy"] + (["dgate"] if need_dgate else []) + (["dup"] if need_dup else [])
        outputs = [n for n in ("dgate", "dup") if n in used]
    else:
        used = ["gate"] + (["up"] if has_up else []) + ["y"]
        outputs = ["y"]
    names = BWD_OPERANDS if backward else FWD_OPERANDS
    for given in (lds or {}), (addresses or {}):
        for name in given:
            if name not in names:
                raise ValueError("%s: unknown operand %r (operands: %s)" % (what, name, ", ".join(names)))
    p.operands = tuple(used)
    p.lds = {name: int((lds or {}).get(name, F)) for name in used}
    for name in used:
        if p.lds[name] < F:
            raise ValueError("%s: the row stride %d of %s is below F = %d" % (what, p.lds[name], name, F))
    known = {n: int(a) for n, a in (addresses or {}).items() if n in used and a is not None}
    if M > 0:
        span = lambda n: (known[n], ((M - 1) * p.lds[n] + F) * itemsize)
        for out in outputs:
            for name in used:
                if name in outputs or out not in known or name not in known:
                    continue
                (a, na), (b, nb) = span(out), span(name)
                if a < b + nb and b < a + na:
                    raise ValueError("%s: the output %s overlaps the input %s" % (what, out, name))
        if "dgate" in known and "dup" in known and not outputs_apart(known["dgate"], known["dup"], p.lds["dgate"],
                                                                    p.lds["dup"], M, F, itemsize):
            raise ValueError("%s: dgate and dup share elements (disjoint ranges, or equal row strides ld with "
                             "F <= (dup - dgate) mod ld <= ld - F)" % what)
    p.wide = wide_access(F, itemsize, p.lds.values(), known.values())
    p.chunks = F // (VEC // itemsize) if p.wide else F
    p.items = M * p.chunks
    p.grid = p.blocks or choose_blocks(p.items)
    ok = bool(native) and bool(float_ok)
    if route is not None and route not in ROUTES:
        raise ValueError("route must be one of %s or None, got %r" % (ROUTES, route))
    if route == "native" and not ok:
        raise ValueError("the native gated activation route needs libtnn_hip.so and float32 / float64 operands")
    if route == "composed" or not ok:
        if act == "gelu":
            raise ValueError("the exact (erf) GELU gate needs the native route of libtnn_hip.so; only act=\"silu\" and "
                             "act=\"gelu_tanh\" have a composed form")
        p.route = "composed"
    else:
        p.route = "native"
    return p


# ---------------------------------------------------------------------- the expressions in numpy (what the composed route computes)
def act_host(g, act):
    """(a, act') in g's dtype, one rounding per arithmetic operation.  "gelu" (erf) has no composed form."""
    g = np.asarray(g)
    one = g.dtype.type(1)
    if act == "silu":
        sig = one / (one + np.exp(-g))
        return g * sig, sig * (one + g * (one - sig))
    if act == "gelu_tanh":
        c, a = g.dtype.type(_GELU_C), g.dtype.type(_GELU_A)
        half = g.dtype.type(0.5)
        t = np.tanh((g + (g * g * g) * a) * c)
        return (g * half) * (t + one), (t + one) * half + (g * half) * (one - t * t) * ((g * g) * (3 * a) + one) * c
    raise ValueError("act_host: %r has no composed form" % (act,))


def gated_host(gate, up=None, act="silu"):
    a, _ = act_host(gate, act)
    return a if up is None else a * np.asarray(up)


def gated_bwd_host(gate, up, dy, act="silu"):
    """(dgate, dup); dup is None without up."""
    a, slope = act_host(gate, act)
    dy = np.asarray(dy)
    if up is None:
        return dy * slope, None
    return (dy * np.asarray(up)) * slope, dy * a
