"""The host planner of the gated activations (tinynn_autograd_amd/gated.py): route, access path, workgroup count, strides and
every refusal of include/tnn_gated.h with its message — numpy only, nothing is launched."""

import pytest

from tinynn_autograd_amd import gated as gt

A = 0x7F0000000000            # a 16-byte aligned address; the operands below sit 1 MiB apart
MB = 1 << 20


def addrs(*names, **moved):
    out = {n: A + i * MB for i, n in enumerate(names)}
    out.update(moved)
    return out


def test_constants_and_hidden_width():
    assert gt.ACTS == ("silu", "gelu_tanh", "gelu") and gt.ROUTES == ("native", "composed")
    assert (gt.VEC, gt.THREADS, gt.MAX_BLOCKS) == (16, 256, 2048)
    assert gt.FWD_OPERANDS == ("gate", "up", "y") and gt.BWD_OPERANDS == ("gate", "up", "dy", "dgate", "dup")
    # 8 E / 3 rounded up to a multiple of 8
    assert [gt.gated_hidden(e) for e in (3, 8, 16, 64, 768, 4096)] == [8, 24, 48, 176, 2048, 10928]


@pytest.mark.parametrize("itemsize,v", [(4, 4), (8, 2)])
def test_wide_path_needs_aligned_bases_strides_and_f(itemsize, v):
    plan = lambda F, lds=None, **moved: gt.plan_gated(5, F, lds=lds, addresses=addrs("gate", "up", "y", **moved), itemsize=itemsize)
    p = plan(4 * v)
    assert p.wide and p.chunks == 4 and p.items == 20 and p.route == "native"
    assert not plan(4 * v + 1).wide and plan(4 * v + 1).chunks == 4 * v + 1                       # F
    assert plan(4 * v, dict(gate=5 * v, up=5 * v, y=6 * v)).wide                                   # padded rows, still wide
    assert not plan(4 * v, dict(y=4 * v + 1)).wide                                                 # a stride
    for name in ("gate", "up", "y"):                                                               # a base off by one element
        assert not plan(4 * v, **{name: A + 7 * MB + itemsize}).wide
    # an operand without an address is a fresh array: aligned
    assert gt.plan_gated(5, 4 * v, addresses=dict(gate=A), itemsize=itemsize).wide
    # the packed projection: gate = z, up = z + F, ld = 2 F — wide iff F is a multiple of V
    packed = lambda F: gt.plan_gated(5, F, lds=dict(gate=2 * F, up=2 * F), addresses=dict(gate=A, up=A + F * itemsize),
                                     itemsize=itemsize)
    assert packed(2 * v).wide and packed(2 * v).strides() == (4 * v, 4 * v, 2 * v)
    assert not packed(2 * v + 1).wide and not packed(v + v // 2).wide
    # an unused operand's stride and address do not count
    p = gt.plan_gated(5, 4 * v, has_up=False, lds=dict(up=4 * v + 1), addresses=dict(up=A + 1), itemsize=itemsize)
    assert p.wide and p.operands == ("gate", "y") and p.strides() == (4 * v, 4 * v, 4 * v)


def test_backward_operands_and_strides():
    p = gt.plan_gated(3, 8, "gelu_tanh", backward=True, lds=dict(gate=16, up=16, dgate=16, dup=16),
                      addresses=dict(gate=A, up=A + 32, dy=A + MB, dgate=A + 2 * MB, dup=A + 2 * MB + 32))
    assert p.operands == gt.BWD_OPERANDS and p.strides() == (16, 16, 8, 16, 16) and p.wide and p.act_code() == 1
    p = gt.plan_gated(3, 8, backward=True, need_dup=False, lds=dict(dup=3), addresses=dict(dup=A + 1))
    assert p.operands == ("gate", "up", "dy", "dgate") and p.wide and p.strides()[4] == 8
    p = gt.plan_gated(3, 8, backward=True, has_up=False, need_dup=False)
    assert p.operands == ("gate", "dy", "dgate")
    with pytest.raises(ValueError, match="the plain activation \\(no up\\) has no dup"):
        gt.plan_gated(3, 8, backward=True, has_up=False)
    with pytest.raises(ValueError, match="neither dgate nor dup is asked for"):
        gt.plan_gated(3, 8, backward=True, need_dgate=False, need_dup=False)


def test_blocks():
    assert gt.plan_gated(1, 1).grid == 1
    assert gt.plan_gated(1, 256, itemsize=4).grid == 1 and gt.plan_gated(1, 257).grid == 2        # 64 wide items; 257 elements
    assert gt.plan_gated(257, 4).grid == 2 and gt.plan_gated(8192, 4096).grid == gt.MAX_BLOCKS
    assert gt.plan_gated(8192, 4096, blocks=3).grid == 3 and gt.plan_gated(8192, 4096, blocks=3).blocks == 3
    assert gt.choose_blocks(0) == 1 and gt.choose_blocks(256 * 2048 + 1) == 2048
    for bad in (-1, gt.MAX_BLOCKS + 1):
        with pytest.raises(ValueError, match="blocks must be 0 \\(the library's choice\\) or 1 .. 2048, got %d" % bad):
            gt.plan_gated(4, 4, blocks=bad)


def test_refusals():
    with pytest.raises(ValueError, match="act must be one of .*got 'relu'"):
        gt.plan_gated(4, 4, "relu")
    with pytest.raises(ValueError, match="F must be >= 1, got 0"):
        gt.plan_gated(4, 0)
    with pytest.raises(ValueError, match="M must be >= 0, got -1"):
        gt.plan_gated(-1, 4)
    with pytest.raises(ValueError, match="M 32768 x F 65536 is 2\\^31 elements or more"):
        gt.plan_gated(1 << 15, 1 << 16)
    assert gt.plan_gated((1 << 15) - 1, 1 << 16).items == ((1 << 15) - 1) << 14
    for name in ("gate", "up", "y"):
        with pytest.raises(ValueError, match="the row stride 7 of %s is below F = 8" % name):
            gt.plan_gated(4, 8, lds={name: 7})
    for name in ("dy", "dgate", "dup"):
        with pytest.raises(ValueError, match="gated_bwd: the row stride 7 of %s is below F = 8" % name):
            gt.plan_gated(4, 8, backward=True, lds={name: 7})
    with pytest.raises(ValueError, match="unknown operand 'dy'"):
        gt.plan_gated(4, 8, lds=dict(dy=8))
    # an output's address range may not touch an input's
    for name in ("gate", "up"):
        with pytest.raises(ValueError, match="the output y overlaps the input %s" % name):
            gt.plan_gated(4, 8, addresses={name: A, "y": A + 4 * 8 * 4 - 4})
        gt.plan_gated(4, 8, addresses={name: A, "y": A + 4 * 8 * 4})
    with pytest.raises(ValueError, match="the output y overlaps the input gate"):           # in place is refused too
        gt.plan_gated(4, 8, addresses=dict(gate=A, y=A))
    for out in ("dgate", "dup"):
        for name in ("gate", "up", "dy"):
            with pytest.raises(ValueError, match="gated_bwd: the output %s overlaps the input %s" % (out, name)):
                gt.plan_gated(4, 8, backward=True, addresses={name: A + 64, out: A})
    # the routes
    with pytest.raises(ValueError, match="route must be one of"):
        gt.plan_gated(4, 8, route="fast")
    for kw in (dict(native=False), dict(float_ok=False)):
        assert gt.plan_gated(4, 8, **kw).route == "composed"
        with pytest.raises(ValueError, match="native gated activation route needs libtnn_hip.so and float32 / float64"):
            gt.plan_gated(4, 8, route="native", **kw)
        with pytest.raises(ValueError, match="exact \\(erf\\) GELU gate needs the native route"):
            gt.plan_gated(4, 8, "gelu", **kw)
    assert gt.plan_gated(4, 8, "gelu").route == "native" and gt.plan_gated(4, 8, "gelu_tanh", route="composed").route == "composed"
    with pytest.raises(ValueError, match="exact \\(erf\\) GELU gate needs the native route"):
        gt.plan_gated(4, 8, "gelu", route="composed")


@pytest.mark.parametrize("itemsize", [4, 8])
def test_dgate_and_dup_share_no_element(itemsize):
    F, M = 6, 3
    plan = lambda dgate, dup, ld_g, ld_u: gt.plan_gated(M, F, backward=True, lds=dict(dgate=ld_g, dup=ld_u),
                                                        addresses=dict(dgate=dgate, dup=dup), itemsize=itemsize)
    el = itemsize
    # the halves of one dz [M, 2 F]: bases F apart are accepted, F - 1 apart share a column
    assert plan(A, A + F * el, 2 * F, 2 * F).strides()[3:] == (2 * F, 2 * F)
    plan(A + F * el, A, 2 * F, 2 * F)                                                    # either order
    with pytest.raises(ValueError, match="dgate and dup share elements"):
        plan(A, A + (F - 1) * el, 2 * F, 2 * F)
    with pytest.raises(ValueError, match="dgate and dup share elements"):
        plan(A, A + (F + 1) * el, 2 * F, 2 * F)                                          # ld - F < 7: dup runs into the next row's dgate
    plan(A, A + (F + 1) * el, 2 * F + 1, 2 * F + 1)                                      # ... a padded row has the room
    with pytest.raises(ValueError, match="dgate and dup share elements"):
        plan(A, A, F, F)
    with pytest.raises(ValueError, match="dgate and dup share elements"):
        plan(A, A + F * el + 1, 2 * F, 2 * F)                                            # not a whole number of elements apart
    # unequal row strides: only disjoint address ranges
    with pytest.raises(ValueError, match="dgate and dup share elements"):
        plan(A, A + F * el, 2 * F, 2 * F + 1)
    span = ((M - 1) * 2 * F + F) * el
    plan(A, A + span, 2 * F, 2 * F + 1)
    plan(A, A + span, F, F)                                                              # two dense arrays, back to back
    # the rule itself, for a distance of whole rows plus a column offset
    assert gt.outputs_apart(A, A + (2 * F + F) * el, 2 * F, 2 * F, M, F, el)
    assert not gt.outputs_apart(A, A + (2 * F) * el, 2 * F, 2 * F, M, F, el)


def test_empty():
    p = gt.plan_gated(0, 8, addresses=dict(gate=A, y=A))                 # nothing is read or written: no overlap to refuse
    assert p.empty() and p.items == 0 and p.grid == 1
    assert gt.plan_gated(0, 8, backward=True, addresses=dict(dgate=A, dup=A)).empty()
    assert not gt.plan_gated(1, 8).empty()
    with pytest.raises(ValueError, match="F must be >= 1"):
        gt.plan_gated(0, 0)
