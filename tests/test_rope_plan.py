"""The rotary planner (tinynn_autograd_amd/rope.py, numpy only): every refusal, the wide / element decision at the alignment
edges, the `blocks` rule, the Rotary object, and the accuracy of the host tables against the fixture's 50-digit spot values
(rope_oracle states the bound)."""

import numpy as np
import pytest

import rope_oracle as ro
import rope_support as rsup
from tinynn_autograd_amd import rope as rp


def plan(a=(2, 5, 4, 8), b=(2, 5, 2, 8), **kw):
    kw.setdefault("max_len", 64)
    return rp.plan_rope(a, b, **kw)


def test_geometry_strides_and_defaults():
    p = plan()
    assert p.geometry() == (2, 5, 4, 2, 8, 8, 64) and p.pairing_code() == 0 and p.route == "native" and not p.empty()
    assert p.strides() == (160, 32, 8) * 2 + (80, 16, 8) * 2
    p = plan((2, 4, 5, 8), (2, 2, 5, 8), layout="bhtd", pairing="interleaved", rotary_dim=4, offset=59, inverse=True)
    assert p.geometry() == (2, 5, 4, 2, 8, 4, 64) and p.pairing_code() == 1 and p.inverse and p.offset == 59
    assert p.strides() == (160, 8, 40) * 2 + (80, 8, 40) * 2
    assert plan((1, 1, 1, 7), None).R == 6 and plan((1, 1, 1, 7), None).Hb == 0
    assert plan((0, 5, 4, 8), (0, 5, 2, 8)).empty() and plan((2, 0, 4, 8), (2, 0, 2, 8)).empty()
    assert plan(native=False).route == "composed" and plan(float_ok=False).route == "composed"
    assert plan(route="composed").route == "composed"


@pytest.mark.parametrize("kw,match", [
    (dict(rotary_dim=3), "rotary width must be even"),
    (dict(rotary_dim=0), "rotary width must be even"),
    (dict(rotary_dim=10), "rotary width must be even"),
    (dict(b=(2, 5, 2, 6)), "agree in B, T and D"),
    (dict(b=(2, 4, 2, 8)), "agree in B, T and D"),
    (dict(b=(3, 5, 2, 8)), "agree in B, T and D"),
    (dict(a=(2, 5, 8)), "operands are"),
    (dict(offset=-1), "lie outside the table"),
    (dict(offset=60), "lie outside the table"),
    (dict(max_len=4), "lie outside the table"),
    (dict(max_len=None), "max_len must be >= 1"),
    (dict(positions_shape=(2,)), "device positions need T == 1"),
    (dict(a=(2, 1, 4, 8), b=None, positions_shape=(2,), offset=1), "device positions need T == 1 and offset == 0"),
    (dict(a=(2, 1, 4, 8), b=None, positions_shape=(3,)), "one position per sequence"),
    (dict(pairing="pairs"), "pairing must be one of"),
    (dict(layout="tbhd"), "layout must be one of"),
    (dict(blocks=-1), "blocks must be 0"),
    (dict(blocks=rp.MAX_BLOCKS + 1), "blocks must be 0"),
    (dict(route="fast"), "route must be one of"),
    (dict(route="native", native=False), "needs libtnn_hip.so"),
])
def test_refusals(kw, match):
    kw = dict(kw)
    a, b = kw.pop("a", (2, 5, 4, 8)), kw.pop("b", (2, 5, 2, 8))
    with pytest.raises(ValueError, match=match):
        plan(a, b, **kw)


def test_overlap():
    na, nb = 2 * 5 * 4 * 8 * 4, 2 * 5 * 2 * 8 * 4
    base = 1 << 20
    free = (base, None, base + na, None, None, None)
    assert plan(addresses=free).in_place == (False, False)
    assert plan(addresses=(base, base, base + na, base + na, None, None)).in_place == (True, True)
    assert plan(addresses=(base, base, base + na, None, None, None)).in_place == (True, False)
    for bad, match in (((base, base + 16, base + 4 * na, None, None, None), "overlaps its input"),
                       ((base, None, base + na, base + na + nb - 4, None, None), "overlaps its input"),
                       ((base, base + na, base + na, None, None, None), "two tensors overlap"),
                       ((base, base + 4 * na, base + na, base + 4 * na + 4, None, None), "two tensors overlap"),
                       ((base, None, base + na, base + 4, None, None), "two tensors overlap"),
                       ((base, base + 4 * na, base + na, None, base + 5 * na - 4, None), "overlaps the tables"),
                       ((base, None, base + na, base + 4 * na, None, base + 4 * na + nb - 4), "overlaps the tables")):
        with pytest.raises(ValueError, match=match):
            plan(addresses=bad)
    # touching is not overlapping
    plan(addresses=(base, base + na, base + 2 * na, base + 2 * na + nb, base + 4 * na, base + 8 * na))


def test_wide_or_element_at_the_alignment_edges():
    al = (4096, 8192, 12288, 16384, 20480, 24576)
    # R / 2 against the V = 4 (float32) and V = 2 (float64) elements of one access
    for R, wide32, wide64 in ((8, True, True), (12, False, True), (4, False, True), (2, False, False), (16, True, True)):
        assert plan((1, 3, 2, 16), (1, 3, 1, 16), rotary_dim=R, addresses=al, itemsize=4).wide is wide32, R
        assert plan((1, 3, 2, 16), (1, 3, 1, 16), rotary_dim=R, addresses=al, itemsize=8).wide is wide64, R
    # interleaved: the condition is on R
    for R, wide32, wide64 in ((4, True, True), (6, False, True), (2, False, True), (8, True, True)):
        assert plan((1, 3, 2, 16), None, rotary_dim=R, pairing="interleaved", addresses=al, itemsize=4).wide is wide32, R
        assert plan((1, 3, 2, 16), None, rotary_dim=R, pairing="interleaved", addresses=al, itemsize=8).wide is wide64, R
    # strides: D = 130 is a multiple of 2 but not of 4; D = 9 of neither
    assert plan((1, 2, 1, 130), (1, 2, 1, 130), rotary_dim=128, addresses=al, itemsize=8).wide
    assert not plan((1, 2, 1, 130), (1, 2, 1, 130), rotary_dim=128, addresses=al, itemsize=4).wide
    assert not plan((1, 2, 3, 9), None, rotary_dim=8, addresses=al, itemsize=8).wide
    # every base address counts, and only those that exist; without addresses the operands count as aligned
    for at in range(6):
        moved = tuple(a + (4 if i == at else 0) for i, a in enumerate(al))
        assert not plan(addresses=moved).wide, at
    assert plan().wide and plan(addresses=(4096, None, 8192, None, None, None)).wide
    assert plan((2, 5, 4, 8), None, addresses=(4096, None, 4100, 4100, None, None)).wide        # no second tensor: not looked at
    assert rp.wide_access("half", 8, 4, (32, 8), (4096,)) and not rp.wide_access("half", 8, 4, (32, 6), (4096,))


def test_items_and_blocks():
    p = plan((8, 1024, 16, 128), (8, 1024, 4, 128), max_len=4096)
    assert p.wide and p.items == 8 * 1024 * 20 * 16 and p.grid == rp.MAX_BLOCKS and p.blocks == 0
    p = plan((1, 5, 2, 8), (1, 5, 2, 8), itemsize=4)                  # one wide unit per row
    assert p.items == 20 and p.grid == 1
    p = plan((3, 1, 4, 16), (3, 1, 2, 16), rotary_dim=8, itemsize=4)      # a unit of rotation and two of tail per row
    assert p.items == 18 * 3
    al = (4096, 4096, 8192, 8192, None, None)
    assert plan((3, 1, 4, 16), (3, 1, 2, 16), rotary_dim=8, addresses=al).items == 18          # in place: the tail is skipped
    assert plan((3, 1, 4, 16), (3, 1, 2, 16), rotary_dim=8, addresses=al, positions_shape=(3,)).items == 18 * 3
    p = plan((2, 5, 3, 3), (2, 5, 1, 3), rotary_dim=2)                # element path: one pair and one tail element per row
    assert not p.wide and p.items == 40 * 2
    assert rp.choose_blocks(0) == 1 and rp.choose_blocks(256) == 1 and rp.choose_blocks(257) == 2
    assert rp.choose_blocks(rp.THREADS * rp.MAX_BLOCKS + 1) == rp.MAX_BLOCKS
    for forced in (1, 3, rp.MAX_BLOCKS):
        assert plan(blocks=forced).grid == forced


def test_rotary_object():
    rot = rp.Rotary(32)
    assert rot.width(8) == 8 and rot.width(7) == 6 and rot.pairing == "half" and rot.base == 10000.0
    with pytest.raises(ValueError, match="rotary width"):
        rot.width(1)
    assert rp.Rotary(32, 4).width(8) == 4
    with pytest.raises(ValueError, match="rotary width"):
        rp.Rotary(32, 10).width(8)
    for bad in (dict(max_len=0), dict(max_len=4, rotary_dim=3), dict(max_len=4, base=0.0), dict(max_len=4, pairing="x")):
        with pytest.raises(ValueError):
            rp.Rotary(**bad)
    cos_t, sin_t = rot.host_tables(8, np.float32)
    assert cos_t.shape == sin_t.shape == (32, 4) and cos_t.dtype == np.float32 and cos_t.flags.c_contiguous
    assert rot.host_tables(8, np.float32)[0] is cos_t                      # computed once
    assert (cos_t[0] == 1).all() and (sin_t[0] == 0).all()
    uploads = []
    first = rot.device_tables(8, np.float32, lambda host: uploads.append(host) or ("dev", len(uploads)))
    again = rot.device_tables(8, np.float32, lambda host: uploads.append(host))
    assert first is again and len(uploads) == 2                            # made once, never reallocated


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_tables_against_the_fifty_digit_spots(dtype):
    """|table - exact| <= u + 4 eps_longdouble p theta_i at every spot of the fixture (P = 4096, R = 128): the angle is formed
    in long double — a float64 angle misses the float64 bound by a factor of about forty at p = 4095."""
    g = rsup.load_golden()
    spots = [tuple(int(v) for v in row) for row in g["table.spots"]]
    assert spots == ro.TABLE_SPOTS
    assert {(0, 0), (ro.P - 1, 0), (0, ro.TABLE_R // 2 - 1), (ro.P - 1, ro.TABLE_R // 2 - 1)} <= set(spots)
    exact_c, exact_s = ro.dd_join(*g["table.cos"].T), ro.dd_join(*g["table.sin"].T)
    cos_t, sin_t = rp.tables(ro.P, ro.TABLE_R, ro.BASE, dtype)
    assert cos_t.dtype == np.dtype(dtype) and cos_t.shape == (ro.P, ro.TABLE_R // 2)
    for n, (p, i) in enumerate(spots):
        bound = ro.table_bound(p, i, ro.TABLE_R, dtype)
        for name, got, exact in (("cos", cos_t[p, i], exact_c[n]), ("sin", sin_t[p, i], exact_s[n])):
            err = float(abs(np.longdouble(got) - exact))
            print("%s[%d, %d] %s: error %.3e, bound %.3e" % (name, p, i, np.dtype(dtype).name, err, bound))
            assert err <= bound
    if np.dtype(dtype) == np.float64:                                     # the test can tell: a float64 angle does not pass
        i = np.arange(ro.TABLE_R // 2)
        angle = np.arange(ro.P, dtype=np.float64)[:, None] * (ro.BASE ** (-2.0 * i / ro.TABLE_R))[None, :]
        worst = max(float(abs(np.longdouble(np.cos(angle[p, i])) - exact_c[n])) / ro.table_bound(p, i, ro.TABLE_R, dtype)
                    for n, (p, i) in enumerate(spots))
        assert worst > 2.0
