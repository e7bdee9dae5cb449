"""The key normaliser of advanced indexing (tinynn-autograd_amd/indexing.py) against numpy itself, with no device and no
library: a pure-numpy evaluation of each descriptor must reproduce `a[key]`, and the kernel's duplicate rule (last advanced
position in C order wins) must reproduce `a[key] = v`."""

import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT

_spec = importlib.util.spec_from_file_location("tnn_indexing", os.path.join(ROOT, "tinynn-autograd_amd", "indexing.py"))
ix = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ix)


def rand_key(rs, shape):
    """ints (negative too), slices (negative steps, empty), None, Ellipsis, integer arrays / lists of 0-2 dims with
    duplicates, boolean masks over 1..k axes, boolean scalars."""
    nd = len(shape)
    items, dim, used_ell = [], 0, False
    while dim < nd and rs.rand() < 0.85:
        r, n = rs.rand(), shape[dim]
        if r < 0.12:
            items.append(None)
            continue
        if r < 0.19 and not used_ell:
            items.append(Ellipsis)
            used_ell = True
            dim = nd - rs.randint(0, nd - dim + 1)
            continue
        if r < 0.21:
            items.append(bool(rs.rand() < 0.5))
            continue
        if r < 0.38:
            a, b = rs.randint(-n - 1, n + 2, 2)
            items.append(slice(int(a), int(b), int(rs.choice([1, 1, 2, -1, -2, 3]))))
            dim += 1
        elif r < 0.48:
            items.append(int(rs.randint(-n, n)))
            dim += 1
        elif r < 0.8:
            sh = tuple(rs.randint(1, 4, rs.randint(0, 3))) if rs.rand() < 0.6 else (rs.randint(0, 7),)
            a = rs.randint(-n, n, sh)
            items.append(a.tolist() if rs.rand() < 0.2 and a.ndim else a)
            dim += 1
        else:
            k = rs.randint(1, nd - dim + 1)
            items.append(rs.rand(*shape[dim:dim + k]) < 0.5)
            dim += k
    return tuple(items) if (len(items) != 1 or rs.rand() < 0.5) else items[0]


def check(a, key):
    ref = a[key]
    plan = ix.normalize(a.shape, key)
    got = ix.evaluate(a.ravel(), plan)
    assert got.shape == ref.shape, (a.shape, key)
    np.testing.assert_array_equal(got, ref, err_msg=str((a.shape, key)))
    v = np.random.RandomState(len(ref.shape)).randn(*ref.shape)
    expect = a.copy()
    expect[key] = v
    flat = a.copy().ravel()
    ix.scatter(flat, plan, v)
    np.testing.assert_array_equal(flat.reshape(a.shape), expect, err_msg=str((a.shape, key)))
    return plan


def test_fuzz_against_numpy():
    rs = np.random.RandomState(2024)
    checked = errors = 0
    for _ in range(1500):
        shape = tuple(rs.randint(1, 6, rs.randint(1, 5)))
        a = rs.randn(*shape)
        key = rand_key(rs, shape)
        try:
            a[key]
        except IndexError:
            with pytest.raises(IndexError):
                ix.normalize(shape, key)
            errors += 1
            continue
        if a[key].ndim > ix.MAX_NDIM:
            with pytest.raises(TypeError, match="up to 6"):
                ix.normalize(shape, key)
            continue
        check(a, key)
        checked += 1
    assert checked >= 500 and errors > 0


@pytest.mark.parametrize("shape,key,out", [
    ((2, 3, 4, 5), (slice(None), [0, 1], slice(None), [1, 2]), (2, 2, 4)),      # separated: broadcast dims first
    ((2, 3, 4, 5), (slice(None), [0, 1], [1, 2]), (2, 2, 5)),                     # adjacent: in place
    ((3, 4, 5), (1, slice(None), [0, 1]), (2, 4)),                                # an int joins the advanced group
    ((3, 4), ([0], Ellipsis, [0]), (1,)),                                         # an empty Ellipsis separates nothing
    ((3, 4, 5), ([0], Ellipsis, [0]), (1, 4)),
    ((3, 4, 5), ([0], None, [0]), (1, 1, 5)),
    ((3, 4), (True,), (1, 3, 4)),
    ((3, 4), (False,), (0, 3, 4)),
    ((10, 4), np.arange(12).reshape(3, 4) % 10, (3, 4, 4)),
])
def test_numpy_placement_rules(shape, key, out):
    a = np.arange(np.prod(shape), dtype=np.float64).reshape(shape)
    assert check(a, key).out_shape == out


def test_duplicates_last_wins_and_uniqueness():
    a = np.zeros((4, 4))
    key = (np.array([0, 0, 1, 0]), np.array([2, 2, 3, 2]))
    plan = check(a, key)
    assert not plan.unique
    assert ix.normalize((5, 3), np.array([3, 0, 1])).unique
    assert ix.normalize((5, 3), np.array([3, 0, -2])).unique is False          # -2 wraps onto 3
    assert ix.normalize((4, 5), np.ones((4, 5), bool)).unique                   # a mask alone
    r = np.zeros(3)
    flat = r.copy()
    ix.scatter(flat, ix.normalize((3,), [0, 0, 1]), np.array([1.0, 2.0, 3.0]))
    assert flat.tolist() == [2.0, 3.0, 0.0]                                   # assignment, not np.add.at


@pytest.mark.parametrize("shape,key,exc", [
    ((4, 3), ([4],), IndexError),                                             # out of range
    ((4, 3), (slice(None), [-4]), IndexError),
    ((4, 3), (7,), IndexError),
    ((4, 3), (np.ones(3, bool),), IndexError),                                # boolean shape mismatch
    ((4, 3), (slice(None), np.ones((3, 1), bool)), IndexError),
    ((4, 3), (0, 0, 0), IndexError),                                          # too many indices
    ((4, 3), (Ellipsis, Ellipsis), IndexError),
    ((4, 3), (np.array([0.0, 1.0]),), IndexError),                            # float index array
    ((4, 3), ([0, 1], [0, 1, 2]), IndexError),                                # arrays that do not broadcast
])
def test_errors_match_numpy(shape, key, exc):
    a = np.zeros(shape)
    with pytest.raises(exc):
        a[key]
    with pytest.raises(exc):
        ix.normalize(shape, key)


def test_device_limits_raise_type_error():
    with pytest.raises(TypeError, match="6 output dimensions"):
        ix.normalize((2,) * 7, (np.array([0]),))
    with pytest.raises(TypeError, match="6 index arrays"):
        ix.normalize((2,) * 7, tuple(np.array([[0, 1]]) for _ in range(7)))


def test_descriptor_fields():
    """x[1::2, [[0, 4]], 3] on a (6, 5, 4) source: the slice's dim, then the adjacent group's broadcast dims (1, 2); the
    scalar of the group folds into the base offset."""
    plan = ix.normalize((6, 5, 4), (slice(1, None, 2), np.array([[0, 4]]), 3))
    assert plan.out_shape == (3, 1, 2)
    assert plan.base == 1 * 20 + 3 and plan.strides == (40, 0, 0) and plan.adv == (1, 2)
    (idx, ist, astride, alen), = plan.arrays
    assert idx.tolist() == [[0, 4]] and ist == (0, 0, 1) and astride == 4 and alen == 5
