"""Advanced indexing on the MI355X (csrc/tnn_index.hip through indexing.py / device_array.py): index tuples, boolean
masks, N-d index arrays, nonzero, pad modes — forward and backward, against the reference's recorded results
(tests/golden/index_cases.npz) and numpy."""

import numpy as np
import pytest

import gen_index_golden as G

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64, np.int64, np.bool_]


def _tn():
    import tinynn_autograd_amd as tn
    return tn


def _host(rs, shape, dtype):
    if dtype == np.bool_:
        return np.asarray(rs.rand(*shape) < 0.5)
    if dtype == np.int64:
        return np.asarray(rs.randint(-1000, 1000, shape), dtype=np.int64)
    return np.asarray(rs.randn(*shape), dtype=dtype)


def _rand_key(rs, shape, device):
    """A numpy-valid key over `shape`: ints, slices, None, Ellipsis, index arrays of 1-2 dims, boolean masks."""
    tn = _tn()
    nd = len(shape)
    items, dim, used_ell = [], 0, False
    while dim < nd and rs.rand() < 0.85:
        r, n = rs.rand(), shape[dim]
        if r < 0.12:
            items.append(None)
            continue
        if r < 0.18 and not used_ell:
            items.append(Ellipsis)
            used_ell = True
            dim = nd - rs.randint(0, nd - dim + 1)
            continue
        if r < 0.38:
            a, b = rs.randint(-n - 1, n + 2, 2)
            items.append(slice(int(a), int(b), int(rs.choice([1, 1, 2, -1, -2]))))
            dim += 1
        elif r < 0.48:
            items.append(int(rs.randint(-n, n)))
            dim += 1
        elif r < 0.8:
            sh = tuple(rs.randint(1, 4, rs.randint(1, 3))) if rs.rand() < 0.5 else (rs.randint(0, 6),)
            a = rs.randint(-n, n, sh).astype(np.int64)
            items.append(tn.asarray(a) if device and rs.rand() < 0.6 else a)
            dim += 1
        else:
            k = rs.randint(1, nd - dim + 1)
            m = rs.rand(*shape[dim:dim + k]) < 0.5
            items.append(tn.asarray(m) if device and rs.rand() < 0.6 else m)
            dim += k
    return tuple(items) if (len(items) != 1 or rs.rand() < 0.5) else items[0]


def _np_key(key):
    if isinstance(key, tuple):
        return tuple(_np_key(k) for k in key)
    tn = _tn()
    return np.asarray(key) if isinstance(key, tn.DeviceArray) else key


@pytest.mark.parametrize("mode", [np.float32, np.float64])
def test_golden_cases_forward_and_backward(mode):
    tn = _tn()
    from tinynn_autograd_amd.core import ops
    from tinynn_autograd_amd.core.tensor import Tensor
    tn.set_default_float(mode)
    gold = G.load()
    for name in G.CASES:
        fwd, grad = G.run_case(name, Tensor, ops, to_values=np.asarray)
        np.testing.assert_array_equal(fwd, gold[name + "/fwd"], err_msg=name)
        np.testing.assert_array_equal(grad, gold[name + "/grad"], err_msg=name)
        assert fwd.shape == gold[name + "/fwd"].shape and grad.shape == gold[name + "/grad"].shape, name


def test_fuzz_get_and_set_against_numpy():
    tn = _tn()
    rs = np.random.RandomState(7)
    done = 0
    for t in range(400):
        dtype = DTYPES[t % 4]
        shape = tuple(rs.randint(1, 6, rs.randint(1, 5)))
        host = _host(rs, shape, dtype)
        dev = tn.asarray(host, dtype=dtype)
        key = _rand_key(rs, shape, device=t % 2 == 1)
        nkey = _np_key(key)
        try:
            ref = host[nkey]
        except IndexError:
            with pytest.raises(IndexError):
                dev[key]
            continue
        if ref.ndim > 6:
            continue
        got = np.asarray(dev[key])
        assert got.dtype == ref.dtype and got.shape == ref.shape, (shape, nkey)
        np.testing.assert_array_equal(got, ref, err_msg=str((shape, nkey)))
        val = _host(rs, ref.shape, dtype)
        expect = host.copy()
        expect[nkey] = val
        dev[key] = tn.asarray(val, dtype=dtype)
        np.testing.assert_array_equal(np.asarray(dev), expect, err_msg=str((shape, nkey)))
        done += 1
    assert done > 250


def test_nd_device_integer_key_gets_numpy_shape():
    tn = _tn()
    x = np.arange(40, dtype=np.float32).reshape(10, 4)
    idx = np.array([[0, 9, 3], [3, 1, 2]], dtype=np.int64)
    got = tn.asarray(x)[tn.asarray(idx)]
    assert got.shape == (2, 3, 4)
    np.testing.assert_array_equal(np.asarray(got), x[idx])


def test_duplicate_device_key_is_deterministic_last_wins():
    tn = _tn()
    rs = np.random.RandomState(3)
    idx = rs.randint(0, 50, 20000).astype(np.int64)
    val = rs.randn(20000, 33).astype(np.float32)
    expect = np.zeros((50, 33), np.float32)
    expect[idx] = val
    results = []
    for _ in range(3):
        d = tn.zeros((50, 33), np.float32)
        d[tn.asarray(idx)] = tn.asarray(val)
        results.append(np.asarray(d))
    for r in results:
        np.testing.assert_array_equal(r, expect)
    # element-granular duplicates through a 2-array device key
    rows, cols = rs.randint(0, 8, 5000), rs.randint(0, 9, 5000)
    v = rs.randn(5000).astype(np.float64)
    e = np.zeros((8, 9))
    e[rows, cols] = v
    for _ in range(3):
        d = tn.zeros((8, 9), np.float64)
        d[tn.asarray(rows), tn.asarray(cols)] = tn.asarray(v, dtype=np.float64)
        np.testing.assert_array_equal(np.asarray(d), e)


@pytest.mark.parametrize("shape,density", [((0,), 0.5), ((37,), 1.1), ((13, 17), 0.3), ((4, 5, 6), 0.4),
                                           ((5_000_000,), 0.19), ((1001,), 0.0)])
def test_nonzero_family(shape, density):
    tn = _tn()
    rs = np.random.RandomState(11)
    m = rs.rand(*shape) < density
    d = tn.asarray(m)
    for got, ref in zip(np.nonzero(d), np.nonzero(m)):
        assert got.dtype == np.int64
        np.testing.assert_array_equal(np.asarray(got), ref)
    assert len(d.nonzero()) == len(shape)
    for got, ref in zip(np.where(d), np.where(m)):
        np.testing.assert_array_equal(np.asarray(got), ref)
    np.testing.assert_array_equal(np.asarray(np.flatnonzero(d)), np.flatnonzero(m))
    assert np.count_nonzero(d) == np.count_nonzero(m)
    if len(shape) == 2:                                   # a float array: nonzero of x != 0
        x = np.where(m, rs.randn(*shape), 0.0).astype(np.float32)
        for got, ref in zip(np.nonzero(tn.asarray(x)), np.nonzero(x)):
            np.testing.assert_array_equal(np.asarray(got), ref)


def test_full_size_gathers_are_exact():
    tn = _tn()
    rs = np.random.RandomState(5)
    X = rs.randn(50_000, 784).astype(np.float32)
    dX = tn.asarray(X)
    rows = rs.randint(0, 50_000, 128)
    cols = rs.permutation(784)[:300]
    np.testing.assert_array_equal(np.asarray(dX[rows[:, None], cols]), X[rows[:, None], cols])
    row_mask = rs.rand(50_000) < 0.3
    np.testing.assert_array_equal(np.asarray(dX[row_mask]), X[row_mask])
    np.testing.assert_array_equal(np.asarray(dX[tn.asarray(row_mask)]), X[row_mask])
    np.testing.assert_array_equal(np.asarray(dX.take(cols, axis=1)), np.take(X, cols, axis=1))


@pytest.mark.parametrize("mode,kw", [("edge", {}), ("reflect", {}), ("symmetric", {}), ("wrap", {}),
                                     ("constant", {"constant_values": 2.5}), ("constant", {})])
def test_pad_modes_large(mode, kw):
    tn = _tn()
    rs = np.random.RandomState(2)
    x = rs.randn(512, 4096).astype(np.float32)
    pw = ((3, 700), (17, 4))                              # 700 > 512: reflect repeats
    got = np.pad(tn.asarray(x), pw, mode, **kw)
    np.testing.assert_array_equal(np.asarray(got), np.pad(x, pw, mode, **kw))


def test_device_mask_inside_capture_raises_and_leaves_no_state():
    tn = _tn()
    x = tn.asarray(np.arange(12, dtype=np.float32).reshape(3, 4))

    def masked():
        return x[x > 5.0]

    with pytest.raises(RuntimeError, match="depends on the data"):
        tn.capture(masked, warmup=0)
    y = tn.zeros((3, 4), np.float32)

    def plain():
        y[...] = x * 2.0
        return y

    f = tn.capture(plain, warmup=1)
    f()
    tn.synchronize()
    np.testing.assert_array_equal(np.asarray(y), np.arange(12, dtype=np.float32).reshape(3, 4) * 2)


def test_mask_and_nll_backward_on_mlp_logits():
    tn = _tn()
    from tinynn_autograd_amd.core.layers import Dense, ReLU
    from tinynn_autograd_amd.core.nn import Net
    from tinynn_autograd_amd.core.tensor import Tensor
    np.random.seed(0)
    rs = np.random.RandomState(4)
    m = 64
    net = Net([Dense(32, num_in=20), ReLU(), Dense(10, num_in=32)])
    x = rs.randn(m, 20).astype(np.float32)
    labels = rs.randint(0, 10, m)
    logits = net.forward(Tensor(x))
    L = np.asarray(logits.values).astype(np.float64)

    leaf = Tensor(logits.values, requires_grad=True)
    picked = leaf[np.arange(m), labels]                   # the NLL gather
    g = rs.randn(m)
    picked.backward(g)
    expect = np.zeros((m, 10))
    expect[np.arange(m), labels] = g
    np.testing.assert_array_equal(np.asarray(picked.values), L[np.arange(m), labels].astype(np.float32))
    np.testing.assert_allclose(np.asarray(leaf.grad), expect, rtol=0, atol=1e-6)

    leaf2 = Tensor(logits.values, requires_grad=True)
    pos = leaf2[leaf2 > 0]                                # a device mask from a comparison
    mask = L > 0
    np.testing.assert_array_equal(np.asarray(pos.values), L[mask].astype(np.float32))
    g2 = rs.randn(int(mask.sum()))
    pos.backward(g2)
    expect2 = np.zeros((m, 10))
    expect2[mask] = g2
    np.testing.assert_allclose(np.asarray(leaf2.grad), expect2, rtol=0, atol=1e-6)


def test_tensor_keys_inside_tuples():
    tn = _tn()
    from tinynn_autograd_amd.core.tensor import Tensor
    x = np.arange(30, dtype=np.float32).reshape(5, 6)
    t = Tensor(x, requires_grad=True)
    idx = Tensor(np.array([4, 0, 4]))
    out = t[idx, 1:3]
    np.testing.assert_array_equal(np.asarray(out.values), x[[4, 0, 4], 1:3])
    out.backward(np.ones((3, 2)))
    e = np.zeros((5, 6))
    e[[4, 0], 1:3] = 1.0
    np.testing.assert_array_equal(np.asarray(t.grad), e)
