"""TEST INFRASTRUCTURE — the float64 yardstick of convolution and max pooling (the reference has neither): numpy only,
`sliding_window_view` + `einsum` forward, the transposed forms for dx / dw / db, `argmax` over the flattened window for
pooling, the forward-error bounds of the tests, and a float64 replica of the LeNet training step (whole-batch softmax loss
of core/losses.py, Adam of oracle/closed_form.py).  tests/gen_conv_golden.py checks these functions against float64 torch."""

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

U32, U64 = 2.0 ** -24, 2.0 ** -53


def pair(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def out_extent(size, kernel, stride, padding):
    return (size + 2 * padding - kernel) // stride + 1


def windows(x, kh, kw, stride, padding, fill=0.0):
    """[N, C, OH, OW, KH, KW] view of the padded input."""
    (sh, sw), (ph, pw) = pair(stride), pair(padding)
    xp = np.pad(np.asarray(x, dtype=np.float64), ((0, 0), (0, 0), (ph, ph), (pw, pw)), constant_values=fill)
    return sliding_window_view(xp, (kh, kw), axis=(2, 3))[:, :, ::sh, ::sw]


def conv2d(x, w, b=None, stride=1, padding=0):
    w = np.asarray(w, dtype=np.float64)
    y = np.einsum("ncijkl,fckl->nfij", windows(x, w.shape[2], w.shape[3], stride, padding), w)
    return y if b is None else y + np.asarray(b, dtype=np.float64).reshape(1, -1, 1, 1)


def conv2d_dx(dy, w, x_shape, stride=1, padding=0):
    (sh, sw), (ph, pw) = pair(stride), pair(padding)
    dy, w = np.asarray(dy, dtype=np.float64), np.asarray(w, dtype=np.float64)
    n, c, h, wd = x_shape
    oh, ow = dy.shape[2:]
    dxp = np.zeros((n, c, h + 2 * ph, wd + 2 * pw))
    for kh in range(w.shape[2]):
        for kw in range(w.shape[3]):
            dxp[:, :, kh:kh + (oh - 1) * sh + 1:sh, kw:kw + (ow - 1) * sw + 1:sw] += np.einsum("nfij,fc->ncij", dy, w[:, :, kh, kw])
    return dxp[:, :, ph:ph + h, pw:pw + wd]


def conv2d_dw(x, dy, w_shape, stride=1, padding=0):
    dy = np.asarray(dy, dtype=np.float64)
    return np.einsum("ncijkl,nfij->fckl", windows(x, w_shape[2], w_shape[3], stride, padding), dy)


def conv2d_db(dy):
    return np.asarray(dy, dtype=np.float64).sum(axis=(0, 2, 3))


def max_pool2d(x, kernel, stride=None, padding=0):
    """(y, idx): idx = h * W + w of the first maximum of each window in row-major order (numpy's argmax)."""
    kh, kw = pair(kernel)
    sh, sw = (kh, kw) if stride is None else pair(stride)
    ph, pw = pair(padding)
    x = np.asarray(x, dtype=np.float64)
    win = windows(x, kh, kw, (sh, sw), (ph, pw), fill=-np.inf)
    flat = win.reshape(win.shape[:4] + (kh * kw,))
    arg = flat.argmax(axis=-1)
    y = np.take_along_axis(flat, arg[..., None], axis=-1)[..., 0]
    oh, ow = arg.shape[2:]
    h = (np.arange(oh) * sh - ph)[:, None] + arg // kw
    w = (np.arange(ow) * sw - pw)[None, :] + arg % kw
    return y, (h * x.shape[3] + w).astype(np.int64)


def max_pool2d_dx(dy, idx, x_shape):
    n, c, h, w = x_shape
    dx = np.zeros((n * c, h * w))
    dy = np.asarray(dy, dtype=np.float64).reshape(n * c, -1)
    np.add.at(dx, (np.arange(n * c)[:, None], np.asarray(idx).reshape(n * c, -1)), dy)
    return dx.reshape(x_shape)


# ---------------------------------------------------------------------- the derived bounds
def unit(dtype):
    return U32 if np.dtype(dtype) == np.float32 else 2.0 * U64


def fwd_bound(x, w, b, stride, padding, dtype):
    """(K + 2) u (|x| (*) |w| + |b|), K = C KH KW: a length-K dot product in any order plus one rounding for the bias."""
    k = w.shape[1] * w.shape[2] * w.shape[3]
    return (k + 2) * unit(dtype) * conv2d(np.abs(x), np.abs(w), None if b is None else np.abs(b), stride, padding)


def dx_bound(dy, w, x_shape, stride, padding, dtype):
    k = w.shape[0] * w.shape[2] * w.shape[3]
    return (k + 2) * unit(dtype) * conv2d_dx(np.abs(dy), np.abs(w), x_shape, stride, padding)


def dw_bound(x, dy, w_shape, stride, padding, dtype):
    k = dy.shape[0] * dy.shape[2] * dy.shape[3]
    return (k + 2) * unit(dtype) * conv2d_dw(np.abs(x), np.abs(dy), w_shape, stride, padding)


def db_bound(dy, dtype):
    k = dy.shape[0] * dy.shape[2] * dy.shape[3]
    return (k + 2) * unit(dtype) * conv2d_db(np.abs(dy))


def pool_dx_bound(dy, idx, x_shape, kernel, stride, dtype):
    """Overlapping windows add at most ceil(k / s) ** 2 terms per pixel; without overlap the result is exact (bound 0)."""
    kh, kw = pair(kernel)
    sh, sw = (kh, kw) if stride is None else pair(stride)
    terms = -(-kh // sh) * -(-kw // sw)
    if terms <= 1:
        return np.zeros(x_shape)
    return (terms + 2) * unit(dtype) * max_pool2d_dx(np.abs(dy), idx, x_shape)


def assert_within(got, want, bound, what):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, "%s: shape %s vs %s" % (what, got.shape, want.shape)
    err = np.abs(got - want)
    worst = float((err - bound).max()) if err.size else 0.0
    assert worst <= 0.0, "%s: error exceeds the derived bound by %.3e (max error %.3e, max bound %.3e)" % (
        what, worst, float(err.max()), float(bound.max()))


# ---------------------------------------------------------------------- float64 LeNet replica
class LeNet64(object):
    """Conv 5x5x1x6 pad 2 -> ReLU -> MaxPool 2 -> Conv 5x5x6x16 -> ReLU -> MaxPool 2 -> Flatten -> Dense 120 -> ReLU -> Dense 84
    -> ReLU -> Dense 10, whole-batch softmax loss, Adam.  Parameters in the package's flatten order (layer by layer, w then b)."""

    def __init__(self, params, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8):
        self.p = [np.array(a, dtype=np.float64) for a in params]        # cw1 cb1 cw2 cb2 w3 b3 w4 b4 w5 b5
        n = sum(a.size for a in self.p)
        self.m, self.v, self.t = np.zeros(n), np.zeros(n), 0
        self.lr, self.b1, self.b2, self.eps = lr, beta1, beta2, eps

    def loss_and_grads(self, x, y):
        cw1, cb1, cw2, cb2, w3, b3, w4, b4, w5, b5 = self.p
        x = np.asarray(x, dtype=np.float64)
        z1 = conv2d(x, cw1, cb1, 1, 2); a1 = np.maximum(z1, 0.0)
        p1, i1 = max_pool2d(a1, 2)
        z2 = conv2d(p1, cw2, cb2, 1, 0); a2 = np.maximum(z2, 0.0)
        p2, i2 = max_pool2d(a2, 2)
        f = p2.reshape(p2.shape[0], -1)
        z3 = f @ w3 + b3; a3 = np.maximum(z3, 0.0)
        z4 = a3 @ w4 + b4; a4 = np.maximum(z4, 0.0)
        z5 = a4 @ w5 + b5
        m = x.shape[0]
        e = np.exp(z5 - z5.max())
        prob = e / e.sum()
        loss = (-np.log((prob * y).sum(1))).sum() / m
        dz5 = prob - y / m
        g = [None] * 10
        g[8], g[9] = a4.T @ dz5, dz5.sum(0, keepdims=True)
        dz4 = (dz5 @ w5.T) * (z4 >= 0)
        g[6], g[7] = a3.T @ dz4, dz4.sum(0, keepdims=True)
        dz3 = (dz4 @ w4.T) * (z3 >= 0)
        g[4], g[5] = f.T @ dz3, dz3.sum(0, keepdims=True)
        dp2 = (dz3 @ w3.T).reshape(p2.shape)
        dz2 = max_pool2d_dx(dp2, i2, a2.shape) * (z2 >= 0)
        g[2], g[3] = conv2d_dw(p1, dz2, cw2.shape, 1, 0), conv2d_db(dz2)
        dp1 = conv2d_dx(dz2, cw2, p1.shape, 1, 0)
        dz1 = max_pool2d_dx(dp1, i1, a1.shape) * (z1 >= 0)
        g[0], g[1] = conv2d_dw(x, dz1, cw1.shape, 1, 2), conv2d_db(dz1)
        return loss, z5, [gi.reshape(pi.shape) for gi, pi in zip(g, self.p)]

    def step(self, x, y):
        loss, logits, grads = self.loss_and_grads(x, y)
        flat = np.concatenate([np.ravel(g) for g in grads])
        self.t += 1
        self.m = self.m + (1.0 - self.b1) * (flat - self.m)
        self.v = self.v + (1.0 - self.b2) * (flat ** 2 - self.v)
        upd = -self.lr * (self.m / (1 - self.b1 ** self.t)) / ((self.v / (1 - self.b2 ** self.t)) ** 0.5 + self.eps)
        off = 0
        for a in self.p:
            a += upd[off:off + a.size].reshape(a.shape)
            off += a.size
        return loss, grads


# ---------------------------------------------------------------------- the fixture's cases (tests/gen_conv_golden.py)
# name -> (x shape, w shape, stride, padding)
CONV_CASES = {
    "filter_1x1": ((2, 3, 5, 4), (4, 3, 1, 1), 1, 0),
    "filter_is_image": ((2, 2, 4, 3), (3, 2, 4, 3), 1, 0),
    "stride2_remainder_row": ((2, 3, 8, 7), (5, 3, 3, 3), 2, 0),
    "padding_larger_than_needed": ((1, 2, 5, 5), (3, 2, 3, 3), 1, 3),
    "one_input_channel": ((3, 1, 9, 9), (6, 1, 5, 5), 1, 2),
    "one_filter": ((2, 4, 6, 6), (1, 4, 3, 3), 1, 1),
    "non_square_everything": ((2, 3, 9, 6), (4, 3, 3, 2), (2, 1), (1, 0)),
    "batch_of_one": ((1, 5, 7, 7), (7, 5, 3, 3), 1, 1),
    "stride3_pad2": ((2, 2, 10, 11), (3, 2, 4, 2), (3, 2), (2, 1)),
    "channels_past_one_tile": ((1, 18, 4, 4), (35, 18, 2, 2), 1, 1),
    "lenet_conv1": ((1, 1, 28, 28), (6, 1, 5, 5), 1, 2),
    "lenet_conv2": ((1, 6, 14, 14), (16, 6, 5, 5), 1, 0),
}
# name -> (x shape, kernel, stride, padding)
POOL_CASES = {
    "pool_2x2": ((2, 3, 6, 6), 2, None, 0),
    "pool_overlap_3s2p1": ((2, 2, 7, 6), 3, 2, 1),
    "pool_overlap_3s1": ((1, 2, 5, 5), 3, 1, 0),
    "pool_non_square": ((2, 2, 9, 7), (3, 2), (2, 1), (1, 0)),
    "pool_remainder": ((1, 3, 7, 7), 2, None, 0),
    "pool_lenet": ((1, 2, 28, 28), 2, None, 0),
}


def case_seed(name):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % (2 ** 31)


def conv_case_input(name):
    """(x, w, b, dy) of a convolution case: float32 values of order 1 - 10, rebuilt from the case's seed."""
    xs, ws, stride, padding = CONV_CASES[name]
    rs = np.random.RandomState(case_seed(name))
    (sh, sw), (ph, pw) = pair(stride), pair(padding)
    oh, ow = out_extent(xs[2], ws[2], sh, ph), out_extent(xs[3], ws[3], sw, pw)
    x = (rs.randn(*xs) * 3).astype(np.float32)
    w = (rs.randn(*ws) * 2).astype(np.float32)
    b = (rs.randn(ws[0]) * 5).astype(np.float32)
    dy = (rs.randn(xs[0], ws[0], oh, ow) * 2).astype(np.float32)
    return x, w, b, dy


def pool_case_input(name):
    """(x, dy): small integers in float32, so windows tie often."""
    xs, kernel, stride, padding = POOL_CASES[name]
    rs = np.random.RandomState(case_seed(name))
    x = rs.randint(-3, 4, xs).astype(np.float32)
    _, idx = max_pool2d(x, kernel, stride, padding)
    dy = (rs.randn(*idx.shape) * 2).astype(np.float32)
    return x, dy


def lenet_batches(steps=5, rows=16, seed=7):
    """MNIST-shaped synthetic rows ([rows, 1, 28, 28], ~19 % of the pixels non-zero) and one-hot labels."""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(steps):
        x = (rs.rand(rows, 1, 28, 28) * (rs.rand(rows, 1, 28, 28) < 0.19)).astype(np.float32)
        y = np.eye(10)[rs.randint(0, 10, rows)]
        out.append((x, y))
    return out
