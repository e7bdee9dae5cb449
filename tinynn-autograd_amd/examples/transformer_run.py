"""A tiny transformer through the ordinary `Model`: one pre-norm TransformerBlock (LayerNorm -> multi-head attention -> residual,
LayerNorm -> Dense -> GELU -> Dense -> residual) and a Dense head over the flattened sequence, Adam, softmax loss.  The data
are synthetic: a sequence of T noise vectors of width E in which ONE position, drawn at random, carries one of `classes`
fixed patterns; the label is the pattern.

    python tinynn-autograd_amd/examples/transformer_run.py [--num_ep 3] [--batch_size 64] [--n_train 2048] [--lr 3e-3] [--seed 0]
"""

import argparse
import os
import sys
import time

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(_HERE)))

import tinynn_autograd_amd as tn                                             # noqa: E402
from tinynn_autograd_amd.core.layers import Dense, Flatten, TransformerBlock  # noqa: E402
from tinynn_autograd_amd.core.losses import SoftmaxCrossEntropyLoss         # noqa: E402
from tinynn_autograd_amd.core.model import Model                             # noqa: E402
from tinynn_autograd_amd.core.nn import Net                                  # noqa: E402
from tinynn_autograd_amd.core.optimizer import Adam                          # noqa: E402
from tinynn_autograd_amd.core.tensor import Tensor                           # noqa: E402


def make_data(rs, count, seq, width, patterns):
    """([count, seq, width] float32, [count] labels): noise, with pattern `label` added at one random position."""
    x = (0.5 * rs.standard_normal((count, seq, width))).astype(np.float32)
    labels = rs.randint(0, len(patterns), count)
    x[np.arange(count), rs.randint(0, seq, count)] += patterns[labels]
    return x, labels


def main(args):
    if args.seed >= 0:
        np.random.seed(args.seed)
    rs = np.random.RandomState(max(args.seed, 0))
    patterns = rs.standard_normal((args.classes, args.width)).astype(np.float32)
    train_x, train_y = make_data(rs, args.n_train, args.seq, args.width, patterns)
    test_x, test_y = make_data(rs, args.n_test, args.seq, args.width, patterns)
    one_hot = np.eye(args.classes, dtype=np.float32)[train_y]
    net = Net([TransformerBlock(args.heads, num_in=args.width, fused=not args.composed), Flatten(), Dense(args.classes)])
    loss_layer = SoftmaxCrossEntropyLoss()
    model = Model(net=net, loss=loss_layer, optimizer=Adam(lr=args.lr))
    print("data: synthetic, %d sequences of %d x %d; backend %s" % (len(train_x), args.seq, args.width, tn.backend_name()))
    history = []
    for epoch in range(args.num_ep):
        t0, losses = time.time(), []
        for start in range(0, len(train_x) - args.batch_size + 1, args.batch_size):
            x = Tensor(train_x[start:start + args.batch_size])
            y = Tensor(one_hot[start:start + args.batch_size])
            model.zero_grad()
            loss = loss_layer.loss(model.forward(x), y)
            loss.backward()
            model.step()
            losses.append(loss)
        mean = float(np.mean([float(l.values) for l in losses]))
        model.set_phase("TEST")
        pred = np.argmax(np.asarray(model.forward(Tensor(test_x)).values), axis=1)
        model.set_phase("TRAIN")
        accuracy = float((pred == test_y).mean())
        history.append((mean, accuracy))
        print("epoch %d: mean loss %.4f, test accuracy %.4f, %.2f s" % (epoch, mean, accuracy, time.time() - t0))
    return history


def parse(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--num_ep", default=3, type=int)
    parser.add_argument("--lr", default=3e-3, type=float)
    parser.add_argument("--batch_size", default=64, type=int)
    parser.add_argument("--n_train", default=2048, type=int)
    parser.add_argument("--n_test", default=512, type=int)
    parser.add_argument("--seq", default=16, type=int)
    parser.add_argument("--width", default=32, type=int)
    parser.add_argument("--heads", default=4, type=int)
    parser.add_argument("--classes", default=8, type=int)
    parser.add_argument("--seed", default=0, type=int)
    parser.add_argument("--composed", action="store_true", help="fused=False: every part on its composed route")
    return parser.parse_args(argv)


if __name__ == "__main__":
    main(parse())
