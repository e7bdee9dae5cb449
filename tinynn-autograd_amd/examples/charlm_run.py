"""A tiny causal language model through the ordinary `Model`: Embedding (tokens + learned positions) -> two pre-norm causal
TransformerBlocks -> LayerNorm -> Dense head over every position -> per-row CrossEntropyLoss, Adam.  The data are synthetic
and generated here: each sequence repeats a random motif of `period` tokens drawn from `vocab`, and the target is the next
token — so every position >= period can be predicted by attending one period back, and the first `period` cannot.

    python tinynn-autograd_amd/examples/charlm_run.py [--num_ep 4] [--batch_size 64] [--n_train 2048] [--lr 3e-3] [--seed 0]

--generate N: after training, the first test sequences are continued greedily by N tokens from a prompt of 2 * period tokens
(generation.generate: a key / value cache, every token chosen on the device), and the share of generated tokens that continue
the motif is printed.  --ragged cuts the prompts to differing lengths between `period` and 2 * period tokens (the ragged path
of generation.generate: the sequences' lengths live on the device), --eos ID ends a sequence at token ID (the pad token 0 is
emitted after it) and --capture records the token step into a graph once and replays it.

--prefill-chunk C runs the prompt through the net in pieces of C tokens (generation.generate(prefill_chunk=): the first piece is
the ordinary prefill, the others extend the cache through ops.attention_extend_, csrc/tnn_extend.hip); --second-turn M keeps the
first turn's cache (a KVCache(extend=True)) and continues it in a second generate call: its prompt is the one token the cache
does not hold yet plus the next `period` tokens of the motif (the "user's turn": several new rows, which extend the cache in
one launch per block), followed by M new tokens — the tokens of one call on the concatenated prompt.  Both belong to the uniform
path (no --ragged, --eos, --capture).

--dropout P: dropout with rate P on the embedding's output and on both residual branches of every block (the fused residual
form of ops.dropout_), drawn from the device generator of rng.py, which --seed seeds; 0, the default, adds no launch.

--rope: rotary position embeddings instead of learned positions — the blocks share ONE rope.Rotary(max_len=--seq), which
rotates q and k of every attention layer (one launch forward, two backward, one per decoding step and block), and the
Embedding is built without max_len, so there is no "pos" table.  It composes with --kv-heads, --generate, --ragged and
--capture.  Default off: the run is what it was.

--mlp {gelu,swiglu,geglu}: the feed-forward of the blocks.  gelu (the default) is GELU(x W1 + b1) W2 + b2 as before; swiglu and
geglu are the gated forms act(x Wg) * (x Wu) projected by W2, with Wg and Wu held as one fc1 [E, 2 hidden] and the product done
by ONE ops.gated_ launch (csrc/tnn_gated.hip); hidden is then 8 E / 3 rounded up to a multiple of 8.

--ragged-train: right-padded batches, the way real text arrives — every sequence of a batch is cut to a random length in
[seq / 4, seq], the targets at and beyond it are set to the loss's ignore_index, and the lengths are uploaded once per batch
and handed to the model (model.forward(x, lens=)): every attention launch reads them on the device (include/tnn_varlen.h),
skips whole 64-row blocks of padding and never reads a padded row.  --no-lens keeps the lengths from the model: the padded
baseline, right for this causal model and wasteful.  The live tokens per second of every epoch are printed.  Default off.

--adamw: core/optimizer.AdamW instead of Adam — decoupled weight decay (--weight_decay, biases and norm parameters exempt),
clipping by the global gradient norm (--clip MAX_NORM, 0 = none) and a linear warm-up over --warmup steps followed by a cosine
decay to zero at the last step, all resident on the device (include/tnn_ostep.h).  Without --adamw the run and its launch
sequence are what they were.
"""

import argparse
import os
import sys
import time

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(_HERE)))

import tinynn_autograd_amd as tn                                                            # noqa: E402
from tinynn_autograd_amd import device_array as da, ostep, rng                              # noqa: E402
from tinynn_autograd_amd.rope import Rotary                                                 # noqa: E402
from tinynn_autograd_amd.core import ops                                                    # noqa: E402
from tinynn_autograd_amd.generation import KVCache, generate                                # noqa: E402
from tinynn_autograd_amd.core.layers import Dense, Embedding, Layer, LayerNorm, TransformerBlock  # noqa: E402
from tinynn_autograd_amd.core.losses import CrossEntropyLoss                                # noqa: E402
from tinynn_autograd_amd.core.model import Model                                            # noqa: E402
from tinynn_autograd_amd.core.nn import Net                                                 # noqa: E402
from tinynn_autograd_amd.core.optimizer import Adam, AdamW                                  # noqa: E402
from tinynn_autograd_amd.core.tensor import Tensor                                          # noqa: E402


class Rows(Layer):
    """[B, T, E] -> [B T, E]: Dense stays 2-D."""

    def __init__(self):
        super().__init__("Rows")

    def forward(self, inputs):
        return ops.reshape(inputs, (-1, int(inputs.shape[-1])))


def make_data(rs, count, seq, vocab, period):
    """(ids [count, seq], targets [count, seq]) int64: a motif of `period` random tokens repeated; the target is the next token."""
    motif = rs.randint(0, vocab, (count, period))
    stream = motif[:, np.arange(seq + 1) % period]
    return np.ascontiguousarray(stream[:, :-1]), np.ascontiguousarray(stream[:, 1:])


IGNORE = -1           # --ragged-train: the target of a position at or beyond its sequence's length


def ragged_batch(rs, x, y, seq):
    """--ragged-train: every sequence of the batch cut to a random length in [seq / 4, seq] — the ids stay (right padding: what
    sits there is never read by the attention), the targets at dead positions become IGNORE.  -> (lens, targets)."""
    lens = rs.randint(max(seq // 4, 1), seq + 1, len(x))
    y = np.where(np.arange(seq)[None, :] < lens[:, None], y, IGNORE)
    return lens, y


def build(args):
    fused = not args.composed
    drop = args.dropout
    rotary = Rotary(args.seq) if getattr(args, "rope", False) else None      # shared by the blocks; then no "pos" table
    mlp = getattr(args, "mlp", "gelu")
    net = Net([Embedding(args.vocab, args.width, max_len=None if rotary else args.seq, fused=fused, dropout=drop),
               TransformerBlock(args.heads, num_in=args.width, causal=True, fused=fused, dropout=drop, kv_heads=args.kv_heads,
                                rope=rotary, mlp=mlp),
               TransformerBlock(args.heads, num_in=args.width, causal=True, fused=fused, dropout=drop, kv_heads=args.kv_heads,
                                rope=rotary, mlp=mlp),
               LayerNorm(args.width, fused=fused), Rows(), Dense(args.vocab, num_in=args.width, fused=fused)])
    # --ragged-train: the targets at dead positions carry this index and count for nothing
    loss_layer = CrossEntropyLoss(ignore_index=IGNORE if getattr(args, "ragged_train", False) else None, fused=fused)
    return Model(net=net, loss=loss_layer, optimizer=make_optimizer(args)), loss_layer


def make_optimizer(args):
    if not getattr(args, "adamw", False):
        return Adam(lr=args.lr)
    steps = args.num_ep * (args.n_train // args.batch_size)                 # cosine to the last step of the run
    schedule = ostep.Cosine(args.warmup, steps) if args.warmup > 0 else None
    return AdamW(lr=args.lr, weight_decay=args.weight_decay, max_norm=args.clip if args.clip > 0 else None, schedule=schedule,
                 fused=not args.composed)


def main(args):
    if args.seed >= 0:
        np.random.seed(args.seed)
    rng.manual_seed(max(args.seed, 0))                    # the device generator the dropout masks come from (host bookkeeping only)
    rs = np.random.RandomState(max(args.seed, 0))
    train_x, train_y = make_data(rs, args.n_train, args.seq, args.vocab, args.period)
    test_x, test_y = make_data(rs, args.n_test, args.seq, args.vocab, args.period)
    model, loss_layer = build(args)
    print("data: synthetic, %d sequences of %d tokens from %d, period %d; backend %s"
          % (len(train_x), args.seq, args.vocab, args.period, tn.backend_name()))
    history = []
    ragged = getattr(args, "ragged_train", False)
    for epoch in range(args.num_ep):
        t0, losses = time.time(), []
        live = 0
        for start in range(0, len(train_x) - args.batch_size + 1, args.batch_size):
            x = Tensor(train_x[start:start + args.batch_size])
            y = train_y[start:start + args.batch_size]
            lens = None
            if ragged:
                host, y = ragged_batch(rs, train_x[start:start + args.batch_size], y, args.seq)
                live += int(host.sum())
                if not getattr(args, "no_lens", False):
                    lens = da.lengths(host)                 # uploaded once per batch; every attention node reads it on the device
            model.zero_grad()
            loss = loss_layer.loss(model.forward(x, lens=lens), y.reshape(-1))
            loss.backward()
            model.step()
            losses.append(loss)
        mean = float(np.mean([float(l.values) for l in losses]))
        if ragged:
            print("         ragged batches: %d live tokens of %d, %.0f live tokens/s%s" % (
                live, len(losses) * args.batch_size * args.seq, live / (time.time() - t0),
                " (lengths NOT handed to the model: causal attention over the padding)" if getattr(args, "no_lens", False) else ""))
        model.set_phase("TEST")
        logits = np.asarray(model.forward(Tensor(test_x)).values).reshape(len(test_x), args.seq, args.vocab)
        model.set_phase("TRAIN")
        hit = np.argmax(logits, axis=2) == test_y
        accuracy = float(hit[:, args.period:].mean())         # the positions whose next token the context determines
        history.append((mean, accuracy))
        print("epoch %d: mean loss %.4f, accuracy on predictable positions %.4f, %.2f s" % (epoch, mean, accuracy, time.time() - t0))
        if isinstance(model.optimizer, AdamW):
            st = model.optimizer.state()                    # the optimizer's only read-back, once per epoch
            print("         step %d, lr %.3e, last gradient norm %.4f (factor %.4f), %d steps skipped"
                  % (st["t"], st["lr"], st["gnorm"], st["coef"], st["skipped"]))
    args.generation = None              # with --generate: (ids [rows, prompt + N], share of motif continuations)
    if args.generate <= 0:
        return history
    prompt_len = 2 * args.period
    chunk, second = getattr(args, "prefill_chunk", None), getattr(args, "second_turn", 0)
    total = args.generate + (args.period + second if second > 0 else 0)      # the second turn: `period` motif tokens, M new
    if prompt_len + total > args.seq:
        raise ValueError("--generate %d: %d prompt + %d new tokens exceed --seq %d (the learned positions, or the rotary tables)"
                         % (args.generate, prompt_len, total, args.seq))
    rows = test_x[:min(len(test_x), 8)]
    if args.ragged or args.eos is not None or args.capture:
        if chunk is not None or second > 0:
            raise ValueError("--prefill-chunk and --second-turn belong to the uniform path: no --ragged, --eos or --capture")
        lens = np.full(len(rows), prompt_len)
        if args.ragged:                                     # prompts of period .. 2 period tokens, the same in every run
            lens = args.period + np.arange(len(rows)) % (args.period + 1)
        out, ends = generate(model, rows[:, :prompt_len], args.generate, temperature=0.0, prompt_lens=lens, eos_id=args.eos,
                             capture=args.capture, return_lengths=True)
        new = np.stack([out[b, p:p + args.generate] for b, p in enumerate(lens)])
        motif = np.stack([rows[b, np.arange(p, p + args.generate) % args.period] for b, p in enumerate(lens)])
        live = np.arange(args.generate)[None, :] < (ends - lens)[:, None]          # up to and including an end of sequence
        share = float((new == motif)[live].mean())
        for b, row in enumerate(out):
            print("  %s | %s" % (" ".join("%2d" % t for t in row[:lens[b]]), " ".join("%2d" % t for t in row[lens[b]:ends[b]])))
        print("generated up to %d tokens for %d sequences (prompts of %d .. %d tokens): %.4f of them continue the motif"
              % (args.generate, len(out), lens.min(), lens.max(), share))
        args.generation = (out, share)
        return history
    kept = KVCache(args.seq, extend=True) if second > 0 else True       # the first turn's cache, kept for the second
    out = generate(model, rows[:, :prompt_len], args.generate, temperature=0.0, cache=kept, prefill_chunk=chunk)
    motif = rows[:, np.arange(prompt_len, prompt_len + args.generate) % args.period]     # what repeating the motif gives
    share = float((out[:, prompt_len:] == motif).mean())
    for row in out:
        print("  %s | %s" % (" ".join("%2d" % t for t in row[:prompt_len]), " ".join("%2d" % t for t in row[prompt_len:])))
    print("generated %d tokens for %d sequences: %.4f of them continue the motif" % (args.generate, len(out), share))
    args.generation = (out, share)
    args.second = None                  # with --second-turn: (ids [rows, 1 + period + M] of the second call, equal to one call's)
    if second > 0:
        # the cache holds every token but the last one generated; the second prompt is that token and the motif's next period
        at = prompt_len + args.generate
        turn = np.concatenate([out[:, -1:], rows[:, np.arange(at, at + args.period) % args.period]], axis=1)
        more = generate(model, turn, second, temperature=0.0, cache=kept)
        whole = generate(model, np.concatenate([out, turn[:, 1:]], axis=1), second, temperature=0.0)
        same = bool(np.array_equal(more[:, -second:], whole[:, -second:]))
        for row in more:
            print("  ... %s | %s" % (" ".join("%2d" % t for t in row[:-second]), " ".join("%2d" % t for t in row[-second:])))
        print("second turn: %d prompt + %d new tokens on the kept cache (%d rows now): %s one call on the concatenated prompt"
              % (turn.shape[1], second, kept.length, "the tokens of" if same else "DIFFERENT from"))
        args.second = (more, same)
    return history


def parse(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--num_ep", default=4, type=int)
    parser.add_argument("--lr", default=3e-3, type=float)
    parser.add_argument("--batch_size", default=64, type=int)
    parser.add_argument("--n_train", default=2048, type=int)
    parser.add_argument("--n_test", default=256, type=int)
    parser.add_argument("--seq", default=16, type=int)
    parser.add_argument("--vocab", default=16, type=int)
    parser.add_argument("--width", default=32, type=int)
    parser.add_argument("--heads", default=4, type=int)
    parser.add_argument("--kv-heads", dest="kv_heads", default=None, type=int, metavar="N",
                        help="grouped-query attention: N key / value heads shared by the --heads query heads (a divisor of it)")
    parser.add_argument("--rope", action="store_true",
                        help="rotary position embeddings (one Rotary shared by the blocks) instead of learned positions")
    parser.add_argument("--mlp", default="gelu", choices=("gelu", "swiglu", "geglu"),
                        help="feed-forward of the blocks: gelu (default), or the gated forms swiglu / geglu (one packed fc1)")
    parser.add_argument("--period", default=4, type=int)
    parser.add_argument("--seed", default=0, type=int)
    parser.add_argument("--dropout", default=0.0, type=float, help="dropout rate of the embedding and the blocks (0: none)")
    parser.add_argument("--generate", default=0, type=int, help="continue the first test sequences greedily by N tokens")
    parser.add_argument("--ragged", action="store_true", help="--generate: prompts of differing lengths (period .. 2 period tokens)")
    parser.add_argument("--eos", default=None, type=int, metavar="ID", help="--generate: a sequence ends at token ID")
    parser.add_argument("--capture", action="store_true", help="--generate: record the token step into a graph and replay it")
    parser.add_argument("--prefill-chunk", dest="prefill_chunk", default=None, type=int, metavar="C",
                        help="--generate: run the prompt in pieces of C tokens (the pieces after the first extend the cache)")
    parser.add_argument("--second-turn", dest="second_turn", default=0, type=int, metavar="M",
                        help="--generate: keep the cache and continue it by M more tokens in a second call")
    parser.add_argument("--ragged-train", dest="ragged_train", action="store_true",
                        help="train on right-padded batches: every sequence cut to a random length in [seq / 4, seq], the targets "
                             "beyond it ignored by the loss, the lengths handed to the model (model.forward(x, lens=))")
    parser.add_argument("--no-lens", dest="no_lens", action="store_true",
                        help="--ragged-train: keep the lengths from the model (the padded baseline; right for a causal model, wasteful)")
    parser.add_argument("--composed", action="store_true", help="fused=False: every part on its composed route")
    parser.add_argument("--adamw", action="store_true", help="AdamW on the device instead of Adam")
    parser.add_argument("--weight_decay", default=0.01, type=float, help="--adamw: decoupled weight decay")
    parser.add_argument("--clip", default=1.0, type=float, help="--adamw: clip the global gradient norm to this (0: none)")
    parser.add_argument("--warmup", default=0, type=int, help="--adamw: warm-up steps, then cosine decay to the last step (0: constant lr)")
    return parser.parse_args(argv)


if __name__ == "__main__":
    main(parse())
