"""Loss functions (reference: core/losses.py:8-32).

SoftmaxCrossEntropyLoss reproduces the reference's WHOLE-BATCH normalisation (max and sum-exp over all
m x c logits, core/losses.py:26-27), not a per-row softmax.  `fused=True` (default) runs it as
one node / three kernels; `fused=False` evaluates the literal 12-op expression through the autograd ops.
With a communicator the shards exchange one {max, sum-exp} pair so a data-parallel run equals the
single-process run on the global batch.

CrossEntropyLoss is NOT in the reference: the per-row softmax cross-entropy with integer targets that a token model needs
(ops.cross_entropy_).
"""

import numpy as np

from . import ops


class BaseLoss(object):

    def loss(self, predicted, actual):
        raise NotImplementedError


class SoftmaxCrossEntropyLoss(BaseLoss):

    def __init__(self, weight=None, fused=True, comm=None):
        self._weight = np.asarray(weight) if weight is not None else None
        self.fused = fused
        self.comm = comm

    def loss(self, logits, labels):
        if self._weight is not None:
            # the reference indexes the weight vector with the one-hot float matrix and raises
            # IndexError (core/losses.py:30-31); there is no defined behaviour to reproduce
            raise IndexError("arrays used as indices must be of integer (or boolean) type")
        if self.fused:
            return ops.softmax_nll_(logits, labels, comm=self.comm)
        if self.comm is not None and self.comm.world > 1:
            raise ValueError("the unfused loss has no data-parallel form; use fused=True")
        m = logits.shape[0]
        exps = ops.exp(logits - logits.max())
        p = exps / exps.sum()
        nll = -ops.log((p * labels).sum(1))
        return nll.sum() / m


class CrossEntropyLoss(BaseLoss):
    """Softmax cross-entropy over the LAST axis of logits [..., V] with INTEGER targets [...]: per row,
    log sum exp(x) - x[target]; `reduction` "mean" divides the sum by the number of counted rows, "sum" does not.  Rows whose
    target equals `ignore_index` contribute nothing and get a zero gradient; when every row is ignored the loss is 0.

    How it differs from SoftmaxCrossEntropyLoss, which is the reference's loss and stays what it is: that one normalises over
    the WHOLE batch (one max and one sum of exponentials over all m x c logits), takes one-hot float labels and divides by m;
    this one normalises each row on its own — the usual definition — takes class indices, knows `ignore_index`, and handles
    rows as wide as a vocabulary.  `fused=False` runs the composed route (max / exp / sum / log and an index gather)."""

    def __init__(self, ignore_index=None, reduction="mean", fused=True):
        from ..tokens import REDUCTIONS
        if reduction not in REDUCTIONS:
            raise ValueError("CrossEntropyLoss: reduction must be one of %s, got %r" % (REDUCTIONS, reduction))
        self.ignore_index, self.reduction, self.fused = ignore_index, reduction, fused

    def loss(self, logits, targets):
        return ops.cross_entropy_(logits, targets, ignore_index=self.ignore_index, reduction=self.reduction,
                                  route=None if self.fused else "composed")


class SquaredErrorLoss(BaseLoss):
    """((pred - target) ** 2).sum() / m — the loss test/test_autograd.py:119-121 builds from ops and the
    one BASELINE.json's 4096-wide autoencoder config uses."""

    def loss(self, predicted, actual):
        m = predicted.shape[0]
        err = predicted - actual
        return (err ** 2).sum() / m
