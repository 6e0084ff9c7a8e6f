"""Streaming metrics of the supervised models (tf_euler/python/utils/metrics.py): f1, acc and auc
over integer counters that live on the device and that the fused loss head adds to
(ops.supervise_loss / Graph.supervise_loss, euler_amd/csrc/supervise.h) - no host read per step.
get(name) mirrors the reference's table; the ranking metrics delegate to ops.rank_metric."""
import functools

import torch

from . import ops

EPSILON = 1e-7
NAMES = ("acc", "auc", "f1", "mrr", "hit1", "hit3", "hit10", "mr")
_STREAMING = ("f1", "acc", "auc")


class Streaming(object):
    """A streaming "f1", "acc" or "auc" (metrics.py:23-48 of the reference over tf.metrics): five
    int64 device counters tp, fp, fn, correct, total - and for auc two histograms [2, T + 1] of
    the predictions' buckets among tf.metrics.auc's num_thresholds thresholds (row 0: label != 0,
    row 1: label == 0).  Pass it as `metric` to ops.supervise_loss / Graph.supervise_loss: every
    call adds its batch with integer atomics.  The prediction is floor(p + 0.5) in fp32; tp / fp /
    fn cast label and prediction to bool, acc counts label == prediction, so a soft label is never
    correct.  The histograms bucket p = sigmoid(logit) once, where auc_score of the reference
    applies sigmoid a second time (a monotone map: only the resolution differs).
    value(): a 0-d float64 tensor on the device, no host wait.  reset(): the counters back to 0.
    The counters are allocated on the device of the first call (or `device`)."""

    def __init__(self, name, num_thresholds=5000, device=None):
        if name not in _STREAMING:
            raise ValueError("metrics.Streaming: name is one of %s" % ", ".join(_STREAMING))
        if name == "auc" and int(num_thresholds) < 2:
            raise ValueError("metrics.Streaming: auc needs 2 thresholds at least")
        self.name = name
        self.num_thresholds = int(num_thresholds)
        self.counts = self.hist = None
        if device is not None:
            self._buffers(torch.device(device))

    def _buffers(self, device):
        """-> (counts [5], hist [2, T + 1] | None, T) on `device`"""
        if self.counts is None:
            self.counts = torch.zeros(5, dtype=torch.int64, device=device)
            if self.name == "auc":
                self.hist = torch.zeros((2, self.num_thresholds + 1), dtype=torch.int64, device=device)
        elif self.counts.device != device:
            raise RuntimeError("metrics.Streaming: the counters live on %s, not %s" % (self.counts.device, device))
        return self.counts, self.hist, self.num_thresholds

    def reset(self):
        if self.counts is not None:
            self.counts.zero_()
            if self.hist is not None:
                self.hist.zero_()
        return self

    def value(self):
        if self.counts is None:
            raise RuntimeError("metrics.Streaming: no call has added to this metric yet")
        c = self.counts.to(torch.float64)
        if self.name == "f1":
            tp, fp, fn = c[0], c[1], c[2]
            precision, recall = tp / (EPSILON + tp + fp), tp / (EPSILON + tp + fn)
            return 2.0 * precision * recall / (precision + recall + EPSILON)
        if self.name == "acc":
            return c[3] / c[4]
        # tp_i = the positives above threshold i = those in buckets > i: reverse cumulative sums
        above = torch.flip(torch.cumsum(torch.flip(self.hist, [1]), 1), [1])[:, 1:].to(torch.float64)
        total = self.hist.sum(1).to(torch.float64)
        tp, fp = above[0], above[1]
        fn, tn = total[0] - tp, total[1] - fp
        tpr = (tp + EPSILON) / (tp + fn + EPSILON)
        fpr = fp / (fp + tn + EPSILON)
        return ((fpr[:-1] - fpr[1:]) * (tpr[:-1] + tpr[1:]) / 2.0).sum()


def get(name):
    """The reference's metrics.get(name): "f1" / "acc" / "auc" -> a factory of Streaming objects
    (call it once, pass the object to supervise_loss at every step); "mrr" / "mr" / "hit1" /
    "hit3" / "hit10" -> a function of skipgram_loss's ranks (ops.rank_metric); else None."""
    if name in _STREAMING:
        return functools.partial(Streaming, name)
    if name in NAMES:
        return functools.partial(ops.rank_metric, name)
    return None
