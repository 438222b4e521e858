"""Exact evaluation metrics on the device: ROC-AUC, equal error rate, a threshold sweep and the confusion matrix.

The scores of a validation or inference pass stay on the device (`ScoreBook`); `binary_roc` sorts them with torch.sort and
runs the counting kernels of csrc/dfd_metrics.hip through `kernels`.  What the kernels return are integers — the ROC curve by
tie group and twice the Mann-Whitney U with ties counted half — so AUC is one correctly rounded division of Python integers
and every figure derived here is a function of those integers alone: independent of the order of the samples, of the order
inside a run of equal scores and of the launch geometry.  The host reads the results once, after the last launch.

`ScoreBook` and `gather_scores` are plain torch (they run on the CPU and under gloo as well); the metrics themselves need a
HIP device, like every kernel front end.
"""

from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

from . import kernels as K

__all__ = ["RocResult", "ScoreBook", "binary_roc", "confusion", "eer_from_curve", "gather_scores", "ovr_auc"]


class ScoreBook:
    """Preallocated device buffers for the class probabilities (f32 [capacity, J]), predictions and targets (int64
    [capacity]) of one pass over a split.  append() copies a batch to a host-known offset: no synchronisation."""

    def __init__(self, capacity: int, num_classes: int, device) -> None:
        self.capacity, self.num_classes, self.count = int(capacity), int(num_classes), 0
        self._probs = torch.empty((self.capacity, self.num_classes), dtype=torch.float32, device=device)
        self._preds = torch.empty(self.capacity, dtype=torch.int64, device=device)
        self._targets = torch.empty(self.capacity, dtype=torch.int64, device=device)

    def append(self, probs: torch.Tensor | None, preds: torch.Tensor | None, targets: torch.Tensor) -> None:
        n = int(targets.shape[0])
        if self.count + n > self.capacity:
            raise ValueError(f"ScoreBook overflow: {self.count} + {n} rows into a capacity of {self.capacity}")
        rows = slice(self.count, self.count + n)
        for dst, src, shape in ((self._probs, probs, (n, self.num_classes)), (self._preds, preds, (n,)), (self._targets, targets, (n,))):
            if src is None:
                continue
            if tuple(src.shape) != shape:
                raise ValueError(f"ScoreBook.append: expected shape {shape}, got {tuple(src.shape)}")
            dst[rows].copy_(src, non_blocking=True)
        self.count += n

    def reset(self) -> None:
        self.count = 0

    @property
    def probs(self) -> torch.Tensor:
        return self._probs[: self.count]

    @property
    def preds(self) -> torch.Tensor:
        return self._preds[: self.count]

    @property
    def targets(self) -> torch.Tensor:
        return self._targets[: self.count]


def eer_from_curve(fps: np.ndarray, tps: np.ndarray, n_pos: int, n_neg: int) -> float | None:
    """Equal error rate from the integer ROC curve (curve()'s counts, thresholds descending): the point of the piecewise-linear
    curve through (0, 0) where fpr = 1 - tpr.  fpr + tpr - 1 = a / (P N) with the integer a = fps P + tps N - P N, which never
    decreases along the curve and runs from -P N to P N: the crossing lies on the first segment that ends with a >= 0, and is
    interpolated there in f64.  None when a class is absent."""
    P, N = int(n_pos), int(n_neg)
    if P == 0 or N == 0:
        return None
    a = np.asarray(fps, dtype=np.int64) * P + np.asarray(tps, dtype=np.int64) * N - P * N
    i = int(np.argmax(a >= 0))                      # a[-1] = P N > 0: there is one
    f1, a1 = int(fps[i]), int(a[i])
    f0, a0 = (int(fps[i - 1]), int(a[i - 1])) if i else (0, -P * N)
    if a1 == 0:
        return f1 / N
    t = -a0 / (a1 - a0)
    return (f0 + t * (f1 - f0)) / N


@dataclass
class RocResult:
    """What binary_roc found.  auc is None when a class is absent and nan when scores are not finite (strict=False)."""

    auc: float | None
    two_u: int
    n_pos: int
    n_neg: int
    groups: int
    nonfinite: int
    cuts: np.ndarray | None = None                  # the cut points of the sweep (f64), with tp / fp per cut
    tp: np.ndarray | None = None
    fp: np.ndarray | None = None
    _device: tuple | None = field(default=None, repr=False)          # (thr, cum_pos, cum_neg) on the device
    _curve: tuple | None = field(default=None, repr=False)
    _eer: tuple | None = field(default=None, repr=False)

    def curve(self) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(fps, tps, thresholds) as sklearn.metrics.roc_curve(drop_intermediate=False) counts them, without its leading
        point: thresholds are the distinct scores in descending order, fps / tps the negatives / positives at or above each.
        Copied from the device once."""
        if self._curve is None:
            thr, cum_pos, cum_neg = (t[: self.groups].cpu().numpy() for t in self._device)
            below_pos = np.concatenate([[0], cum_pos])[: self.groups].astype(np.int64)      # counts below each group
            below_neg = np.concatenate([[0], cum_neg])[: self.groups].astype(np.int64)
            self._curve = ((self.n_neg - below_neg)[::-1].copy(), (self.n_pos - below_pos)[::-1].copy(), thr[::-1].copy())
        return self._curve

    @property
    def eer(self) -> float | None:
        if self._eer is None:
            if self.n_pos == 0 or self.n_neg == 0:
                value = None
            elif self.nonfinite:
                value = float("nan")
            else:
                fps, tps, _ = self.curve()
                value = eer_from_curve(fps, tps, self.n_pos, self.n_neg)
            self._eer = (value,)
        return self._eer[0]

    def balanced_accuracy(self) -> np.ndarray:
        """(tp / P + (N - fp) / N) / 2 per cut, in the arithmetic of orchestrator.best_balanced_accuracy_threshold."""
        if self.cuts is None:
            raise ValueError("binary_roc was called without cuts")
        recall_pos = self.tp / max(self.n_pos, 1)
        recall_neg = (self.n_neg - self.fp) / max(self.n_neg, 1)
        return (recall_pos + recall_neg) / 2.0

    def best_balanced_accuracy_threshold(self) -> float:
        """The first cut that maximises the balanced accuracy of (score >= cut)."""
        return float(self.cuts[int(np.argmax(self.balanced_accuracy()))])


def binary_roc(scores: torch.Tensor, labels: torch.Tensor, positive: int = 1, cuts=None, strict: bool = True) -> RocResult:
    """ROC statistics of `scores` (float [n] on the device, higher = more `positive`) against int64 `labels`: a sample is a
    positive when its label equals `positive`, a negative otherwise.  `cuts`: ascending thresholds (at most kernels.ROC_MAX_CUTS)
    for which the positives / negatives at or above each are counted, compared in f64.  One sort, four or five launches, then
    one read of the results.  Non-finite scores raise ValueError under `strict`; otherwise auc (and eer) are nan."""
    scores = scores.detach().reshape(-1).float()
    labels = labels.detach().reshape(-1).to(torch.int64)
    if scores.numel() != labels.numel():
        raise ValueError(f"binary_roc: {scores.numel()} scores for {labels.numel()} labels")
    ordered, order = torch.sort(scores)
    thr, cum_pos, cum_neg, stats = K.roc_curve(ordered.contiguous(), labels[order].contiguous(), positive)
    sweep = None
    if cuts is not None:
        cuts_np = np.ascontiguousarray(np.asarray(cuts, dtype=np.float64).reshape(-1))
        if cuts_np.size > 1 and not bool(np.all(cuts_np[1:] >= cuts_np[:-1])):
            raise ValueError("binary_roc: cuts must ascend")
        cuts_dev = torch.from_numpy(cuts_np).to(scores.device, non_blocking=True)
        sweep = K.roc_sweep(thr, cum_pos, cum_neg, stats, cuts_dev)
    n_pos, n_neg, groups, nonfinite, two_u = (int(v) for v in stats.tolist())             # the one synchronisation
    if nonfinite and strict:
        raise ValueError(f"binary_roc: {nonfinite} of {scores.numel()} scores are NaN or infinite")
    if n_pos == 0 or n_neg == 0:
        auc = None
    elif nonfinite:
        auc = float("nan")
    else:
        auc = two_u / (2 * n_pos * n_neg)                 # Python integers: one correctly rounded division
    res = RocResult(auc=auc, two_u=two_u, n_pos=n_pos, n_neg=n_neg, groups=groups, nonfinite=nonfinite,
                    _device=(thr, cum_pos, cum_neg))
    if sweep is not None:
        res.cuts, res.tp, res.fp = cuts_np, sweep[0].cpu().numpy(), sweep[1].cpu().numpy()
    return res


def ovr_auc(probs: torch.Tensor, targets: torch.Tensor, num_classes: int, strict: bool = True) -> float | None:
    """Macro average of the one-vs-rest AUC over the columns of `probs` [n, J] (sklearn's roc_auc_score(multi_class="ovr"));
    None unless every class occurs in `targets`."""
    if probs.dim() != 2 or probs.shape[1] != num_classes:
        raise ValueError(f"ovr_auc: expected probabilities [n, {num_classes}], got {tuple(probs.shape)}")
    aucs = []
    for j in range(num_classes):
        res = binary_roc(probs[:, j], targets, positive=j, strict=strict)
        if res.n_pos == 0:
            return None
        aucs.append(res.auc)
    if any(a is None for a in aucs):
        return None
    return float(sum(aucs) / len(aucs))


def confusion(truth: torch.Tensor, pred: torch.Tensor, num_classes: int) -> torch.Tensor:
    """int64 [J, J] counts on the device, row = truth, column = prediction; a label outside [0, J) raises ValueError."""
    counts, oob = K.confusion_counts(truth.detach().reshape(-1).to(torch.int64).contiguous(),
                                     pred.detach().reshape(-1).to(torch.int64).contiguous(), num_classes)
    bad = int(oob.item())
    if bad:
        raise ValueError(f"confusion: {bad} pairs have a label outside [0, {num_classes})")
    return counts


def gather_scores(scores: torch.Tensor, labels: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """Under an initialised process group of more than one rank: every rank's (scores [n_r, ...], labels [n_r]) concatenated
    in rank order, on every rank — one all_gather of the counts and one of each buffer, padded to the largest count.  The
    identity otherwise.  Validation shards are disjoint (ShardedSampler(pad=False)), so the result is the split exactly once."""
    import torch.distributed as dist

    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return scores, labels
    world = dist.get_world_size()
    count = torch.tensor([scores.shape[0]], dtype=torch.int64, device=scores.device)
    counts = [torch.zeros_like(count) for _ in range(world)]
    dist.all_gather(counts, count)
    counts = [int(c.item()) for c in counts]
    width = max(max(counts), 1)

    def gather(t: torch.Tensor) -> torch.Tensor:
        padded = t.new_zeros((width,) + tuple(t.shape[1:]))
        padded[: t.shape[0]] = t
        parts = [torch.empty_like(padded) for _ in range(world)]
        dist.all_gather(parts, padded)
        return torch.cat([p[:c] for p, c in zip(parts, counts)])

    return gather(scores), gather(labels)
