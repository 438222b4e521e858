"""Reference of the device metrics (csrc/dfd_metrics.hip, deepfakedetection_amd/metrics.py) in numpy and Python integers.

Everything the kernels return is a count, so everything here is an integer too; the only floating point is the final
division (auc) and the interpolation of the equal error rate, done in rationals and rounded once."""

from __future__ import annotations

from fractions import Fraction

import numpy as np


def split(scores, labels, positive: int = 1):
    """(positives' scores, negatives' scores): a sample is a negative when its label is anything but `positive`."""
    scores, labels = np.asarray(scores, dtype=np.float32), np.asarray(labels, dtype=np.int64)
    return scores[labels == positive], scores[labels != positive]


def two_u(scores, labels, positive: int = 1) -> int:
    """Twice the Mann-Whitney U with ties counted half: over the positives, 2 * #{negatives below} + #{negatives equal}."""
    pos, neg = split(scores, labels, positive)
    neg = np.sort(neg)
    below, upto = np.searchsorted(neg, pos, side="left"), np.searchsorted(neg, pos, side="right")
    return int(below.astype(np.int64).sum()) + int(upto.astype(np.int64).sum())


def two_u_by_groups(scores, labels, positive: int = 1) -> int:
    """The same number the way the kernel's contract states it: sum over tie groups of p_g * (cum_neg[g - 1] + cum_neg[g])."""
    scores, labels = np.asarray(scores, dtype=np.float32), np.asarray(labels, dtype=np.int64)
    _, inverse = np.unique(scores, return_inverse=True)
    groups = int(inverse.max()) + 1 if scores.size else 0
    p = np.bincount(inverse[labels == positive], minlength=groups)
    n = np.bincount(inverse[labels != positive], minlength=groups)
    total, seen = 0, 0
    for pg, ng in zip(p.tolist(), n.tolist()):
        total += pg * (2 * seen + ng)
        seen += ng
    return total


def auc(scores, labels, positive: int = 1) -> float | None:
    pos, neg = split(scores, labels, positive)
    if pos.size == 0 or neg.size == 0:
        return None
    return two_u(scores, labels, positive) / (2 * pos.size * neg.size)


def groups(scores, labels, positive: int = 1):
    """The kernel's outputs: (thr [G], cum_pos [G], cum_neg [G], stats = [P, N, G, nonfinite, two_u]).  A tie group is a maximal
    run of the ascending scores with s[i] == s[i + 1] under float comparison: -0.0 and +0.0 are one group and every NaN (sorted
    last) is its own.  With a NaN among the scores two_u is computed by the group formula all the same."""
    scores, labels = np.asarray(scores, dtype=np.float32), np.asarray(labels, dtype=np.int64)
    order = np.argsort(scores, kind="stable")
    s, is_pos = scores[order], labels[order] == positive
    if s.size == 0:
        return s, np.zeros(0, np.int64), np.zeros(0, np.int64), [0, 0, 0, 0, 0]
    ends = np.concatenate([s[1:] != s[:-1], [True]])
    cum_pos, cum_neg = np.cumsum(is_pos)[ends].astype(np.int64), np.cumsum(~is_pos)[ends].astype(np.int64)
    total, prev_pos, prev_neg = 0, 0, 0
    for cp, cn in zip(cum_pos.tolist(), cum_neg.tolist()):
        total += (cp - prev_pos) * (prev_neg + cn)
        prev_pos, prev_neg = cp, cn
    stats = [int(is_pos.sum()), int((~is_pos).sum()), int(ends.sum()), int((~np.isfinite(s)).sum()), total]
    return s[ends], cum_pos, cum_neg, stats


def roc_counts(scores, labels, positive: int = 1):
    """(fps, tps, thresholds) as sklearn.metrics.roc_curve(drop_intermediate=False) counts them before it prepends its first point
    and divides: the distinct scores descending, and the negatives / positives at or above each."""
    pos, neg = split(scores, labels, positive)
    thresholds = np.unique(np.asarray(scores, dtype=np.float32))[::-1]
    pos, neg = np.sort(pos), np.sort(neg)
    tps = pos.size - np.searchsorted(pos, thresholds, side="left")
    fps = neg.size - np.searchsorted(neg, thresholds, side="left")
    return fps.astype(np.int64), tps.astype(np.int64), thresholds


def sweep(scores, labels, cuts, positive: int = 1):
    """(tp, fp) per cut: the positives / negatives with float64(score) >= cut — numpy's promotion of float32 scores against
    float64 cuts."""
    pos, neg = split(scores, labels, positive)
    pos, neg = np.sort(pos.astype(np.float64)), np.sort(neg.astype(np.float64))
    cuts = np.asarray(cuts, dtype=np.float64)
    tp = pos.size - np.searchsorted(pos, cuts, side="left")
    fp = neg.size - np.searchsorted(neg, cuts, side="left")
    return tp.astype(np.int64), fp.astype(np.int64)


def best_threshold(scores, labels, cuts, positive: int = 1) -> float:
    """The first cut that maximises (tp / P + (N - fp) / N) / 2, compared as exact rationals."""
    pos, neg = split(scores, labels, positive)
    tp, fp = sweep(scores, labels, cuts, positive)
    P, N = max(int(pos.size), 1), max(int(neg.size), 1)
    best, where = None, 0
    for k, (a, b) in enumerate(zip(tp.tolist(), fp.tolist())):
        value = Fraction(a, P) + Fraction(int(neg.size) - b, N)
        if best is None or value > best:
            best, where = value, k
    return float(np.asarray(cuts, dtype=np.float64)[where])


def confusion(truth, pred, num_classes: int):
    """(counts int64 [J, J], pairs with a label outside [0, J))."""
    truth, pred = np.asarray(truth, dtype=np.int64), np.asarray(pred, dtype=np.int64)
    inside = (truth >= 0) & (truth < num_classes) & (pred >= 0) & (pred < num_classes)
    flat = np.bincount(truth[inside] * num_classes + pred[inside], minlength=num_classes * num_classes)
    return flat.reshape(num_classes, num_classes).astype(np.int64), int((~inside).sum())


def eer(scores, labels, positive: int = 1) -> float | None:
    """The point of the piecewise-linear ROC curve through (0, 0) where fpr = 1 - tpr, in rationals, rounded once."""
    fps, tps, _ = roc_counts(scores, labels, positive)
    pos, neg = split(scores, labels, positive)
    P, N = int(pos.size), int(neg.size)
    if P == 0 or N == 0:
        return None
    prev = (Fraction(0), Fraction(0))
    for f, t in zip(fps.tolist(), tps.tolist()):
        here = (Fraction(f, N), Fraction(t, P))
        h0, h1 = prev[0] + prev[1] - 1, here[0] + here[1] - 1
        if h1 >= 0:
            if h1 == 0:
                return float(here[0])
            w = -h0 / (h1 - h0)
            return float(prev[0] + w * (here[0] - prev[0]))
        prev = here
    raise AssertionError("the curve ends at (1, 1)")
