"""Exact evaluation metrics on the device: ROC-AUC, equal error rate, a threshold sweep, the confusion matrix, and the
calibration of the probabilities (reliability bins, ECE / MCE, Brier score, NLL and a fitted temperature).

The scores of a validation or inference pass stay on the device (`ScoreBook`); `binary_roc` sorts them with torch.sort and
runs the counting kernels of csrc/dfd_metrics.hip through `kernels`.  What the kernels return are integers — the ROC curve by
tie group and twice the Mann-Whitney U with ties counted half — so AUC is one correctly rounded division of Python integers
and every figure derived here is a function of those integers alone: independent of the order of the samples, of the order
inside a run of equal scores and of the launch geometry.  The host reads the results once, after the last launch.

`calibration` bins the top-label confidence with csrc/dfd_calib.hip: the bins hold integers (rows, right predictions and the
confidences as multiples of 2^-32), so ECE and MCE are again one division of Python integers each.  `fit_temperature` finds
the single temperature T (Guo et al. 2017) that minimises the NLL of softmax(z / T): the NLL is convex in beta = 1 / T, and
one launch evaluates it with its derivative for up to kernels.CALIB_MAX_BETAS values of beta, so the fit is a bracketing
search with one read-back per round and no optimiser.

`fuse` combines the logits of K models with csrc/dfd_fuse.hip: a log-linear pool softmax(sum_k a_k z_k) or a linear pool of the
members' probabilities.  `fit_fusion` fits the a_k of the log-linear pool on held-out logits: the NLL is convex in a, one launch
returns it with its gradient and Hessian for eight step lengths at once, so the fit is a damped Newton method with one read-back
per iteration.  `diversity` counts how the members' right and wrong predictions coincide; every figure it returns is one division
of Python integers.

`group_ids` turns the sample paths of a split into group ids on the host (the video a frame was cut from), `group_pool` pools the
rows of every group into one row with csrc/dfd_group.hip (exact integer sums, or the member row with the largest positive score),
and `bootstrap(groups=...)` resamples whole groups instead of samples: the cluster bootstrap, for samples that are correlated
inside a group.

`ScoreBook`, `group_ids` and `gather_scores` are plain torch / numpy (they run on the CPU and under gloo as well); the metrics themselves need a
HIP device, like every kernel front end.
"""

from __future__ import annotations

import os
import re
from dataclasses import dataclass, field

import numpy as np
import torch

from . import kernels as K

__all__ = ["BootstrapResult", "CalibrationResult", "DeltaResult", "DiversityResult", "FusionFit", "GroupScores", "RocResult", "ScoreBook",
           "TemperatureFit", "apply_temperature", "binary_roc", "boot_values", "bootstrap", "calibration", "confusion", "diversity",
           "eer_from_curve", "fit_fusion", "fit_temperature", "fuse", "gather_scores", "group_ids", "group_pool", "mean_nll", "ovr_auc",
           "paired_delta", "percentile_interval"]


class ScoreBook:
    """Preallocated device buffers for the class probabilities (f32 [capacity, J]), predictions and targets (int64
    [capacity]) of one pass over a split.  append() copies a batch to a host-known offset: no synchronisation.
    keep_logits: a fourth buffer for the logits (f32 [capacity, J]), which calibration needs (fit_temperature)."""

    def __init__(self, capacity: int, num_classes: int, device, keep_logits: bool = False) -> None:
        self.capacity, self.num_classes, self.count = int(capacity), int(num_classes), 0
        self._logits = torch.empty((self.capacity, self.num_classes), dtype=torch.float32, device=device) if keep_logits else None
        self._probs = torch.empty((self.capacity, self.num_classes), dtype=torch.float32, device=device)
        self._preds = torch.empty(self.capacity, dtype=torch.int64, device=device)
        self._targets = torch.empty(self.capacity, dtype=torch.int64, device=device)

    def append(self, probs: torch.Tensor | None, preds: torch.Tensor | None, targets: torch.Tensor,
               logits: torch.Tensor | None = None) -> None:
        n = int(targets.shape[0])
        if logits is not None and self._logits is None:
            raise ValueError("ScoreBook.append: logits handed to a book built without keep_logits")
        if self.count + n > self.capacity:
            raise ValueError(f"ScoreBook overflow: {self.count} + {n} rows into a capacity of {self.capacity}")
        rows = slice(self.count, self.count + n)
        for dst, src, shape in ((self._probs, probs, (n, self.num_classes)), (self._preds, preds, (n,)), (self._targets, targets, (n,)),
                                (self._logits, logits, (n, self.num_classes))):
            if src is None:
                continue
            if tuple(src.shape) != shape:
                raise ValueError(f"ScoreBook.append: expected shape {shape}, got {tuple(src.shape)}")
            dst[rows].copy_(src, non_blocking=self._targets.is_cuda)    # a host book is read back at once: no pending copy
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

    @property
    def logits(self) -> torch.Tensor:
        if self._logits is None:
            raise ValueError("ScoreBook.logits: the book was built without keep_logits")
        return self._logits[: self.count]


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
    return _roc_of_sorted(ordered.contiguous(), labels[order].contiguous(), positive, cuts, strict)


def _roc_of_sorted(scores: torch.Tensor, labels: torch.Tensor, positive: int, cuts, strict: bool) -> RocResult:
    """binary_roc behind its sort: f32 [n] scores ascending and their int64 labels in that order."""
    thr, cum_pos, cum_neg, stats = K.roc_curve(scores, labels, positive)
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


BOOT_METRICS = ("auc", "eer", "accuracy", "balanced_accuracy", "tpr", "fpr", "hit_rate")


def boot_values(stats: np.ndarray, metric: str) -> np.ndarray:
    """One metric of every resample from kernels.boot_stats' integers [..., BOOT_STATS_LEN]: f64 of the leading shape.  Every
    value is one division of integers below 2^53 (the equal error rate: eer_from_curve's arithmetic on the segment's two ends);
    a resample with a class absent gives NaN for every metric but hit_rate (hits / n; NaN only for n == 0)."""
    if metric not in BOOT_METRICS:
        raise ValueError(f"bootstrap: metric must be one of {', '.join(BOOT_METRICS)}, got {metric!r}")
    s = np.asarray(stats, dtype=np.int64)
    P, N, two_u, tp, fp, hits, f0, t0, f1, t1 = (s[..., k] for k in range(K.BOOT_STATS_LEN))
    with np.errstate(invalid="ignore", divide="ignore"):
        if metric == "hit_rate":
            return np.where(P + N > 0, hits / np.maximum(P + N, 1), np.nan)
        both = (P > 0) & (N > 0)
        Ps, Ns = np.maximum(P, 1), np.maximum(N, 1)
        if metric == "auc":
            value = two_u / (2 * Ps * Ns)
        elif metric == "accuracy":
            value = (tp + N - fp) / (Ps + Ns)
        elif metric == "balanced_accuracy":
            value = (tp * N + (N - fp) * P) / (2 * Ps * Ns)
        elif metric == "tpr":
            value = tp / Ps
        elif metric == "fpr":
            value = fp / Ns
        else:
            a0, a1 = f0 * P + t0 * N - P * N, f1 * P + t1 * N - P * N        # a0 < 0 <= a1 on the segment
            t = -a0 / np.where(a1 - a0 != 0, a1 - a0, 1)
            value = np.where(a1 == 0, f1 / Ns, (f0 + t * (f1 - f0)) / Ns)
        return np.where(both, value, np.nan)


def percentile_interval(values: np.ndarray, level: float) -> tuple[float, float] | None:
    """np.quantile(valid, [(1 - level) / 2, (1 + level) / 2]) over the values that are not NaN; None when there is none."""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    v = v[~np.isnan(v)]
    if v.size == 0:
        return None
    lo, hi = np.quantile(v, [(1.0 - level) / 2.0, (1.0 + level) / 2.0])
    return float(lo), float(hi)


@dataclass
class DeltaResult:
    """A paired comparison of two members (BootstrapResult.delta): the difference of the point figures, the percentile interval of
    the per-resample differences (None without a valid resample), the two-sided p value and the resamples it rests on."""

    metric: str
    point: float | None
    lo: float | None
    hi: float | None
    p: float
    valid: int


def paired_delta(metric: str, point_a: float | None, point_b: float | None, values_a: np.ndarray, values_b: np.ndarray,
                 level: float) -> DeltaResult:
    """DeltaResult of two members' per-resample values over the same resamples: d = a - b where neither is NaN, and
    p = min(1, 2 min(#{d <= 0} + 1, #{d >= 0} + 1) / (valid + 1))."""
    d = np.asarray(values_a, dtype=np.float64) - np.asarray(values_b, dtype=np.float64)
    d = d[~np.isnan(d)]
    interval = percentile_interval(d, level)
    lo, hi = interval if interval is not None else (None, None)
    p = min(1.0, 2 * min(int((d <= 0).sum()) + 1, int((d >= 0).sum()) + 1) / (d.size + 1))
    point = None if point_a is None or point_b is None else point_a - point_b
    return DeltaResult(metric, point, lo, hi, p, int(d.size))


@dataclass
class BootstrapResult:
    """What bootstrap found: kernels.boot_stats' integers of every member and resample (numpy int64 [M, B, BOOT_STATS_LEN]), the
    settings, and per member the point figures of the full sample (a dict over BOOT_METRICS; None where a figure does not exist)."""

    stats: np.ndarray
    replicates: int
    seed: int
    level: float
    point: list
    clusters: int | None = None                     # the groups a resample draws (the cluster bootstrap); None: it draws samples

    def values(self, metric: str) -> np.ndarray:
        """f64 [M, B]: the metric of every member in every resample (boot_values)."""
        return boot_values(self.stats, metric)

    def degenerate(self, member: int = 0) -> int:
        """The resamples that lost a class."""
        s = self.stats[member]
        return int(((s[:, K.BOOT_P] == 0) | (s[:, K.BOOT_N] == 0)).sum())

    def interval(self, metric: str, member: int = 0) -> tuple[float, float] | None:
        """The percentile interval of `level` over the resamples where the metric exists; None when there is none."""
        return percentile_interval(self.values(metric)[member], self.level)

    def delta(self, metric: str, a: int, b: int) -> DeltaResult:
        """Member a minus member b, paired by resample (paired_delta)."""
        values = self.values(metric)
        return paired_delta(metric, self.point[a][metric], self.point[b][metric], values[a], values[b], self.level)


def _point_figures(roc: RocResult, hits: int | None, n: int) -> dict:
    """The full sample's figures in boot_values' arithmetic; roc carries one cut or none."""
    P, N = roc.n_pos, roc.n_neg
    out = dict.fromkeys(BOOT_METRICS)
    if hits is not None and n:
        out["hit_rate"] = hits / n
    if P and N:
        out["auc"], out["eer"] = roc.auc, roc.eer
        if roc.cuts is not None:
            tp, fp = int(roc.tp[0]), int(roc.fp[0])
            out.update(accuracy=(tp + N - fp) / (P + N), balanced_accuracy=(tp * N + (N - fp) * P) / (2 * P * N), tpr=tp / P, fpr=fp / N)
    return out


def bootstrap(scores, labels: torch.Tensor, *, positive: int = 1, cut=None, hits: torch.Tensor | None = None, replicates: int = 2000,
              seed: int = 0, level: float = 0.95, groups: torch.Tensor | None = None) -> BootstrapResult:
    """The nonparametric bootstrap of the ROC figures: `replicates` resamples of the n samples, drawn on the device by the rule of
    include/dfd_hip.h (Philox4x32-10 keyed by `seed`), each judged by kernels.boot_stats.  scores: one float tensor [n] on the
    device or a list of M <= kernels.BOOT_MAX_MEMBERS over the same samples, which then share every resample (BootstrapResult.delta
    compares them pairwise).  cut: the threshold of accuracy / balanced_accuracy / tpr / fpr (score >= cut predicts `positive`,
    compared in f64), one number or one per member; it is held fixed, not chosen again per resample.  hits: optional [n] flags
    (nonzero = this sample was judged right) behind hit_rate.  Each member is sorted once; the resamples are multiplicities over
    that order, so none of them sorts.  Non-finite scores raise ValueError.  One read-back after the last launch.
    groups: integer group ids [n] (the video of each frame, ids >= 0) turn this into the cluster bootstrap: a resample draws
    G = max id + 1 whole groups by the same rule and every sample counts as often as its group was drawn, which is the right unit
    when the samples of a group are correlated.  G and the largest group are read back once before the launches."""
    members = [scores] if isinstance(scores, torch.Tensor) else list(scores)
    if not 1 <= len(members) <= K.BOOT_MAX_MEMBERS:
        raise ValueError(f"bootstrap: takes 1..{K.BOOT_MAX_MEMBERS} score vectors, got {len(members)}")
    members = [m.detach().reshape(-1).float() for m in members]
    labels = labels.detach().reshape(-1).to(torch.int64)
    n, count, B = labels.numel(), len(members), int(replicates)
    if any(m.numel() != n for m in members):
        raise ValueError(f"bootstrap: {[m.numel() for m in members]} scores for {n} labels")
    if not 1 <= n <= K.BOOT_MAX_N or not 1 <= B <= K.BOOT_MAX_REPLICATES or not 0.0 < float(level) < 1.0:
        raise ValueError(f"bootstrap: takes 1..{K.BOOT_MAX_N} samples, 1..{K.BOOT_MAX_REPLICATES} replicates and 0 < level < 1, got "
                         f"{n}, {B}, {level!r}")
    cuts = list(cut) if isinstance(cut, (list, tuple)) else [cut] * count
    if len(cuts) != count or any(c is not None and not np.isfinite(float(c)) for c in cuts):
        raise ValueError(f"bootstrap: cut must be one finite number or one per member ({count}), got {cut!r}")
    if hits is not None and hits.numel() != n:
        raise ValueError(f"bootstrap: {hits.numel()} hits for {n} labels")
    is_positive = (labels == int(positive)).to(torch.uint8)
    hit = (hits.detach().reshape(-1) != 0).to(torch.uint8) if hits is not None else None
    ordered, perms, rocs = [], [], []
    for m, c in zip(members, cuts):
        s, order = torch.sort(m)
        ordered.append(s.contiguous())
        perms.append(order.to(torch.int32).contiguous())
        rocs.append(_roc_of_sorted(ordered[-1], labels[order].contiguous(), int(positive), None if c is None else [float(c)], True))
    clusters = None
    if groups is not None:
        ids = groups.detach().reshape(-1).to(device=labels.device, dtype=torch.int32).contiguous()
        if ids.numel() != n:
            raise ValueError(f"bootstrap: {ids.numel()} group ids for {n} labels")
        uniq, sizes = torch.unique(ids, return_counts=True)
        low, high, largest = (int(v) for v in torch.stack([uniq.min().long(), uniq.max().long(), sizes.max()]).tolist())   # the extra read-back
        if low < 0:
            raise ValueError(f"bootstrap: group ids must be >= 0, got {low}")
        clusters = high + 1
        stats_d = K.boot_stats_grouped(ordered, perms, is_positive, ids, clusters, largest, B, seed, cuts, hit)
    else:
        stats_d = K.boot_stats(ordered, perms, is_positive, B, seed, cuts, hit)
    total_hits = hit.sum(dtype=torch.int64).reshape(1) if hit is not None else stats_d.new_zeros(1)
    packed = torch.cat([stats_d.reshape(-1), total_hits]).cpu().numpy()   # the one read-back of the resamples
    stats = packed[:-1].reshape(count, B, K.BOOT_STATS_LEN).copy()
    n_hits = int(packed[-1]) if hit is not None else None
    return BootstrapResult(stats, B, int(seed), float(level), [_point_figures(r, n_hits, n) for r in rocs], clusters)


GROUP_POOLS = {"mean": K.GROUP_MEAN, "vote": K.GROUP_VOTE, "max": K.GROUP_MAX}


@dataclass
class GroupScores:
    """What group_pool found, on the device: one row per group (probs f32 [G, J], preds / targets int64 [G], sizes int32 [G]; an
    empty group holds zeros, pred 0, target -1, size 0) and info = the rows left out as invalid, the rows left out for an id out of
    range, the groups with mixed targets (always 0: they raise) and the empty groups, as Python integers."""

    probs: torch.Tensor
    preds: torch.Tensor
    targets: torch.Tensor
    sizes: torch.Tensor
    info: tuple


def group_pool(probs: torch.Tensor, groups: torch.Tensor, targets: torch.Tensor, mode: str = "mean", positive: int = 1,
               num_groups: int | None = None) -> GroupScores:
    """Pool the rows of every group (the frames of a video) into one row with kernels.group_pool: `mean` of the probabilities,
    `vote` = the share of rows whose arg max is each class, `max` = the member row with the largest probs[:, positive].  mean and
    vote are sums of integers (multiples of 2^-32), so the pooled bits do not depend on the order of the rows.  groups: integer ids
    [n]; num_groups: G (default: the largest id + 1, one more read-back).  A group is judged against its smallest member target; a
    group whose members disagree raises ValueError.  One read-back of `info` after the last launch."""
    if mode not in GROUP_POOLS:
        raise ValueError(f"group_pool: mode must be one of {', '.join(GROUP_POOLS)}, got {mode!r}")
    probs = probs.detach().float().contiguous()
    targets = targets.detach().reshape(-1).to(torch.int64).contiguous()
    ids = groups.detach().reshape(-1).to(device=probs.device, dtype=torch.int32).contiguous()
    G = int(ids.max().item()) + 1 if num_groups is None else int(num_groups)
    pooled, preds, tgt, sizes, info_d = K.group_pool(probs, ids, targets, G, GROUP_POOLS[mode], positive)
    info = tuple(int(v) for v in info_d.tolist())
    if info[K.GROUP_MIXED]:
        raise ValueError(f"group_pool: {info[K.GROUP_MIXED]} of {G} groups hold rows with different targets")
    return GroupScores(pooled, preds, tgt, sizes, info)


def group_ids(paths, root, key: str = "parent", pattern: str | None = None) -> tuple[np.ndarray, int, list[str]]:
    """The group (video) of every file of a split, on the host: (int32 ids [n], G, the groups' names).  Ids are dense, in order of
    first appearance.  The class directory is part of every key, so a video name under two classes gives two groups.
    key="parent": the file's directory relative to `root`; a file lying directly in a class directory is a group of its own.
    key="regex": (that directory, group 1 of re.fullmatch(pattern, stem)); a stem that does not match is a group of its own."""
    if key not in ("parent", "regex"):
        raise ValueError(f"group_ids: key must be 'parent' or 'regex', got {key!r}")
    if key == "regex":
        if not pattern:
            raise ValueError("group_ids: key='regex' needs a pattern")
        rx = re.compile(pattern)
        if rx.groups < 1:
            raise ValueError(f"group_ids: the pattern {pattern!r} has no capture group")
    root = os.path.normpath(os.fspath(root))
    table: dict = {}
    ids = np.empty(len(paths), dtype=np.int32)
    for i, path in enumerate(paths):
        rel = os.path.relpath(os.path.normpath(os.fspath(path)), root).replace(os.sep, "/")
        folder, _, name = rel.rpartition("/")
        video = None
        if key == "parent":
            if "/" in folder:                                           # below the class directory: the directory is the video
                video = folder
        else:
            m = rx.fullmatch(os.path.splitext(name)[0])
            if m is not None and m.group(1) is not None:
                video = f"{folder}/{m.group(1)}"
        ident = ("group", video) if video is not None else ("file", rel)       # a file of its own never merges with a video's key
        ids[i] = table.setdefault(ident, len(table))
    names = [k[1] for k in table]
    return ids, len(table), names


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


Q_ONE = 1 << 32                 # the confidences are summed as integers q = llrint(conf * 2^32)


@dataclass
class CalibrationResult:
    """What calibration found.  ece / mce / brier / accuracy are None when no row is valid.  count, accuracy and confidence are
    the per-bin arrays of the reliability diagram (nan in an empty bin); bins is the device's integer table [M, 3]."""

    ece: float | None
    mce: float | None
    brier: float | None
    accuracy_total: float | None
    valid: int
    nonfinite: int
    count: np.ndarray
    accuracy: np.ndarray
    confidence: np.ndarray
    bins: np.ndarray
    brier_sum: float


def calibration(probs: torch.Tensor, targets: torch.Tensor, bins: int = 15) -> CalibrationResult:
    """Expected and maximum calibration error of the top-label confidence over `bins` equal-width right-closed bins (Guo et al.
    2017), and the Brier score, of f32 probabilities [n, J] on the device against int64 targets.  With the integers of
    kernels.calib_bins, ece = sum_b |right_b 2^32 - sum q_b| / (valid 2^32) and mce = max_b |right_b 2^32 - sum q_b| /
    (rows_b 2^32): one correctly rounded division each.  Rows with a NaN or an infinity are left out and counted in
    `nonfinite`; a target outside [0, J) raises ValueError.  One read-back after the last launch."""
    probs = probs.detach().float().contiguous()
    targets = targets.detach().reshape(-1).to(torch.int64).contiguous()
    table_d, stats_d, brier_d = K.calib_bins(probs, targets, bins)
    packed = torch.cat([table_d.reshape(-1), stats_d, brier_d.view(torch.int64)]).cpu().numpy()        # the one synchronisation
    M = int(bins)
    table = packed[: 3 * M].reshape(M, 3).copy()
    valid, nonfinite, oob, right = (int(v) for v in packed[3 * M: 3 * M + 4])
    brier_sum = float(packed[3 * M + 4:].view(np.float64)[0])
    if oob:
        raise ValueError(f"calibration: {oob} targets are outside [0, {probs.shape[1]})")
    count = table[:, 0].astype(np.int64)
    gaps = [abs(int(c) * Q_ONE - int(q)) for _, c, q in table.tolist()]
    with np.errstate(invalid="ignore", divide="ignore"):
        accuracy = np.where(count > 0, table[:, 1] / np.maximum(count, 1), np.nan)
        confidence = np.array([int(q) / (int(r) * Q_ONE) if r else float("nan") for r, _, q in table.tolist()], dtype=np.float64)
    if valid == 0:
        return CalibrationResult(None, None, None, None, 0, nonfinite, count, accuracy, confidence, table, brier_sum)
    ece = sum(gaps) / (valid * Q_ONE)
    mce = max(g / (int(r) * Q_ONE) for g, r in zip(gaps, count.tolist()) if r)
    return CalibrationResult(ece, mce, brier_sum / valid, right / valid, valid, nonfinite, count, accuracy, confidence, table, brier_sum)


@dataclass
class TemperatureFit:
    """What fit_temperature found: the temperature, the mean NLL of the valid rows at T = 1 and at `temperature`, whether the
    minimum lies at or beyond a bound (temperature is then that bound), and the bracketing rounds run."""

    temperature: float
    nll_before: float | None
    nll_after: float | None
    at_bound: bool
    rounds: int
    valid: int = 0
    nonfinite: int = 0


FIT_ROUND_BETAS = 32            # geometrically spaced betas per bracketing round
FIT_MAX_ROUNDS = 8
FIT_BRACKET_TOL = 1e-9          # stop at hi / lo - 1 <= this


def _geometric(lo: float, hi: float, count: int) -> list[float]:
    """`count` values from lo to hi inclusive with a constant ratio; the ends are lo and hi themselves."""
    ratio = hi / lo
    return [lo] + [lo * ratio ** (i / (count - 1)) for i in range(1, count - 1)] + [hi]


def fit_temperature(logits: torch.Tensor, targets: torch.Tensor, t_min: float = 0.05, t_max: float = 100.0) -> TemperatureFit:
    """The temperature T in [t_min, t_max] that minimises the NLL of softmax(logits / T) (f32 [n, J] on the device) against
    int64 targets.  The NLL is convex in beta = 1 / T, so its derivative g never decreases: the first launch looks at the two
    bounds and at beta = 1; a g >= 0 at 1 / t_max or <= 0 at 1 / t_min returns that bound (at_bound).  Otherwise rounds of
    FIT_ROUND_BETAS geometrically spaced betas shrink the bracket to the adjacent pair where g changes sign, until hi / lo - 1
    <= FIT_BRACKET_TOL or FIT_MAX_ROUNDS rounds, and one secant step inside the bracket gives beta.  One read-back per round
    and no host loop over samples.  A target outside [0, J) raises ValueError; no valid row raises ValueError."""
    if not (0.0 < t_min < 1.0 < t_max and np.isfinite(t_max)):
        raise ValueError(f"fit_temperature: need 0 < t_min < 1 < t_max, got {t_min!r}, {t_max!r}")
    logits = logits.detach().float().contiguous()
    targets = targets.detach().reshape(-1).to(torch.int64).contiguous()
    n = logits.shape[0]

    def evaluate(betas):
        sums_d, stats_d = K.calib_nll(logits, targets, betas)
        packed = torch.cat([sums_d.reshape(-1).view(torch.int64), stats_d]).cpu().numpy()             # the round's one synchronisation
        return packed[:-2].view(np.float64).reshape(-1, 3), int(packed[-2]), int(packed[-1])

    lo, hi = 1.0 / float(t_max), 1.0 / float(t_min)
    first, nonfinite, oob = evaluate([lo, 1.0, hi])
    if oob:
        raise ValueError(f"fit_temperature: {oob} targets are outside [0, {logits.shape[1]})")
    valid = n - nonfinite
    if valid <= 0:
        raise ValueError("fit_temperature: no row with finite logits")
    nll_before = float(first[1, 0]) / valid
    if first[0, 1] >= 0.0:
        return TemperatureFit(float(t_max), nll_before, float(first[0, 0]) / valid, True, 0, valid, nonfinite)
    if first[2, 1] <= 0.0:
        return TemperatureFit(float(t_min), nll_before, float(first[2, 0]) / valid, True, 0, valid, nonfinite)
    g_lo, g_hi = float(first[0, 1]), float(first[2, 1])
    rounds = 0
    while rounds < FIT_MAX_ROUNDS and hi / lo - 1.0 > FIT_BRACKET_TOL:
        betas = _geometric(lo, hi, FIT_ROUND_BETAS)
        g = evaluate(betas)[0][:, 1]
        rounds += 1
        i = next((i for i in range(1, FIT_ROUND_BETAS) if g[i] > 0.0), FIT_ROUND_BETAS - 1)      # g[0] < 0 < g[-1] by the bracket
        lo, hi, g_lo, g_hi = betas[i - 1], betas[i], float(g[i - 1]), float(g[i])
    beta = lo - g_lo * (hi - lo) / (g_hi - g_lo) if g_hi > g_lo else lo
    beta = min(max(beta, lo), hi)
    final = evaluate([beta])[0]
    return TemperatureFit(1.0 / beta, nll_before, float(final[0, 0]) / valid, False, rounds, valid, nonfinite)


def mean_nll(logits: torch.Tensor, targets: torch.Tensor, temperature: float = 1.0) -> float | None:
    """The mean negative log-likelihood of softmax(logits / temperature) over the rows with finite logits, summed in f64 on the
    device; None when there is none.  A target outside [0, J) raises ValueError.  One launch pair, one read-back."""
    sums_d, stats_d = K.calib_nll(logits.detach().float().contiguous(), targets.detach().reshape(-1).to(torch.int64).contiguous(),
                                  [1.0 / float(temperature)])
    packed = torch.cat([sums_d.reshape(-1).view(torch.int64), stats_d]).cpu().numpy()
    nonfinite, oob = int(packed[-2]), int(packed[-1])
    if oob:
        raise ValueError(f"mean_nll: {oob} targets are outside [0, {logits.shape[1]})")
    valid = logits.shape[0] - nonfinite
    return float(packed[:1].view(np.float64)[0]) / valid if valid > 0 else None


def apply_temperature(logits: torch.Tensor, temperature: float) -> tuple[torch.Tensor, torch.Tensor]:
    """(softmax(logits / temperature), its arg max) of f32 logits [n, J] on the device; at temperature 1 the bits of
    kernels.softmax_argmax."""
    return K.softmax_argmax_t(logits.detach().float().contiguous(), 1.0 / float(temperature))


def _members(op: str, tensors, dtype: torch.dtype) -> list[torch.Tensor]:
    members = [t.detach().to(dtype).contiguous() for t in tensors]
    if not members:
        raise ValueError(f"{op}: no members")
    return members


def fuse(logits_list, coef=None, mode: str = "logit", temperatures=None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(probabilities f32 [n, J], their first arg max int64 [n], fused logits f32 [n, J]) of K models' f32 logits [n, J] on the
    device.  mode "logit": softmax(sum_k coef_k z_k / T_k), the log-linear pool; "prob": sum_k coef_k softmax(z_k / T_k), the
    linear pool, whose logits are log p; coef_k >= 0 summing to 1 there.  coef: equal weights 1 / K by default.  temperatures: one
    per member (None entries and None itself: 1).  A row with a non-finite logit in any member holds NaN and predicts 0."""
    if mode not in ("logit", "prob"):
        raise ValueError(f"fuse: mode must be logit or prob, got {mode!r}")
    members = _members("fuse", logits_list, torch.float32)
    count = len(members)
    coef = [1.0 / count] * count if coef is None else [float(c) for c in coef]
    betas = [1.0 if t is None else 1.0 / float(t) for t in (temperatures if temperatures is not None else [None] * count)]
    if len(coef) != count or len(betas) != count:
        raise ValueError(f"fuse: {count} members, {len(coef)} coefficients and {len(betas)} temperatures")
    if mode == "logit":
        probs, preds, fused, _ = K.fuse_scores(members, [c * b for c, b in zip(coef, betas)], K.FUSE_LOGIT)
    else:
        probs, preds, fused, _ = K.fuse_scores(members, coef, K.FUSE_PROB, betas)
    return probs, preds, fused


@dataclass
class FusionFit:
    """What fit_fusion found: the coefficients of the log-linear pool, the mean NLL of the valid rows at `start` and at `coef`,
    the Newton iterations run, whether an iterate left the box of coef_max (the data are separable: coef is then the last iterate
    and no minimum), whether the gradient met the stopping rule, and the valid and non-finite rows."""

    coef: list[float]
    nll_before: float
    nll_after: float
    iterations: int
    at_bound: bool
    converged: bool
    valid: int = 0
    nonfinite: int = 0


FUSION_STEPS = 8                # step lengths 1, 1/2, ..., 2^-7 per launch (kernels.FUSE_MAX_CANDS)
FUSION_MAX_ITERATIONS = 30
FUSION_GRADIENT_TOL = 1e-10     # stop at max |g| / valid <= this
FUSION_ARMIJO = 1e-4


def unpack_fusion_terms(row: np.ndarray, K: int) -> tuple[float, np.ndarray, np.ndarray]:
    """One candidate's kernels.fuse_terms(K) doubles -> (nll, g [K], the symmetric H [K, K])."""
    g = np.array(row[1:1 + K], dtype=np.float64)
    H = np.zeros((K, K), dtype=np.float64)
    H[np.triu_indices(K)] = row[1 + K:]
    return float(row[0]), g, H + np.triu(H, 1).T


def newton_fusion(evaluate, start, l2: float, coef_max: float):
    """The damped Newton method of fit_fusion on `evaluate(candidates) -> ([(nll, g, H), ...], valid)`, sums over the valid rows:
    (coef, the summed nll at start, the summed nll at coef, iterations, at_bound, converged, valid).  The ridge l2 valid / 2
    |a - start|^2 joins nll, g and H here.  Kept apart from the device so that a host reference can run the same steps."""
    start = np.asarray(start, dtype=np.float64)
    a = start.copy()
    (first,), valid = evaluate([a.tolist()])
    ridge = float(l2) * valid

    def with_ridge(a, nll, g, H):
        d = a - start
        return nll + 0.5 * ridge * float(d @ d), g + ridge * d, H + ridge * np.eye(len(start))

    nll, g, H = first
    nll_before = nll
    F, g, H = with_ridge(a, nll, g, H)
    iterations, at_bound, converged = 0, False, False
    while True:
        if float(np.max(np.abs(g))) / valid <= FUSION_GRADIENT_TOL:
            converged = True
            break
        if iterations >= FUSION_MAX_ITERATIONS:
            break
        try:
            d = -np.linalg.solve(H, g)
        except np.linalg.LinAlgError:
            d = -g / max(float(np.max(np.abs(np.diag(H)))), 1.0)       # a singular Hessian (identical members): steepest descent
        slope = float(g @ d)
        if not np.isfinite(d).all() or slope >= 0.0:
            d = -g / max(float(np.max(np.abs(np.diag(H)))), 1.0)
            slope = float(g @ d)
        steps = [2.0 ** -i for i in range(FUSION_STEPS)]
        cands = [a + t * d for t in steps]
        results, _ = evaluate([c.tolist() for c in cands])
        iterations += 1
        taken = None
        for t, c, (c_nll, c_g, c_H) in zip(steps, cands, results):
            c_F, c_g, c_H = with_ridge(c, c_nll, c_g, c_H)
            if c_F <= F + FUSION_ARMIJO * t * slope:
                taken = (c, c_nll, c_F, c_g, c_H)
                break
        if taken is None:                                               # no step length lowers the objective: the rounding floor
            break
        a, nll, F, g, H = taken
        if float(np.max(np.abs(a))) > coef_max:
            at_bound = True
            break
    return a.tolist(), nll_before, nll, iterations, at_bound, converged, valid


def fit_fusion(logits_list, targets: torch.Tensor, start=None, l2: float = 0.0, coef_max: float = 32.0) -> FusionFit:
    """The coefficients a of the log-linear pool softmax(sum_k a_k z_k) that minimise its NLL (plus l2 valid / 2 |a - start|^2) on K
    models' f32 logits [n, J] on the device against int64 targets: a damped Newton method on a convex function.  Every launch
    evaluates the candidates a + t d for t = 1, 1/2, ..., 2^-7 with their gradients and Hessians (kernels.fuse_nll); the first t
    that satisfies the Armijo condition (c = 1e-4) is taken, and its g and H give the next direction: one launch pair and one
    read-back per iteration.  Stops at max |g| / valid <= 1e-10 (converged) or after 30 iterations; an iterate whose largest
    |a_k| exceeds coef_max stops the fit with at_bound (separable data have no minimum).  start: 1 / K each by default.  A target
    outside [0, J) raises ValueError; no valid row raises ValueError."""
    members = _members("fit_fusion", logits_list, torch.float32)
    targets = targets.detach().reshape(-1).to(torch.int64).contiguous()
    count = len(members)
    n, J = members[0].shape
    start = [1.0 / count] * count if start is None else [float(v) for v in start]
    if len(start) != count or not (float(l2) >= 0.0 and coef_max > 0.0):
        raise ValueError(f"fit_fusion: {count} members need {count} starting coefficients, l2 >= 0 and coef_max > 0")
    seen = {}

    def evaluate(cands):
        sums_d, stats_d = K.fuse_nll(members, targets, cands)
        packed = torch.cat([sums_d.reshape(-1).view(torch.int64), stats_d]).cpu().numpy()             # the iteration's one synchronisation
        nonfinite, oob = int(packed[-2]), int(packed[-1])
        if oob:
            raise ValueError(f"fit_fusion: {oob} targets are outside [0, {J})")
        if n - nonfinite <= 0:
            raise ValueError("fit_fusion: no row with finite logits")
        seen["nonfinite"] = nonfinite
        table = packed[:-2].view(np.float64).reshape(len(cands), -1)
        return [unpack_fusion_terms(row, count) for row in table], n - nonfinite

    coef, before, after, iterations, at_bound, converged, valid = newton_fusion(evaluate, start, l2, coef_max)
    return FusionFit(coef, before / valid, after / valid, iterations, at_bound, converged, valid, seen["nonfinite"])


@dataclass
class DiversityResult:
    """What diversity found, from the integer tables alone; every figure is one division of Python integers, None where its
    denominator is 0.  The [K][K] lists are indexed by (member a, member b); pair holds the counts (both right, a right b wrong,
    a wrong b right, both wrong), hist the rows by the number of members that are right."""

    accuracy: list
    disagreement: list
    double_fault: list
    yule_q: list
    kappa: list
    oracle_accuracy: float | None
    majority_accuracy: float | None
    hist: list
    pair: list
    valid: int


def _ratio(num: int, den: int) -> float | None:
    return num / den if den else None


def diversity_from_counts(pair: list, hist: list, valid: int) -> DiversityResult:
    """DiversityResult of the Python-integer tables pair [K][K][4] and hist [K + 1] over `valid` rows."""
    K = len(hist) - 1
    accuracy = [_ratio(pair[k][k][0], valid) for k in range(K)]
    disagreement, double_fault, yule_q, kappa = ([[None] * K for _ in range(K)] for _ in range(4))
    for a in range(K):
        for b in range(K):
            n11, n10, n01, n00 = pair[a][b]
            disagreement[a][b] = _ratio(n10 + n01, valid)
            double_fault[a][b] = _ratio(n00, valid)
            yule_q[a][b] = _ratio(n11 * n00 - n10 * n01, n11 * n00 + n10 * n01)
            chance = (n11 + n10) * (n11 + n01) + (n01 + n00) * (n10 + n00)       # valid^2 times the agreement expected by chance
            kappa[a][b] = _ratio(valid * (n11 + n00) - chance, valid * valid - chance)
    return DiversityResult(accuracy, disagreement, double_fault, yule_q, kappa, _ratio(valid - hist[0], valid),
                           _ratio(sum(h for c, h in enumerate(hist) if 2 * c > K), valid), list(hist), pair, valid)


def diversity(preds_list, targets: torch.Tensor, num_classes: int) -> DiversityResult:
    """How K models' int64 predictions [n] on the device coincide on being right: per-member accuracy, and per pair the
    disagreement rate, the double-fault rate, Yule's Q and Cohen's kappa of right / wrong (Kuncheva & Whitaker 2003), plus the
    accuracy of an oracle (any member right) and of a majority (more than K / 2 right).  kernels.fuse_agree counts; one
    read-back.  A target outside [0, num_classes) raises ValueError."""
    members = _members("diversity", preds_list, torch.int64)
    targets = targets.detach().reshape(-1).to(torch.int64).contiguous()
    count = len(members)
    pair_d, hist_d, stats_d = K.fuse_agree(members, targets, num_classes)
    packed = [int(v) for v in torch.cat([pair_d.reshape(-1), hist_d, stats_d]).tolist()]       # the one synchronisation
    valid, oob = packed[-2], packed[-1]
    if oob:
        raise ValueError(f"diversity: {oob} targets are outside [0, {num_classes})")
    pair = [[packed[(a * count + b) * 4:(a * count + b) * 4 + 4] for b in range(count)] for a in range(count)]
    return diversity_from_counts(pair, packed[4 * count * count:4 * count * count + count + 1], valid)


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
