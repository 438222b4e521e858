"""Reference of the bootstrap (csrc/dfd_boot.hip, deepfakedetection_amd.metrics.bootstrap) in numpy and Python integers.

The draws restate the resampling rule of include/dfd_hip.h: Philox4x32-10 in uint64 arithmetic, vectorised over the draws.  The
statistics of a resample come from EXPANDING it — np.repeat(scores, counts) with its labels and hits — and calling the functions
of tests/_metrics_ref.py on the expansion, so they do not share the weighted formulation the kernel uses; `weighted_stats`
restates that formulation too, for the CPU test that holds the two against each other."""

from __future__ import annotations

import numpy as np

from tests import _metrics_ref as R

BOOT_STREAM = 0x626F6F74
MASK = np.uint64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
METRICS = ("auc", "eer", "accuracy", "balanced_accuracy", "tpr", "fpr", "hit_rate")


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two ints -> the four output words as uint64 arrays below 2^32."""
    c = [np.atleast_1d(np.asarray(w, dtype=np.uint64)) & MASK for w in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c[0], PHILOX_M1 * c[2]                      # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + PHILOX_W0) & 0xFFFFFFFF, (k1 + PHILOX_W1) & 0xFFFFFFFF
    return c


def draws(n: int, b: int, seed: int) -> np.ndarray:
    """The n sample indices resample b draws under `seed`, in draw order."""
    blocks = np.arange((n + 3) // 4, dtype=np.uint64)
    words = philox4x32_10((blocks, b, 0, BOOT_STREAM), (seed & 0xFFFFFFFF, seed >> 32))
    u = np.stack(words, axis=1).reshape(-1)[:n]                         # draw t = word t & 3 of block t >> 2
    return ((u * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def counts(n: int, b0: int, R_: int, seed: int) -> np.ndarray:
    """int64 [R, n]: how often each sample is drawn in resamples b0 .. b0 + R - 1."""
    return np.stack([np.bincount(draws(n, b, seed), minlength=n) for b in range(b0, b0 + R_)]).astype(np.int64).reshape(R_, n)


def eer_segment(fps, tps, P: int, N: int) -> list[int]:
    """[f0, t0, f1, t1]: the two ends of the segment on which metrics.eer_from_curve interpolates; zeros when a class is absent."""
    if P == 0 or N == 0:
        return [0, 0, 0, 0]
    a = [int(f) * P + int(t) * N - P * N for f, t in zip(fps.tolist(), tps.tolist())]
    i = next(k for k, v in enumerate(a) if v >= 0)
    return [int(fps[i - 1]) if i else 0, int(tps[i - 1]) if i else 0, int(fps[i]), int(tps[i])]


def resample_stats(scores, is_positive, c, cut=None, hit=None) -> list[int]:
    """The ten statistics of one member in the resample with multiplicities c, by expansion."""
    scores, labels = np.asarray(scores, dtype=np.float32), (np.asarray(is_positive) != 0).astype(np.int64)
    c = np.asarray(c, dtype=np.int64)
    s, l = np.repeat(scores, c), np.repeat(labels, c)
    P, N, _, _, two_u = R.groups(s, l)[3]
    tp, fp = (int(v[0]) for v in R.sweep(s, l, [cut])) if cut is not None else (0, 0)
    hits = int(np.repeat((np.asarray(hit) != 0).astype(np.int64), c).sum()) if hit is not None else 0
    fps, tps, _ = R.roc_counts(s, l)
    return [P, N, two_u, tp, fp, hits] + eer_segment(fps, tps, P, N)


def stats(members, is_positive, B: int, seed: int, cuts=None, hit=None) -> np.ndarray:
    """int64 [M, B, 10]: dfd_boot_stats' output for the members' UNSORTED scores in sample order."""
    n = len(is_positive)
    cuts = [None] * len(members) if cuts is None else list(cuts)
    out = np.zeros((len(members), B, 10), dtype=np.int64)
    for b in range(B):
        c = np.bincount(draws(n, b, seed), minlength=n)
        for m, (scores, cut) in enumerate(zip(members, cuts)):
            out[m, b] = resample_stats(scores, is_positive, c, cut, hit)
    return out


def weighted_stats(scores, is_positive, c, cut=None, hit=None) -> list[int]:
    """The same ten numbers the way the kernel forms them: one sweep of the ascending order with the multiplicities as weights,
    empty tie groups left in."""
    scores = np.asarray(scores, dtype=np.float32)
    order = np.argsort(scores, kind="stable")
    s, pos, w = scores[order], np.asarray(is_positive)[order] != 0, np.asarray(c, dtype=np.int64)[order]
    P, N = int(w[pos].sum()), int(w[~pos].sum())
    two_u, p, nn, bp, bn, seg = 0, 0, 0, 0, 0, [0, 0, 0, 0]
    for i in range(s.size):
        if pos[i]:
            p += int(w[i])
        else:
            nn += int(w[i])
        if i == s.size - 1 or s[i] != s[i + 1]:
            two_u += (p - bp) * (bn + nn)
            if bn * P + bp * N <= P * N < nn * P + p * N:
                seg = [N - nn, P - p, N - bn, P - bp]
            bp, bn = p, nn
    at = s.astype(np.float64) >= cut if cut is not None else np.zeros(s.size, dtype=bool)
    hits = int((np.asarray(c, dtype=np.int64) * (np.asarray(hit) != 0)).sum()) if hit is not None else 0
    return [P, N, two_u, int(w[at & pos].sum()), int(w[at & ~pos].sum()), hits] + seg


def value(row, metric: str) -> float:
    """One metric of one resample's ten integers, in Python integers; NaN where it does not exist."""
    P, N, two_u, tp, fp, hits, f0, t0, f1, t1 = (int(v) for v in row)
    if metric == "hit_rate":
        return hits / (P + N) if P + N else float("nan")
    if P == 0 or N == 0:
        return float("nan")
    if metric == "auc":
        return two_u / (2 * P * N)
    if metric == "accuracy":
        return (tp + N - fp) / (P + N)
    if metric == "balanced_accuracy":
        return (tp * N + (N - fp) * P) / (2 * P * N)
    if metric == "tpr":
        return tp / P
    if metric == "fpr":
        return fp / N
    if metric == "eer":
        a0, a1 = f0 * P + t0 * N - P * N, f1 * P + t1 * N - P * N
        if a1 == 0:
            return f1 / N
        t = -a0 / (a1 - a0)
        return (f0 + t * (f1 - f0)) / N
    raise ValueError(metric)


def values(table, metric: str) -> np.ndarray:
    table = np.asarray(table)
    flat = [value(row, metric) for row in table.reshape(-1, 10).tolist()]
    return np.array(flat, dtype=np.float64).reshape(table.shape[:-1])


def interval(v, level: float):
    v = np.asarray(v, dtype=np.float64)
    v = v[~np.isnan(v)]
    if v.size == 0:
        return None
    lo, hi = np.quantile(v, [(1 - level) / 2, (1 + level) / 2])
    return float(lo), float(hi)


def delta(va, vb, level: float):
    """(lo, hi, p, valid) of the paired differences."""
    d = [a - b for a, b in zip(np.asarray(va).tolist(), np.asarray(vb).tolist()) if a == a and b == b]
    lo_hi = interval(d, level) if d else None
    below, above = sum(1 for x in d if x <= 0), sum(1 for x in d if x >= 0)
    p = min(1.0, 2 * min(below + 1, above + 1) / (len(d) + 1))
    return (lo_hi[0] if lo_hi else None, lo_hi[1] if lo_hi else None, p, len(d))
