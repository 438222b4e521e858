"""Reference of group pooling (csrc/dfd_group.hip) and of the cluster bootstrap (dfd_boot_stats_grouped) in numpy and Python integers.

Pooling is a plain Python loop over the groups: the fixed point q = rint(p 2^32) in f64, Python-int sums, one f64 division and the
f32 cast.  The cluster bootstrap draws G groups with tests/_boot_ref.draws, turns the group counts into per-sample counts and hands
them to tests/_boot_ref.weighted_stats (whose equality with the literal expansion tests/test_group_cpu.py checks)."""

from __future__ import annotations

import numpy as np

from tests import _boot_ref as B

Q_ONE = 1 << 32
MODES = {"mean": 0, "vote": 1, "max": 2}


def pool(probs, group, targets, G: int, mode: str = "mean", positive: int = 1):
    """(probs f32 [G, J], preds int64 [G], targets int64 [G], sizes int32 [G], info [4]) as include/dfd_hip.h states them."""
    probs = np.asarray(probs, dtype=np.float32)
    group, targets = np.asarray(group, dtype=np.int64), np.asarray(targets, dtype=np.int64)
    n, J = probs.shape
    members: list[list[int]] = [[] for _ in range(G)]
    with np.errstate(invalid="ignore"):
        valid = np.all((probs >= 0) & (probs <= 1), axis=1) & (targets >= 0) & (targets < J)       # a NaN compares false
    inside = (group >= 0) & (group < G)
    info = [int((~valid).sum()), int((valid & ~inside).sum()), 0, 0]
    for i in np.flatnonzero(valid & inside).tolist():
        members[int(group[i])].append(i)
    out = np.zeros((G, J), dtype=np.float32)
    preds, tgt, sizes = np.zeros(G, dtype=np.int64), np.full(G, -1, dtype=np.int64), np.zeros(G, dtype=np.int32)
    for g, rows in enumerate(members):
        if not rows:
            info[3] += 1
            continue
        sizes[g] = len(rows)
        seen = {int(targets[i]) for i in rows}
        tgt[g] = min(seen)
        info[2] += len(seen) > 1
        if mode == "max":
            best = rows[0]
            for i in rows[1:]:                                          # ascending i: a tie keeps the lowest index
                if probs[i, positive] > probs[best, positive]:
                    best = i
            out[g] = probs[best]
        else:
            if mode == "mean":
                q = np.rint(probs[rows].astype(np.float64) * 4294967296.0).astype(np.int64)
                sums = [sum(q[:, j].tolist()) for j in range(J)]       # Python integers
            else:
                votes = np.argmax(probs[rows], axis=1).tolist()         # the first arg max of every member row
                sums = [votes.count(j) * Q_ONE for j in range(J)]
            for j in range(J):
                out[g, j] = np.float32(np.float64(float(sums[j])) / (np.float64(len(rows)) * 4294967296.0))
        preds[g] = int(np.argmax(out[g]))                               # the first arg max of the stored f32 row
    return out, preds, tgt, sizes, info


def sample_counts(group, G: int, b: int, seed: int) -> np.ndarray:
    """int64 [n]: how often each sample counts in cluster resample b: the count of its group, 0 for an id outside [0, G)."""
    group = np.asarray(group, dtype=np.int64)
    per_group = np.bincount(B.draws(G, b, seed), minlength=G).astype(np.int64)
    ok = (group >= 0) & (group < G)
    return np.where(ok, per_group[np.clip(group, 0, G - 1)], 0)


def cluster_stats(members, is_positive, group, G: int, replicates: int, seed: int, cuts=None, hit=None) -> np.ndarray:
    """int64 [M, B, 10]: dfd_boot_stats_grouped's output for the members' UNSORTED scores in sample order."""
    cuts = [None] * len(members) if cuts is None else list(cuts)
    out = np.zeros((len(members), replicates, 10), dtype=np.int64)
    for b in range(replicates):
        c = sample_counts(group, G, b, seed)
        for m, (scores, cut) in enumerate(zip(members, cuts)):
            out[m, b] = B.weighted_stats(scores, is_positive, c, cut, hit)
    return out
