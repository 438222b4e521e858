"""Host reference of the ensemble kernels (csrc/dfd_fuse.hip) and of metrics.fuse / fit_fusion / diversity: the same definitions in
numpy float64 and Python integers, sums with math.fsum.  Shared by tests/test_fuse_cpu.py, tests/test_fuse_gpu.py and
scripts/bench_fuse.py.

Row rules (include/dfd_hip.h): a row that holds a NaN or an infinity in any member is `nonfinite` and left out; a finite row whose
target is outside [0, J) is `oob` and left out; the rest are valid.
"""

from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from tests._calib_ref import U, sum_bound  # noqa: F401  (sum_bound is the one bound formula of both references)

LOGIT, PROB = 0, 1
STEPS, MAX_ITERATIONS, GRADIENT_TOL, ARMIJO = 8, 30, 1e-10, 1e-4


def terms(K: int) -> int:
    return 1 + K + K * (K + 1) // 2


def stack(zs) -> np.ndarray:
    """The members' f32 [n, J] logits as one float64 [K, n, J] array (every f32 is an f64)."""
    return np.stack([np.asarray(z, dtype=np.float32) for z in zs]).astype(np.float64)


def split_rows(zs, targets):
    """(valid mask, nonfinite count, oob count) of K members' rows and int64 targets."""
    z = stack(zs)
    targets = np.asarray(targets, dtype=np.int64)
    finite = np.isfinite(z).all(axis=(0, 2))
    inside = (targets >= 0) & (targets < z.shape[2])
    return finite & inside, int((~finite).sum()), int((finite & ~inside).sum())


def pool(z: np.ndarray, a, reverse: bool = False) -> np.ndarray:
    """sum_k a_k z_k as the kernel adds it: from 0.0, k ascending (reverse: descending, the other order of the two-orderings check)."""
    f = np.zeros(z.shape[1:], dtype=np.float64)
    for k in (range(len(a) - 1, -1, -1) if reverse else range(len(a))):
        f = f + float(a[k]) * z[k]
    return f


def _row_sum(e: np.ndarray, reverse: bool) -> np.ndarray:
    s = np.zeros(e.shape[0], dtype=np.float64)
    for j in (range(e.shape[1] - 1, -1, -1) if reverse else range(e.shape[1])):
        s = s + e[:, j]
    return s


def scores(zs, coef, mode: int = LOGIT, beta=None, reverse: bool = False):
    """(probs f32 [n, J], preds int64 [n], fused logits f32 [n, J], nonfinite rows): float64 throughout, one rounding to f32, the
    first arg max of the rounded probabilities; a non-finite row holds NaN and predicts 0.  reverse: every sum in the opposite
    order."""
    z = stack(zs)
    K, n, J = z.shape
    finite = np.isfinite(z).all(axis=(0, 2))
    zf = z[:, finite]
    if mode == LOGIT:
        f = pool(zf, coef, reverse)
        e = np.exp(f - f.max(axis=1, keepdims=True)) if f.size else f
        p = e / _row_sum(e, reverse)[:, None]
    else:
        p = np.zeros(zf.shape[1:], dtype=np.float64)
        for k in (range(K - 1, -1, -1) if reverse else range(K)):
            b = float(beta[k]) * zf[k]
            e = np.exp(b - b.max(axis=1, keepdims=True)) if b.size else b
            p = p + float(coef[k]) * (e / _row_sum(e, reverse)[:, None])
        with np.errstate(divide="ignore"):
            f = np.log(p)
    probs = np.full((n, J), np.nan, dtype=np.float32)
    fused = np.full((n, J), np.nan, dtype=np.float32)
    preds = np.zeros(n, dtype=np.int64)
    probs[finite], fused[finite] = p.astype(np.float32), f.astype(np.float32)
    preds[finite] = probs[finite].argmax(axis=1) if p.size else 0
    return probs, preds, fused, int((~finite).sum())


@dataclass
class NllRef:
    out: np.ndarray         # [C, terms(K)] fsum of the rows' terms, packed {nll, g[0..K), H[0][0..K), H[1][1..K), ...}
    mag: np.ndarray         # [C, terms(K)] summed magnitude of what each row's term is made of (nll: |m| + |log s| + |f_y| + 1;
    #                         g_k: sum_j p_j |z_kj| + |z_ky|; H_kl: sum_j p_j |z_kj z_kl| + |E z_k| |E z_l|)
    amax: np.ndarray        # [C] max over the valid rows and j of sum_k |a_k z_kj|
    stats: list             # [nonfinite, oob]
    valid: int


def nll(zs, targets, cands) -> NllRef:
    targets = np.asarray(targets, dtype=np.int64)
    valid, nonfinite, oob = split_rows(zs, targets)
    z, y = stack(zs)[:, valid], targets[valid]
    K, n, _ = z.shape
    C, T = len(cands), terms(K)
    out, mag, amax = np.zeros((C, T)), np.zeros((C, T)), np.zeros(C)
    if n:
        rows = np.arange(n)
        zy = z[:, rows, y]                                                      # [K, n]
        for c, a in enumerate(cands):
            f = pool(z, a)
            m = f.max(axis=1)
            e = np.exp(f - m[:, None])
            s = e.sum(axis=1)
            p = e / s[:, None]
            fy = f[rows, y]
            mean = (p[None] * z).sum(axis=2)                                    # [K, n]
            out[c, 0] = math.fsum((m + np.log(s) - fy).tolist())
            mag[c, 0] = math.fsum((np.abs(m) + np.abs(np.log(s)) + np.abs(fy) + 1.0).tolist())
            o = 1 + K
            for k in range(K):
                out[c, 1 + k] = math.fsum((mean[k] - zy[k]).tolist())
                mag[c, 1 + k] = math.fsum(((p * np.abs(z[k])).sum(axis=1) + np.abs(zy[k])).tolist())
                for l in range(k, K):
                    second = (p * (z[k] * z[l])).sum(axis=1)
                    out[c, o] = math.fsum((second - mean[k] * mean[l]).tolist())
                    mag[c, o] = math.fsum(((p * np.abs(z[k] * z[l])).sum(axis=1) + np.abs(mean[k]) * np.abs(mean[l])).tolist())
                    o += 1
            amax[c] = float(sum(abs(float(a[k])) * np.abs(z[k]) for k in range(K)).max())
    return NllRef(out, mag, amax, [nonfinite, oob], int(n))


def fuse_per_row(J: int, K: int, amax: float) -> float:
    """The per-row factor of sum_bound for nll, g and H, derived as _calib_ref.nll_per_row is, with A = max sum_k |a_k z_kj| (which
    bounds max |sum_k a_k z_kj| and is what the K roundings of the pooled logit scale with).  f_j = sum_k a_k z_kj takes K products
    and K - 1 additions: an absolute error of at most K u A; so does m, and their difference (up to 2 A) is rounded once more: the
    exponent f_j - m carries at most (2 K + 2) u A =: c u A, which exp turns into a relative error of each e_j; exp and log are
    good to 1 ulp; a sum of J positive terms adds (J - 1) u.  So s and every p_j are good to (2 c A + J + 4) u, the weighted means
    sum_j p_j z_kj to (2 c A + 2 J + 6) u of sum_j p_j |z_kj|, the second moments (one product more) to (2 c A + 2 J + 7) u of
    sum_j p_j |z_kj z_kl|, the product of two means to twice the first plus a rounding, and H_kl, their difference, to
    (4 c A + 4 J + 15) u of its magnitude.  g_k = mean - z_ky is within (2 c A + 2 J + 7) u.  nll = m + log s - f_y is within
    u (2 (|m| + |f_y| + |log s|) + (2 K + 2 c) A + J + 5), which the `+ 1` per row in its magnitude covers under the same factor.
    One factor for all three: 4 c A + 4 J + 16 = (8 K + 8) A + 4 J + 16; at K = 1, a = beta this is _calib_ref's 12 A + 4 J + 16
    with one rounding more counted for the product inside the pool."""
    return (8.0 * K + 8.0) * amax + 4.0 * J + 16.0


def unpack(row: np.ndarray, K: int):
    """One candidate's packed terms -> (nll, g [K], the symmetric H [K, K])."""
    H = np.zeros((K, K))
    H[np.triu_indices(K)] = row[1 + K:]
    return float(row[0]), np.array(row[1:1 + K]), H + np.triu(H, 1).T


@dataclass
class FitRef:
    coef: list
    nll_before: float       # means over the valid rows
    nll_after: float
    nll_after_sum: float    # the summed NLL at coef, with its magnitude and the A of sum_bound / fuse_per_row
    nll_after_mag: float
    amax: float
    iterations: int
    at_bound: bool
    converged: bool
    valid: int


def fit(zs, targets, start=None, l2: float = 0.0, coef_max: float = 32.0) -> FitRef:
    """metrics.fit_fusion step for step, on nll() above: damped Newton, the candidates a + t d for t = 1 .. 2^-7 per round, the first
    that satisfies Armijo (c = 1e-4) taken with the g and H of that evaluation."""
    K = len(zs)
    start = np.full(K, 1.0 / K) if start is None else np.asarray(start, dtype=np.float64)
    first = nll(zs, targets, [start])
    valid = first.valid
    ridge = l2 * valid

    def objective(a, row):
        value, g, H = unpack(row, K)
        d = a - start
        return value, value + 0.5 * ridge * float(d @ d), g + ridge * d, H + ridge * np.eye(K)

    a = start.copy()
    value, F, g, H = objective(a, first.out[0])
    before, iterations, at_bound, converged = value, 0, False, False
    while True:
        if np.abs(g).max() / valid <= GRADIENT_TOL:
            converged = True
            break
        if iterations >= MAX_ITERATIONS:
            break
        try:
            d = -np.linalg.solve(H, g)
        except np.linalg.LinAlgError:
            d = -g / max(np.abs(np.diag(H)).max(), 1.0)
        if not np.isfinite(d).all() or g @ d >= 0.0:
            d = -g / max(np.abs(np.diag(H)).max(), 1.0)
        slope = float(g @ d)
        cands = [a + 2.0 ** -i * d for i in range(STEPS)]
        res = nll(zs, targets, cands)
        iterations += 1
        for i, cand in enumerate(cands):
            c_value, c_F, c_g, c_H = objective(cand, res.out[i])
            if c_F <= F + ARMIJO * 2.0 ** -i * slope:
                break
        else:
            break
        a, value, F, g, H = cand, c_value, c_F, c_g, c_H
        if np.abs(a).max() > coef_max:
            at_bound = True
            break
    last = nll(zs, targets, [a])
    return FitRef(a.tolist(), before / valid, value / valid, float(last.out[0, 0]), float(last.mag[0, 0]), float(last.amax[0]), iterations,
                  at_bound, converged, valid)


def agree(preds, targets, J: int):
    """(pair [K][K][4], hist [K + 1], [valid, oob]) in Python integers."""
    targets = np.asarray(targets, dtype=np.int64)
    inside = (targets >= 0) & (targets < J)
    right = [(np.asarray(p, dtype=np.int64) == targets)[inside] for p in preds]
    K = len(right)
    pair = [[[int((ra & rb).sum()), int((ra & ~rb).sum()), int((~ra & rb).sum()), int((~ra & ~rb).sum())] for rb in right] for ra in right]
    votes = sum(r.astype(np.int64) for r in right)
    return pair, [int((votes == c).sum()) for c in range(K + 1)], [int(inside.sum()), int((~inside).sum())]


def members_case(seed: int, n: int, J: int, K: int, scale: float = 3.0, skill: float = 1.0):
    """K members' f32 logits [n, J] and int64 targets that are not separable: every member sees the label through its own noise."""
    rng = np.random.default_rng(seed)
    y = rng.integers(0, J, size=n).astype(np.int64)
    signal = np.eye(J)[y] * skill
    zs = [((signal + rng.standard_normal((n, J))) * scale).astype(np.float32) for _ in range(K)]
    return zs, y


def separable_case(n: int, J: int = 2, K: int = 8, margin: float = 0.1):
    """Noisy members beside one that is always right by a small margin: the NLL of the pool has no minimum, it falls for ever as
    that member's coefficient grows, and a gradient of 1e-10 per row needs a coefficient of about 23 / margin."""
    zs, y = members_case(1234, n, J, K)
    zs[0] = (np.eye(J)[y] * margin).astype(np.float32)
    return zs, y


def capped_coef(zs, seed: int, cap: float = 30.0):
    """Random coefficients of both signs, shrunk by a power of two until max sum_k |a_k z_kj| <= cap: every probability then stays
    a normal f32 (exp(-60) = 9e-27)."""
    rng = np.random.default_rng(seed)
    K = len(zs)
    a = rng.uniform(-0.5, 1.5, size=K)
    spread = sum(abs(a[k]) * np.abs(np.asarray(zs[k], dtype=np.float64)) for k in range(K)).max() if zs[0].size else 0.0
    while spread > cap:
        a, spread = a / 2.0, spread / 2.0
    return a.tolist()


# (members, classes) of the GPU tests: the issue's list, then the pairs on both sides of the thread / wave boundary K J = 16
SHAPES = [(1, 2), (2, 2), (3, 3), (8, 2), (8, 17), (2, 16), (2, 17), (2, 65), (2, 1000), (2, 1024), (4, 4), (1, 16), (1, 17), (2, 8), (2, 9),
          (8, 3)]


def sizes(rows: int, width: int) -> list:
    """1, the wave width and its neighbours, the rows of one workgroup and its neighbours, two workgroups + 1, and the smallest n
    whose stage-2 loop takes a second trip."""
    return sorted({1, 63, 64, 65, rows - 1, rows, rows + 1, 2 * rows + 1, width * rows + 1})


def score_case(K: int, J: int, n: int):
    """The inputs of the scores tests at (K, J): logits and coefficients with max sum_k |a_k z_kj| <= 30."""
    zs, _ = members_case(100 * K + J, n, J, K)
    return zs, capped_coef(zs, K + J)


def ramp_weights(K: int) -> list:
    """Weights 1 : 2 : ... : K of the linear pool; they sum to 1 within a rounding or two."""
    return (np.arange(1, K + 1) / (K * (K + 1) / 2)).tolist()


def ramp_betas(K: int) -> list:
    return [0.5 + 0.25 * k for k in range(K)]


def ulp_mismatches(got: np.ndarray, want: np.ndarray):
    """(elements whose f32 bit patterns differ, the largest difference in units of the last place) of two arrays of positive normals."""
    d = np.abs(np.ascontiguousarray(got).view(np.int32).astype(np.int64) - np.ascontiguousarray(want).view(np.int32).astype(np.int64))
    return int((d != 0).sum()), int(d.max()) if d.size else 0
