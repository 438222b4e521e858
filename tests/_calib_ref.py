"""Host reference of the calibration kernels (csrc/dfd_calib.hip) and of metrics.calibration / metrics.fit_temperature: the same
definitions in numpy float64 and Python integers, sums with math.fsum.  Shared by tests/test_calib_cpu.py, tests/test_calib_gpu.py
and scripts/bench_calib.py.

Row rules (include/dfd_hip.h): a row that holds a NaN or an infinity is `nonfinite` and left out; a finite row whose target is
outside [0, J) is `oob` and left out; the rest are valid.
"""

from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

Q_ONE = 1 << 32
U = 2.0 ** -53                          # unit roundoff of float64
ROUND_BETAS, MAX_ROUNDS, BRACKET_TOL = 32, 8, 1e-9


def split_rows(rows: np.ndarray, targets: np.ndarray):
    """(valid mask, nonfinite count, oob count) of f32 [n, J] rows and int64 targets."""
    rows = np.asarray(rows, dtype=np.float32)
    targets = np.asarray(targets, dtype=np.int64)
    J = rows.shape[1]
    finite = np.isfinite(rows).all(axis=1)
    inside = (targets >= 0) & (targets < J)
    return finite & inside, int((~finite).sum()), int((finite & ~inside).sum())


def bin_index(conf: np.ndarray, M: int) -> np.ndarray:
    """#{k in 1..M-1 : (double)conf > (double)k / (double)M}: right-closed bins, compared in float64."""
    edges = np.arange(M, dtype=np.float64) / np.float64(M)
    return (np.asarray(conf, dtype=np.float32).astype(np.float64)[:, None] > edges[None, 1:]).sum(axis=1).astype(np.int64)


def quantise(conf: np.ndarray) -> np.ndarray:
    """q = llrint((double)conf * 2^32), ties to even."""
    return np.rint(np.asarray(conf, dtype=np.float32).astype(np.float64) * 4294967296.0).astype(np.int64)


@dataclass
class BinsRef:
    table: list             # M rows of Python ints [rows, right, sum q]
    stats: list             # [valid, nonfinite, oob, right]
    brier_sum: float        # fsum of every squared difference of the valid rows
    brier_mag: float        # the same: every term is >= 0
    brier_terms: int


def bins(probs: np.ndarray, targets: np.ndarray, M: int) -> BinsRef:
    probs = np.asarray(probs, dtype=np.float32)
    targets = np.asarray(targets, dtype=np.int64)
    valid, nonfinite, oob = split_rows(probs, targets)
    p, y = probs[valid], targets[valid]
    n, J = p.shape
    table = [[0, 0, 0] for _ in range(M)]
    right_total = 0
    brier = 0.0
    if n:
        conf = p.max(axis=1)
        pred = p.argmax(axis=1)                     # the first index that attains the maximum
        b, q, right = bin_index(conf, M), quantise(conf), pred == y
        for k in range(M):
            sel = b == k
            table[k] = [int(sel.sum()), int((sel & right).sum()), sum(int(v) for v in q[sel].tolist())]
        right_total = int(right.sum())
        d = p.astype(np.float64)
        d[np.arange(n), y] -= 1.0
        brier = math.fsum((d * d).reshape(-1).tolist())
    return BinsRef(table, [int(n), nonfinite, oob, right_total], brier, brier, int(n) * int(J))


def ece_mce(table, valid: int):
    """(ece, mce) from the integer table: one division of Python integers each; (None, None) without a valid row."""
    if not valid:
        return None, None
    gaps = [abs(c * Q_ONE - q) for _, c, q in table]
    return sum(gaps) / (valid * Q_ONE), max(g / (r * Q_ONE) for g, (r, _, _) in zip(gaps, table) if r)


@dataclass
class NllRef:
    out: np.ndarray         # [K, 3] fsum of the rows' nll / g / h terms
    mag: np.ndarray         # [K, 3] summed magnitude of what each row's term is made of (nll: |m| + |log s| + |a_y| + 1;
    #                         g: sum_j p_j |z_j| + |z_y|; h: sum_j p_j z_j^2 + (sum_j p_j z_j)^2)
    amax: np.ndarray        # [K] max |beta z| over the valid rows
    stats: list             # [nonfinite, oob]
    valid: int


def nll(logits: np.ndarray, targets: np.ndarray, betas) -> NllRef:
    logits = np.asarray(logits, dtype=np.float32)
    targets = np.asarray(targets, dtype=np.int64)
    valid, nonfinite, oob = split_rows(logits, targets)
    z, y = logits[valid].astype(np.float64), targets[valid]
    n = z.shape[0]
    betas = [float(b) for b in betas]
    out, mag, amax = np.zeros((len(betas), 3)), np.zeros((len(betas), 3)), np.zeros(len(betas))
    if n:
        rows = np.arange(n)
        zy = z[rows, y]
        for k, beta in enumerate(betas):
            a = beta * z
            m = a.max(axis=1)
            e = np.exp(a - m[:, None])
            s = e.sum(axis=1)
            p = e / s[:, None]
            mean1, mean2 = (p * z).sum(axis=1), (p * (z * z)).sum(axis=1)
            ay = beta * zy
            out[k] = [math.fsum((m + np.log(s) - ay).tolist()), math.fsum((mean1 - zy).tolist()),
                      math.fsum((mean2 - mean1 * mean1).tolist())]
            mag[k] = [math.fsum((np.abs(m) + np.abs(np.log(s)) + np.abs(ay) + 1.0).tolist()),
                      math.fsum(((p * np.abs(z)).sum(axis=1) + np.abs(zy)).tolist()),
                      math.fsum((mean2 + mean1 * mean1).tolist())]
            amax[k] = float(np.abs(a).max())
    return NllRef(out, mag, amax, [nonfinite, oob], int(n))


def sum_bound(mag: float, addends: int, per_row: float) -> float:
    """|device sum - fsum reference| <= this.  The device adds `addends` terms in some fixed order: at most (addends - 1) u /
    (1 - (addends - 1) u) times the summed magnitude (Higham, Accuracy and Stability, eq. 4.4).  Each side evaluates a term with
    a relative error of at most `per_row` u of its magnitude; fsum itself is exact to one rounding of the total."""
    gamma = (addends - 1) * U / (1.0 - (addends - 1) * U) if addends > 1 else 0.0
    return mag * (gamma + 2.0 * per_row * U + U)


def nll_per_row(J: int, amax: float) -> float:
    """The per-row factor of sum_bound for nll, g and h.  beta z_j - m carries an absolute error of at most 3 u A (A = max
    |beta z|: two roundings of products up to A and one of a difference up to 2 A), which exp turns into a relative error of
    each e_j; exp and log are good to 1 ulp; a sum of J positive terms adds (J - 1) u.  So s and every p_j are good to
    (6 A + J + 4) u, the weighted means sum_j p_j z_j and sum_j p_j z_j^2 to (6 A + 2 J + 6) u of sum_j p_j |z_j|^k, the square of
    the first and h to twice that, and nll = m + log s - a_y to u (|m| + |a_y| + |log s| + 3 A + J + 2), which the `+ 1` per row
    in its magnitude covers.  One factor for all three: 12 A + 4 J + 16."""
    return 12.0 * amax + 4.0 * J + 16.0


def geometric(lo: float, hi: float, count: int) -> list:
    ratio = hi / lo
    return [lo] + [lo * ratio ** (i / (count - 1)) for i in range(1, count - 1)] + [hi]


@dataclass
class FitRef:
    temperature: float
    nll_before: float
    nll_after: float
    at_bound: bool
    rounds: int
    beta: float


def fit_temperature(logits: np.ndarray, targets: np.ndarray, t_min: float = 0.05, t_max: float = 100.0) -> FitRef:
    """metrics.fit_temperature round for round, on nll() above."""
    lo, hi = 1.0 / float(t_max), 1.0 / float(t_min)
    first = nll(logits, targets, [lo, 1.0, hi])
    valid = first.valid
    before = first.out[1, 0] / valid
    if first.out[0, 1] >= 0.0:
        return FitRef(float(t_max), before, first.out[0, 0] / valid, True, 0, lo)
    if first.out[2, 1] <= 0.0:
        return FitRef(float(t_min), before, first.out[2, 0] / valid, True, 0, hi)
    g_lo, g_hi = float(first.out[0, 1]), float(first.out[2, 1])
    rounds = 0
    while rounds < MAX_ROUNDS and hi / lo - 1.0 > BRACKET_TOL:
        betas = geometric(lo, hi, ROUND_BETAS)
        g = nll(logits, targets, betas).out[:, 1]
        rounds += 1
        i = next((i for i in range(1, ROUND_BETAS) if g[i] > 0.0), ROUND_BETAS - 1)
        lo, hi, g_lo, g_hi = betas[i - 1], betas[i], float(g[i - 1]), float(g[i])
    beta = lo - g_lo * (hi - lo) / (g_hi - g_lo) if g_hi > g_lo else lo
    beta = min(max(beta, lo), hi)
    after = nll(logits, targets, [beta]).out[0, 0] / valid
    return FitRef(1.0 / beta, before, after, False, rounds, beta)


def gradient(logits: np.ndarray, targets: np.ndarray, beta: float) -> float:
    """g(beta) = d nll / d beta, summed over the valid rows."""
    return float(nll(logits, targets, [beta]).out[0, 1])


def planted(n: int, J: int, t0: float, seed: int, scale: float = 2.0):
    """Logits whose best temperature is t0 up to sampling noise: labels drawn from softmax(z), logits handed over as t0 z."""
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((n, J)) * scale).astype(np.float64)
    p = np.exp(z - z.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    y = (rng.random(n)[:, None] > np.cumsum(p, axis=1)).sum(axis=1).clip(0, J - 1).astype(np.int64)
    return (t0 * z).astype(np.float32), y
