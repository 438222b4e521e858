"""The bootstrap without a device: the Philox known answers and the resampling rule of tests/_boot_ref.py, the reference's weighted
and expanded formulations against a brute-force pair count, the interval / delta / p arithmetic of deepfakedetection_amd.metrics on
hand-made arrays, the settings parser, the ABI's argument checks, and one sanity check of the method itself."""

from __future__ import annotations

import ctypes
import json
import math

import numpy as np
import pytest
import torch

from deepfakedetection_amd import _lib
from deepfakedetection_amd import metrics as M
from tests import _boot_ref as B
from tests import _metrics_ref as R


@pytest.fixture(scope="module")
def lib():
    if not _lib.LIB_PATH.exists():
        from deepfakedetection_amd.build import build

        build()
    return _lib.load()


# ------------------------------------------------------------------ the generator and the draws
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
])
def test_philox_known_answers(counter, key, want):
    """The Random123 known-answer vectors of Philox4x32-10."""
    assert tuple(int(w[0]) for w in B.philox4x32_10(counter, key)) == want


def test_philox_is_vectorised_over_the_counter():
    blocks = np.arange(5, dtype=np.uint64)
    table = np.stack(B.philox4x32_10((blocks, 7, 0, B.BOOT_STREAM), (3, 9)), axis=1)
    for q in range(5):
        assert tuple(int(w[0]) for w in B.philox4x32_10((q, 7, 0, B.BOOT_STREAM), (3, 9))) == tuple(table[q].tolist())


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 4097])
def test_counts_sum_to_n_and_follow_the_rule(n):
    seed = (0xDEADBEEF << 32) | 0x1234
    c = B.counts(n, 5, 3, seed)
    assert c.shape == (3, n) and (c.sum(axis=1) == n).all() and (c >= 0).all()
    for r in range(3):                                                  # the rule, draw by draw
        for t in sorted({0, n // 2, n - 1}):
            word = B.philox4x32_10((t >> 2, 5 + r, 0, 0x626F6F74), (seed & 0xFFFFFFFF, seed >> 32))[t & 3]
            assert B.draws(n, 5 + r, seed)[t] == (int(word[0]) * n) >> 32
    assert not np.array_equal(B.counts(64, 0, 1, 0), B.counts(64, 0, 1, 1)) and not np.array_equal(B.counts(64, 0, 1, 0), B.counts(64, 1, 1, 0))
    assert not np.array_equal(B.counts(64, 0, 1, 1), B.counts(64, 0, 1, 1 << 32))


# ------------------------------------------------------------------ the statistics of a resample
def _brute(scores, labels, c, cut, hit):
    """Pair counts over the expansion: every positive against every negative."""
    s, l, h = np.repeat(scores, c), np.repeat(labels, c), np.repeat(hit, c)
    pos, neg = s[l == 1], s[l == 0]
    two_u = sum(2 * int((neg < p).sum()) + int((neg == p).sum()) for p in pos)
    at = s.astype(np.float64) >= cut
    return [int(pos.size), int(neg.size), two_u, int((at & (l == 1)).sum()), int((at & (l == 0)).sum()), int(h.sum())]


@pytest.mark.parametrize("n,grid", [(1, 3), (2, 2), (7, 3), (25, 5), (40, 1), (40, 4), (40, 1000)])
def test_weighted_statistics_equal_the_expansion_and_a_pair_count(n, grid):
    rng = np.random.default_rng(n * 31 + grid)
    for trial in range(6):
        labels = rng.integers(0, 2, size=n).astype(np.int64)
        scores = ((rng.integers(0, grid, size=n) + 0.4 * grid * labels) / grid).astype(np.float32)
        hit = rng.integers(0, 2, size=n).astype(np.uint8)
        cut = float(scores[rng.integers(0, n)]) if trial % 2 else 0.55
        c = B.counts(n, trial, 1, 11)[0]
        expanded, weighted = B.resample_stats(scores, labels, c, cut, hit), B.weighted_stats(scores, labels, c, cut, hit)
        assert expanded == weighted
        assert expanded[:6] == _brute(scores, labels, c, cut, hit)
        s, l = np.repeat(scores, c), np.repeat(labels, c)
        assert expanded[2] == R.two_u(s, l)
        want = R.eer(s, l)
        got = B.value(expanded, "eer")
        assert (want is None and math.isnan(got)) or abs(got - want) <= 1e-15
        fps, tps, _ = R.roc_counts(s, l)
        if expanded[0] and expanded[1]:
            assert got == M.eer_from_curve(fps, tps, expanded[0], expanded[1])


def test_statistics_without_cut_and_hit_are_zero():
    scores, labels = np.array([0.1, 0.7, 0.7, 0.9], dtype=np.float32), np.array([0, 1, 0, 1])
    row = B.resample_stats(scores, labels, [1, 1, 1, 1])
    assert row == [2, 2, 7, 0, 0, 0, 0, 1, 1, 2] == B.weighted_stats(scores, labels, [1, 1, 1, 1])
    assert B.resample_stats(scores, labels, [0, 2, 0, 2])[:3] == [4, 0, 0] and B.resample_stats(scores, labels, [0, 2, 0, 2])[6:] == [0, 0, 0, 0]


# ------------------------------------------------------------------ values, interval, delta
def _table(rows):
    return np.array(rows, dtype=np.int64)


def test_values_are_single_divisions_and_nan_without_a_class():
    #                P   N  two_u tp fp hits f0 t0 f1 t1
    table = _table([[[3, 4, 17, 2, 1, 5, 0, 1, 2, 2], [0, 7, 0, 0, 3, 4, 0, 0, 0, 0], [7, 0, 0, 6, 0, 7, 0, 0, 0, 0]]])
    for metric in B.METRICS:
        got, want = M.boot_values(table, metric), B.values(table, metric)
        assert got.shape == (1, 3) and np.array_equal(got, want, equal_nan=True), metric
    assert M.boot_values(table, "auc")[0, 0] == 17 / 24 and M.boot_values(table, "accuracy")[0, 0] == 5 / 7
    assert M.boot_values(table, "balanced_accuracy")[0, 0] == (2 * 4 + 3 * 3) / 24
    assert M.boot_values(table, "tpr")[0, 0] == 2 / 3 and M.boot_values(table, "fpr")[0, 0] == 1 / 4
    # the segment (0, 1) -> (2, 2): a0 = 4 - 12, a1 = 6 + 8 - 12
    assert M.boot_values(table, "eer")[0, 0] == (0 + (8 / 10) * 2) / 4
    for metric in B.METRICS[:-1]:
        assert np.isnan(M.boot_values(table, metric)[0, 1:]).all()
    assert M.boot_values(table, "hit_rate")[0].tolist() == [5 / 7, 4 / 7, 1.0]
    res = M.BootstrapResult(table, 3, 0, 0.9, [dict.fromkeys(M.BOOT_METRICS)])
    assert res.degenerate(0) == 2 and res.interval("auc") == (17 / 24, 17 / 24)
    with pytest.raises(ValueError):
        M.boot_values(table, "f1")


def test_interval_and_delta_on_hand_made_arrays():
    nan = float("nan")
    v = np.array([0.5, nan, 0.1, 0.9, 0.3, nan, 0.7])
    assert M.percentile_interval(v, 0.5) == tuple(np.quantile([0.5, 0.1, 0.9, 0.3, 0.7], [0.25, 0.75]).tolist()) == B.interval(v, 0.5)
    assert M.percentile_interval(np.array([nan, nan]), 0.95) is None and M.percentile_interval(np.array([]), 0.95) is None
    assert M.percentile_interval(np.array([0.25]), 0.95) == (0.25, 0.25)

    a = np.array([0.9, 0.8, nan, 0.7, 0.6, 0.5])
    b = np.array([0.8, 0.8, 0.1, nan, 0.7, 0.4])
    d = M.paired_delta("auc", 0.75, 0.5, a, b, 0.9)
    # differences where both exist: 0.1, 0.0, -0.1, 0.1 -> #{<= 0} = 2, #{>= 0} = 3, valid = 4
    assert d.valid == 4 and d.point == 0.25 and d.p == min(1.0, 2 * 3 / 5) == 1.0
    assert (d.lo, d.hi, d.p, d.valid) == B.delta(a, b, 0.9)
    better = M.paired_delta("auc", 0.9, 0.8, np.full(99, 0.9), np.full(99, 0.8), 0.95)
    assert better.p == 2 * 1 / 100 and better.valid == 99 and better.lo == better.hi and better.lo > 0
    worse = M.paired_delta("auc", 0.8, 0.9, np.full(99, 0.8), np.full(99, 0.9), 0.95)
    assert worse.p == 0.02 and worse.hi < 0
    ties = M.paired_delta("auc", 0.5, 0.5, np.full(9, 0.5), np.full(9, 0.5), 0.95)          # all differences 0: both counts are 9
    assert ties.p == 1.0 and (ties.lo, ties.hi) == (0.0, 0.0)
    none = M.paired_delta("auc", None, 0.5, np.full(4, nan), np.full(4, 0.5), 0.95)
    assert (none.point, none.lo, none.hi, none.p, none.valid) == (None, None, None, 1.0, 0) and B.delta(np.full(4, nan), np.full(4, 0.5), 0.95) == (None, None, 1.0, 0)


# ------------------------------------------------------------------ the method itself, on the reference alone
def _hanley_mcneil(auc: float, P: int, N: int) -> float:
    q1, q2 = auc / (2 - auc), 2 * auc * auc / (1 + auc)
    return math.sqrt((auc * (1 - auc) + (P - 1) * (q1 - auc * auc) + (N - 1) * (q2 - auc * auc)) / (P * N))


def _boot_sd_over_hm(seed: int, n: int = 2000, replicates: int = 1000):
    rng = np.random.default_rng(seed)
    labels = (np.arange(n) % 5 == 0).astype(np.int64)                   # a 1:4 split
    scores = (rng.standard_normal(n) + 1.5 * labels).astype(np.float32)
    point = R.auc(scores, labels)
    aucs = np.array([R.auc(scores[idx], labels[idx]) for idx in (B.draws(n, b, seed) for b in range(replicates))])
    lo, hi = B.interval(aucs, 0.95)
    return point, lo, hi, float(aucs.std(ddof=1)) / _hanley_mcneil(point, int(labels.sum()), int(n - labels.sum()))


HM_BOUND = 0.3975               # twice the worst |ratio - 1| over seeds 0..4 (the test's docstring)


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_the_percentile_interval_is_sane_against_hanley_mcneil(seed):
    """n = 2000 (400 positives N(1.5, 1), 1600 negatives N(0, 1): AUC about 0.86), B = 1000.  The 95 % percentile interval of the
    AUC contains the point AUC, and the bootstrap standard deviation over the Hanley-McNeil standard error stays within HM_BOUND of
    1.  HM_BOUND is twice the worst |ratio - 1| measured with this reference over the seeds 0..4 before the bound was fixed.  The
    five ratios were 0.84298, 0.80128, 0.82984, 0.81955 and 0.84396 (Hanley-McNeil's exponential model overstates the variance of
    normal scores a little), the worst deviation 0.19872, so the bound is 0.3975."""
    point, lo, hi, ratio = _boot_sd_over_hm(seed)
    assert lo < point < hi
    assert abs(ratio - 1.0) <= HM_BOUND, ratio


# ------------------------------------------------------------------ the ABI without a device
def test_abi_constants_and_sources(lib):
    from deepfakedetection_amd import kernels as K
    from deepfakedetection_amd.build import SOURCES

    assert lib.dfd_version() >= 153 and "dfd_boot.hip" in SOURCES
    header = (_lib.LIB_PATH.parents[1] / "include" / "dfd_hip.h").read_text()
    for name, value in (("DFD_BOOT_MAX_REPLICATES", _lib.BOOT_MAX_REPLICATES), ("DFD_BOOT_MAX_MEMBERS", _lib.BOOT_MAX_MEMBERS),
                        ("DFD_BOOT_STATS_LEN", _lib.BOOT_STATS_LEN), ("DFD_BOOT_SCRATCH_BYTES", _lib.BOOT_SCRATCH_BYTES),
                        ("DFD_BOOT_DRAW_TILE", _lib.BOOT_DRAW_TILE), ("DFD_BOOT_TIER_LDS", _lib.BOOT_TIER_LDS),
                        ("DFD_BOOT_TIER_GLOBAL", _lib.BOOT_TIER_GLOBAL)):
        assert f"#define {name} {value}\n" in header, name
    assert "#define DFD_BOOT_STREAM 0x626f6f74u" in header and _lib.BOOT_STREAM == 0x626F6F74 == B.BOOT_STREAM
    assert "#define DFD_BOOT_MAX_N (1 << 24)" in header and _lib.BOOT_MAX_N == 1 << 24
    assert "#define DFD_BOOT_LDS_MAX_N ((160 * 1024 - DFD_BOOT_SCRATCH_BYTES) / 4)" in header
    assert _lib.BOOT_LDS_MAX_N == (160 * 1024 - _lib.BOOT_SCRATCH_BYTES) // 4 == 40832
    assert (_lib.BOOT_MAX_REPLICATES, _lib.BOOT_MAX_MEMBERS, _lib.BOOT_STATS_LEN) == (65536, 8, 10)
    for name in ("BootstrapResult", "DeltaResult", "bootstrap"):
        assert name in M.__all__ and hasattr(M, name)
    for name in ("boot_plan", "boot_ws", "boot_counts", "boot_stats"):
        assert hasattr(K, name)
    philox = (_lib.LIB_PATH.parent / "csrc" / "dfd_philox.h").read_text()
    for source in ("dfd_vit.hip", "dfd_boot.hip"):
        text = (_lib.LIB_PATH.parent / "csrc" / source).read_text()
        assert '#include "dfd_philox.h"' in text and "0xD2511F53" not in text and "0xD2511F53" in philox


def test_plan_and_bad_arguments_without_a_gpu(lib):
    from deepfakedetection_amd import kernels as K

    EINVAL = -1
    one, edge = 0x1000, _lib.BOOT_LDS_MAX_N
    plan = (ctypes.c_int * 4)()
    assert lib.dfd_boot_ws(edge, 10) == 0 and lib.dfd_boot_ws(edge + 1, 10) == 10 * 4 * (edge + 1)
    assert lib.dfd_boot_ws(-1, 10) == 0 and lib.dfd_boot_ws(_lib.BOOT_MAX_N + 1, 10) == 0 and lib.dfd_boot_ws(100000, 0) == 0
    assert lib.dfd_boot_ws(100000, _lib.BOOT_MAX_REPLICATES + 1) == 0
    assert K.boot_plan(edge, 65, 3, 0) == K.BootPlan(K.BOOT_TIER_LDS, 65, 1, (edge + 4095) // 4096)
    assert K.boot_plan(0, 1, 1, 0).tier == K.BOOT_TIER_LDS
    n = edge + 1
    assert K.boot_plan(n, 65, 3, 4 * n * 65) == K.BootPlan(K.BOOT_TIER_GLOBAL, 65, 1, (n + 4095) // 4096)
    assert K.boot_plan(n, 65, 3, 4 * n * 1000).per_pass == 65
    assert K.boot_plan(n, 65, 3, 4 * n * 3 + 4 * n - 1) == K.BootPlan(K.BOOT_TIER_GLOBAL, 3, 22, (n + 4095) // 4096)
    assert K.boot_plan(n, 65, 3, 4 * n) == K.BootPlan(K.BOOT_TIER_GLOBAL, 1, 65, (n + 4095) // 4096)
    assert K.boot_plan(1_000_000, 2000).per_pass == (1 << 30) // 4_000_000             # the workspace boot_stats allocates is capped
    with pytest.raises(RuntimeError, match="DFD_EINVAL"):
        K.boot_plan(n, 65, 3, 4 * n - 1)
    for bad in ((-1, 5, 1), (_lib.BOOT_MAX_N + 1, 5, 1), (10, 0, 1), (10, _lib.BOOT_MAX_REPLICATES + 1, 1), (10, 5, 0), (10, 5, 9)):
        assert lib.dfd_boot_plan(*bad, 1 << 40, plan) == EINVAL, bad
        with pytest.raises(ValueError):
            K.boot_plan(*bad)
    assert lib.dfd_boot_plan(10, 5, 1, 0, None) == EINVAL
    # dfd_boot_counts(n, b0, R, seed, counts, stream)
    for n_, b0, R_ in ((-1, 0, 1), (_lib.BOOT_MAX_N + 1, 0, 1), (10, -1, 1), (10, 0, 0), (10, 65536, 1), (10, 65530, 7)):
        assert lib.dfd_boot_counts(n_, b0, R_, 0, one, None) == EINVAL, (n_, b0, R_)
    assert lib.dfd_boot_counts(10, 0, 1, 0, None, None) == EINVAL
    # dfd_boot_stats(score_ptrs, perm_ptrs, M, is_positive, hit, cuts, n, B, seed, ws, ws_bytes, stats, stream)
    ptrs = (ctypes.c_void_p * 2)(one, one)
    holes = (ctypes.c_void_p * 2)(one, None)
    cuts = (ctypes.c_double * 2)(0.5, float("nan"))
    call = lambda **kw: lib.dfd_boot_stats(*[{**dict(s=ptrs, p=ptrs, M=2, pos=one, hit=None, cuts=cuts, n=10, B=5, seed=0, ws=None,
                                                     wsb=0, stats=one, stream=None), **kw}[k]
                                             for k in ("s", "p", "M", "pos", "hit", "cuts", "n", "B", "seed", "ws", "wsb", "stats", "stream")])
    for kw in (dict(n=-1), dict(n=_lib.BOOT_MAX_N + 1), dict(B=0), dict(B=65537), dict(M=0), dict(M=9), dict(s=None), dict(p=None),
               dict(s=holes), dict(p=holes), dict(pos=None), dict(stats=None), dict(n=edge + 1, ws=one, wsb=4 * edge), dict(n=edge + 1, ws=None, wsb=1 << 30)):
        assert call(**kw) == EINVAL, kw


def test_front_end_argument_checks_need_no_gpu():
    from deepfakedetection_amd import kernels as K

    s, p, pos = torch.zeros(4), torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.uint8)
    for args, kw in ((([s], [p.long()], pos, 5), {}), (([s.double()], [p], pos, 5), {}), (([s], [p], pos.bool(), 5), {}),
                     (([s], [p], pos, 0), {}), (([s], [p], pos, 65537), {}), (([s], [p, p], pos, 5), {}), (([s], [p], pos[:3], 5), {}),
                     (([s], [p], pos, 5), dict(cuts=[0.5, 0.5])), (([s], [p], pos, 5), dict(hit=pos.long())), (([s], [p], pos, 5), dict(seed=-1)),
                     (([s], [p], pos, 5), dict(seed=1 << 64)), (([s] * 9, [p] * 9, pos, 5), {})):
        with pytest.raises(ValueError):
            K.boot_stats(*args, **kw)
    for args in ((-1, 0, 1, 0), (4, -1, 1, 0), (4, 0, 0, 0), (4, 65536, 1, 0), (4, 0, 1, -1)):
        with pytest.raises(ValueError):
            K.boot_counts(*args, "cpu")
    labels = torch.tensor([0, 1, 0, 1])
    for kw in (dict(replicates=0), dict(level=1.0), dict(level=0.0), dict(cut=[0.5, 0.5]), dict(cut=float("nan")), dict(hits=torch.ones(3))):
        with pytest.raises(ValueError):
            M.bootstrap(torch.rand(4), labels, **kw)
    with pytest.raises(ValueError):
        M.bootstrap([torch.rand(4), torch.rand(5)], labels)
    with pytest.raises(ValueError):
        M.bootstrap([], labels)


# ------------------------------------------------------------------ the settings
def test_bootstrap_settings_parse():
    from deepfakedetection_amd.orchestration.orchestrator import bootstrap_settings

    assert bootstrap_settings(None) is None and bootstrap_settings(False) is None
    assert bootstrap_settings({}) == (2000, 0.95, 0) == bootstrap_settings(True)
    assert bootstrap_settings({"replicates": 500, "level": "0.9", "seed": (1 << 64) - 1}) == (500, 0.9, (1 << 64) - 1)
    for bad in ({"replicates": 0}, {"replicates": 65537}, {"level": 0}, {"level": 1.0}, {"level": "wide"}, {"seed": -1}, {"seed": 1 << 64},
                {"resamples": 100}, {"replicates": 100, "stratified": True}):
        with pytest.raises(ValueError):
            bootstrap_settings(bad)
    with pytest.raises(ValueError, match="ensemble.bootstrap"):
        bootstrap_settings(2000, "ensemble.bootstrap")


def test_inference_settings_ignore_the_key_where_it_cannot_run(tmp_path):
    import io

    from rich.console import Console

    from deepfakedetection_amd.orchestration import orchestrator as O

    def settings(infer, num_classes=2, device="cpu"):
        sink = io.StringIO()
        cfg = {"device": device, "data": {"root": str(tmp_path), "num_classes": num_classes, "img_size": 32}}
        s = O.inference_settings(cfg, {"name": "efficientnet_b0", "inference": infer}, Console(file=sink, width=200))
        return s, sink.getvalue()

    s, text = settings({})
    assert s.bootstrap is None and "bootstrap" not in text
    s, text = settings({"bootstrap": {"replicates": 100}})                                  # no device_metrics
    assert s.bootstrap is None and text.count("inference.bootstrap ignored") == 1
    s, text = settings({"bootstrap": {"replicates": 100}, "device_metrics": True})          # no CUDA device: device_metrics falls away
    assert s.bootstrap is None and text.count("inference.bootstrap ignored") == 1
    s, text = settings({"bootstrap": True, "device_metrics": True}, num_classes=3)
    assert s.bootstrap is None and text.count("inference.bootstrap ignored") == 1
    with pytest.raises(ValueError):
        settings({"bootstrap": {"replicate": 100}})
    parse = lambda raw: O.ensemble_settings({"models": {"a": {}, "b": {}}, "ensemble": raw}, Console(file=io.StringIO()))
    assert parse({}).bootstrap is None and parse({"bootstrap": {"seed": 3}}).bootstrap == (2000, 0.95, 3)
    with pytest.raises(ValueError, match="ensemble.bootstrap"):
        parse({"bootstrap": {"level": 2}})
    assert json.dumps(parse({"bootstrap": True}).bootstrap) == "[2000, 0.95, 0]"
