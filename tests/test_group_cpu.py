"""Group pooling and the cluster bootstrap without a device: the reference of tests/_group_ref.py against the literal expansion of a
resample and against tests/_boot_ref.py, the duplication property that ties the cluster bootstrap to the plain one, metrics.group_ids,
the settings parser, and the ABI's constants, plans and argument checks."""

from __future__ import annotations

import ctypes
import io

import numpy as np
import pytest
import torch

from deepfakedetection_amd import _lib
from deepfakedetection_amd import metrics as M
from tests import _boot_ref as B
from tests import _group_ref as G
from tests import _metrics_ref as R


@pytest.fixture(scope="module")
def lib():
    if not _lib.LIB_PATH.exists():
        from deepfakedetection_amd.build import build

        build()
    return _lib.load()


# ------------------------------------------------------------------ the reference of the cluster bootstrap
@pytest.mark.parametrize("sizes", [[1], [3, 1], [2, 5, 1, 4], [7, 7, 7], [1, 1, 1, 1, 1, 9]])
def test_weighted_statistics_of_the_sample_counts_equal_the_expanded_resample(sizes):
    groups = len(sizes)
    rng = np.random.default_rng(sum(sizes) * 7 + groups)
    ids = rng.permutation(np.repeat(np.arange(groups), sizes))
    n = ids.size
    for trial in range(6):
        labels = rng.integers(0, 2, size=n).astype(np.int64)
        scores = ((rng.integers(0, 4, size=n) + 1.5 * labels) / 4).astype(np.float32)
        hit = rng.integers(0, 2, size=n).astype(np.uint8)
        cut = float(scores[rng.integers(0, n)])
        c = G.sample_counts(ids, groups, trial, 5)
        drawn = B.draws(groups, trial, 5)
        assert c.sum() == sum(sizes[g] for g in drawn.tolist())          # a resample's size varies with the groups it draws
        weighted = B.weighted_stats(scores, labels, c, cut, hit)
        index = np.concatenate([np.flatnonzero(ids == g) for g in drawn.tolist()])       # the resample, literally
        s, l, h = scores[index], labels[index], hit[index]
        P, N, _, _, two_u = R.groups(s, l)[3]
        tp, fp = (int(v[0]) for v in R.sweep(s, l, [cut]))
        fps, tps, _ = R.roc_counts(s, l)
        assert weighted == [P, N, two_u, tp, fp, int(h.sum())] + B.eer_segment(fps, tps, P, N)
        assert weighted[2] == R.two_u(s, l)


@pytest.mark.parametrize("n", [1, 2, 5, 33])
def test_identity_groups_give_the_plain_bootstrap(n):
    rng = np.random.default_rng(n)
    labels = rng.integers(0, 2, size=n).astype(np.int64)
    members = [((rng.integers(0, 5, size=n) + labels) / 5).astype(np.float32), rng.random(n).astype(np.float32)]
    hit = rng.integers(0, 2, size=n).astype(np.uint8)
    got = G.cluster_stats(members, labels == 1, np.arange(n), n, 9, 3, [0.5, 0.4], hit)
    assert np.array_equal(got, B.stats(members, labels == 1, 9, 3, [0.5, 0.4], hit))


def test_ids_out_of_range_count_for_nothing_in_the_reference():
    ids = np.array([0, 1, -1, 2, 3, 1])
    assert (G.sample_counts(ids, 3, 0, 0)[[2, 4]] == 0).all()
    per_group = np.bincount(B.draws(3, 0, 0), minlength=3)
    assert G.sample_counts(ids, 3, 0, 0)[[0, 1, 3, 5]].tolist() == per_group[[0, 1, 2, 1]].tolist()


DUP_GROUPS, DUP_M, DUP_SEED, DUP_B = 40, 7, 11, 200


def _dup_case():
    rng = np.random.default_rng(4)
    labels = (np.arange(DUP_GROUPS) % 2).astype(np.int64)
    base = ((2 * rng.permutation(DUP_GROUPS) + 21 * labels) / 120.0).astype(np.float32)         # even / odd numerators: distinct
    assert np.unique(base).size == DUP_GROUPS
    return base, labels, np.repeat(np.arange(DUP_GROUPS), DUP_M)


def test_duplicated_scores_the_cluster_bootstrap_is_the_plain_bootstrap_of_the_groups():
    """G distinct scores, each repeated m = 7 times as one group.  A cluster resample is the plain resample of the G scores with
    every count times m: P and N scale by m, two_u, P N by m^2, so AUC and accuracy are the same rationals and, the division being
    correctly rounded, the same f64 bits.  The frame bootstrap of the same 280 rows treats them as independent: its interval is
    strictly narrower."""
    base, labels, ids = _dup_case()
    cut = float(np.sort(base)[DUP_GROUPS // 2])
    plain = B.stats([base], labels == 1, DUP_B, DUP_SEED, [cut])
    clustered = G.cluster_stats([base[ids]], labels[ids] == 1, ids, DUP_GROUPS, DUP_B, DUP_SEED, [cut])
    assert np.array_equal(clustered[0, :, :2], DUP_M * plain[0, :, :2]) and np.array_equal(clustered[0, :, 2], DUP_M ** 2 * plain[0, :, 2])
    for metric in ("auc", "accuracy"):
        a, b = M.boot_values(clustered, metric), M.boot_values(plain, metric)
        assert np.array_equal(a.view(np.int64), b.view(np.int64)), metric
        assert np.array_equal(a, B.values(clustered, metric), equal_nan=True)
    frames = B.stats([base[ids]], labels[ids] == 1, DUP_B, DUP_SEED, [cut])
    for metric in ("auc", "accuracy"):
        lo, hi = B.interval(M.boot_values(clustered, metric)[0], 0.95)
        flo, fhi = B.interval(M.boot_values(frames, metric)[0], 0.95)
        assert fhi - flo < hi - lo, (metric, (flo, fhi), (lo, hi))


# ------------------------------------------------------------------ the reference of the pooling
def test_pool_reference_on_hand_made_rows():
    half = 2.0 ** -33                                                   # q = rint(half 2^32) = rint(0.5) = 0, 3 half -> rint(1.5) = 2
    p = np.array([[half, 1.0], [3 * half, 0.0], [0.25, 0.75], [0.5, 0.5], [np.nan, 0.1], [0.1, 0.2]], dtype=np.float32)
    ids, targets = [0, 0, 1, 1, 1, 7], [1, 1, 0, 0, 0, 0]
    probs, preds, tgt, sizes, info = G.pool(p, ids, targets, 3, "mean")
    assert probs[0].tolist() == [np.float32(2 / (2 * 2.0 ** 32)), 0.5] and probs[1].tolist() == [0.375, 0.625] and probs[2].tolist() == [0, 0]
    assert preds.tolist() == [1, 1, 0] and tgt.tolist() == [1, 0, -1] and sizes.tolist() == [2, 2, 0] and info == [1, 1, 0, 1]
    vote = G.pool(p, ids, targets, 3, "vote")
    assert vote[0].tolist() == [[0.5, 0.5], [0.5, 0.5], [0.0, 0.0]] and vote[1].tolist() == [0, 0, 0]      # [0.5, 0.5] votes for class 0
    top = G.pool(p, ids, targets, 3, "max", positive=1)
    assert top[0][0].tolist() == [np.float32(half), 1.0] and top[0][1].tolist() == [0.25, 0.75]
    low = G.pool(np.array([[0.5, 0.1], [0.5, 0.9], [-0.0, 0.3], [0.0, 0.4]], dtype=np.float32), [0, 0, 1, 1], [0, 0, 1, 1], 2, "max", positive=0)
    assert low[0].tolist() == [[0.5, np.float32(0.1)], [0.0, np.float32(0.3)]]         # ties (and -0.0 == 0.0) keep the lowest index
    mixed = G.pool(p[:4], [0, 0, 0, 0], [1, 0, 1, 1], 1)
    assert mixed[2].tolist() == [0] and mixed[4] == [0, 0, 1, 0]


# ------------------------------------------------------------------ group_ids
def test_group_ids_by_parent_directory():
    root = "/data/test"
    paths = [f"{root}/Fake/v1/0.png", f"{root}/Fake/v1/1.png", f"{root}/Fake/v2/0.png", f"{root}/Real/v1/0.png", f"{root}/Real/loose.png",
             f"{root}/Real/other.png", f"{root}/Real/v1/1.png", f"{root}/Fake/v1/deep/2.png"]
    ids, count, names = M.group_ids(paths, root)
    assert ids.dtype == np.int32 and ids.tolist() == [0, 0, 1, 2, 3, 4, 2, 5] and count == 6
    assert names == ["Fake/v1", "Fake/v2", "Real/v1", "Real/loose.png", "Real/other.png", "Fake/v1/deep"]
    flat = [f"{root}/Fake/a_1.png", f"{root}/Fake/a_2.png", f"{root}/Real/b_1.png"]
    assert M.group_ids(flat, root)[0].tolist() == [0, 1, 2]             # a flat layout: every file is its own group
    assert M.group_ids([], root) [1] == 0
    assert M.group_ids([f"{root}/Fake/v1/0.png"], root + "/")[2] == ["Fake/v1"]


def test_group_ids_by_regex():
    root = "/data/test"
    pattern = r"^(.+)_\d+$"
    paths = [f"{root}/Fake/v1_000.png", f"{root}/Fake/v1_001.png", f"{root}/Real/v1_000.png", f"{root}/Fake/v2_7.png", f"{root}/Fake/nomatch.png",
             f"{root}/Fake/v1_002.jpg", f"{root}/Fake/sub/v1_000.png", f"{root}/Fake/v1.png"]
    ids, count, names = M.group_ids(paths, root, "regex", pattern)
    assert ids.tolist() == [0, 0, 1, 2, 3, 0, 4, 5] and count == 6
    assert names == ["Fake/v1", "Real/v1", "Fake/v2", "Fake/nomatch.png", "Fake/sub/v1", "Fake/v1.png"]     # the lone file is not the video v1
    for bad in (dict(key="stem"), dict(key="regex"), dict(key="regex", pattern=r"^.+_\d+$")):
        with pytest.raises(ValueError):
            M.group_ids(paths, root, **bad)


# ------------------------------------------------------------------ the settings
def test_group_settings_parse():
    from deepfakedetection_amd.orchestration.orchestrator import group_settings

    assert group_settings(None) is None and group_settings(False) is None
    assert group_settings({}) == ("parent", None, "mean") == group_settings({"key": "parent", "pool": "mean"})
    assert group_settings({"key": "regex", "pattern": r"^(.+)_\d+$", "pool": "vote"}) == ("regex", r"^(.+)_\d+$", "vote")
    assert group_settings({"pool": "MAX"}) == ("parent", None, "max")
    for bad in (True, "parent", {"key": "stem"}, {"pool": "median"}, {"key": "regex"}, {"key": "regex", "pattern": "^.+$"},
                {"key": "regex", "pattern": "(("}, {"key": "parent", "pattern": "(.)"}, {"by": "parent"}):
        with pytest.raises(ValueError):
            group_settings(bad)


def test_inference_settings_ignore_group_by_where_it_cannot_run(tmp_path):
    from rich.console import Console

    from deepfakedetection_amd.orchestration import orchestrator as O

    def settings(infer):
        sink = io.StringIO()
        cfg = {"device": "cpu", "data": {"root": str(tmp_path), "num_classes": 2, "img_size": 32}}
        s = O.inference_settings(cfg, {"name": "efficientnet_b0", "inference": infer}, Console(file=sink, width=200))
        return s, sink.getvalue()

    s, text = settings({})
    assert s.group_by is None and "group_by" not in text
    s, text = settings({"group_by": {"key": "parent"}})                                     # no device_metrics
    assert s.group_by is None and text.count("inference.group_by ignored") == 1
    s, text = settings({"group_by": {"key": "parent"}, "device_metrics": True})            # no CUDA device: device_metrics falls away
    assert s.group_by is None and text.count("inference.group_by ignored") == 1
    with pytest.raises(ValueError):
        settings({"group_by": {"pool": "median"}})


# ------------------------------------------------------------------ the ABI without a device
def test_abi_constants_and_sources(lib):
    from deepfakedetection_amd import kernels as K
    from deepfakedetection_amd.build import SOURCES

    assert lib.dfd_version() >= 154 and "dfd_group.hip" in SOURCES
    header = (_lib.LIB_PATH.parents[1] / "include" / "dfd_hip.h").read_text()
    for name, value in (("DFD_GROUP_MEAN", _lib.GROUP_MEAN), ("DFD_GROUP_VOTE", _lib.GROUP_VOTE), ("DFD_GROUP_MAX", _lib.GROUP_MAX),
                        ("DFD_GROUP_MAX_J", _lib.GROUP_MAX_J), ("DFD_GROUP_LDS_BYTES", _lib.GROUP_LDS_BYTES),
                        ("DFD_GROUP_LDS_MAX_BLOCKS", _lib.GROUP_LDS_MAX_BLOCKS), ("DFD_GROUP_GLOBAL_MAX_BLOCKS", _lib.GROUP_GLOBAL_MAX_BLOCKS),
                        ("DFD_GROUP_TIER_LDS", _lib.GROUP_TIER_LDS), ("DFD_GROUP_TIER_GLOBAL", _lib.GROUP_TIER_GLOBAL),
                        ("DFD_BOOT_GROUPED_MAX_WEIGHT", _lib.BOOT_GROUPED_MAX_WEIGHT)):
        assert f"#define {name} {value}\n" in header, name
    assert "#define DFD_GROUP_MAX_N (1 << 24)" in header and _lib.GROUP_MAX_N == 1 << 24
    assert _lib.GROUP_MAX_J == _lib.FUSE_MAX_J and _lib.BOOT_GROUPED_MAX_WEIGHT == 2 ** 31 - 1
    assert G.MODES == {"mean": K.GROUP_MEAN, "vote": K.GROUP_VOTE, "max": K.GROUP_MAX} == M.GROUP_POOLS
    for name in ("GroupScores", "group_pool", "group_ids"):
        assert name in M.__all__ and hasattr(M, name)
    for name in ("group_pool", "group_plan", "group_ws", "boot_stats_grouped", "boot_plan_grouped", "boot_ws_grouped"):
        assert hasattr(K, name)
    assert M.BootstrapResult(np.zeros((1, 1, 10), dtype=np.int64), 1, 0, 0.9, []).clusters is None


def test_group_plan_and_bad_arguments_without_a_gpu(lib):
    from deepfakedetection_amd import kernels as K

    EINVAL, one = -1, 0x1000
    plan = (ctypes.c_int * 4)()
    for J in (1, 2, 5, 1024):
        edge = _lib.GROUP_LDS_BYTES // (8 * J + 12)                    # the cells, sizes and target bounds of G groups: G (8 J + 12) bytes
        n = edge + 10
        assert lib.dfd_group_ws(n, edge, J) == edge * (8 * J + 12) <= _lib.GROUP_LDS_BYTES < lib.dfd_group_ws(n, edge + 1, J)
        lds, glb = K.group_plan(n, edge, J), K.group_plan(n, edge + 1, J)
        assert lds == K.GroupPlan(K.GROUP_TIER_LDS, (n + 4095) // 4096, edge * (8 * J + 12), (edge + 255) // 256)
        assert glb == K.GroupPlan(K.GROUP_TIER_GLOBAL, min((n + 255) // 256, _lib.GROUP_GLOBAL_MAX_BLOCKS), 0, (edge + 256) // 256)
    assert K.group_plan(1 << 24, 7, 2).workgroups == _lib.GROUP_LDS_MAX_BLOCKS
    assert K.group_plan(1 << 24, 1 << 24, 2) == K.GroupPlan(K.GROUP_TIER_GLOBAL, _lib.GROUP_GLOBAL_MAX_BLOCKS, 0, 1 << 16)
    for bad in ((0, 0, 2), (10, 0, 2), (10, 11, 2), ((1 << 24) + 1, 5, 2), (10, 5, 0), (10, 5, 1025), (-1, -1, 2)):
        assert lib.dfd_group_plan(*bad, plan) == EINVAL and lib.dfd_group_ws(*bad) == 0, bad
        with pytest.raises(ValueError):
            K.group_plan(*bad)
    assert lib.dfd_group_plan(10, 5, 2, None) == EINVAL
    # dfd_group_pool(probs, group, targets, n, G, J, mode, positive, ws, ws_bytes, out_probs, out_preds, out_targets, sizes, info, stream)
    names = ("probs", "group", "targets", "n", "G", "J", "mode", "positive", "ws", "wsb", "o0", "o1", "o2", "o3", "o4", "stream")
    base = dict(probs=one, group=one, targets=one, n=10, G=5, J=2, mode=0, positive=1, ws=one, wsb=5 * 28, o0=one, o1=one, o2=one, o3=one,
                o4=one, stream=None)
    call = lambda **kw: lib.dfd_group_pool(*[{**base, **kw}[k] for k in names])
    for kw in (dict(G=0), dict(G=11), dict(n=0, G=0), dict(n=(1 << 24) + 1), dict(J=0), dict(J=1025), dict(mode=-1), dict(mode=3),
               dict(positive=-1), dict(positive=2), dict(wsb=5 * 28 - 1), dict(ws=one + 4), *[{k: None} for k in names if base[k] == one]):
        assert call(**kw) == EINVAL, kw


def test_grouped_boot_plan_and_bad_arguments_without_a_gpu(lib):
    from deepfakedetection_amd import kernels as K

    EINVAL, one, edge = -1, 0x1000, _lib.BOOT_LDS_MAX_N
    plan = (ctypes.c_int * 4)()
    n = 1 << 22                                                         # the boundary is on G, at an n far above it
    assert K.boot_plan_grouped(n, edge, 50, 65, 3, 0) == K.BootPlan(K.BOOT_TIER_LDS, 65, 1, (edge + 4095) // 4096)
    assert K.boot_plan_grouped(n, 1, n, 65, 3, 0).tier == K.BOOT_TIER_LDS and K.boot_plan(n, 65, 3).tier == K.BOOT_TIER_GLOBAL
    G1 = edge + 1
    assert K.boot_plan_grouped(n, G1, 50, 65, 3, 4 * G1 * 65) == K.BootPlan(K.BOOT_TIER_GLOBAL, 65, 1, (G1 + 4095) // 4096)
    assert K.boot_plan_grouped(n, G1, 50, 65, 3, 4 * G1) == K.BootPlan(K.BOOT_TIER_GLOBAL, 1, 65, (G1 + 4095) // 4096)
    assert K.boot_plan_grouped(n, G1, 50, 65, 3).per_pass == 65         # the default workspace
    assert lib.dfd_boot_ws_grouped(n, edge, 10) == 0 and lib.dfd_boot_ws_grouped(n, G1, 10) == 40 * G1 == K.boot_ws_grouped(n, G1, 10)
    assert lib.dfd_boot_ws_grouped(10, 11, 10) == 0 and lib.dfd_boot_ws_grouped(n, 0, 10) == 0 and lib.dfd_boot_ws_grouped(n, G1, 0) == 0
    with pytest.raises(RuntimeError, match="DFD_EINVAL"):
        K.boot_plan_grouped(n, G1, 50, 65, 3, 4 * G1 - 1)
    # G * max_size: 2^31 - 1 = 2147483647 = 1 x (2^31 - 1); at n = 2^24: 128 x 2^24 = 2^31 is just over, 127 x 2^24 under
    big = 1 << 24
    assert lib.dfd_boot_plan_grouped(big, 128, big, 5, 1, 0, plan) == EINVAL and lib.dfd_boot_plan_grouped(big, 127, big, 5, 1, 0, plan) == 0
    assert lib.dfd_boot_plan_grouped(big, 46341, 46341, 5, 1, 1 << 40, plan) == EINVAL          # 46341^2 = 2^31 + 4633
    assert lib.dfd_boot_plan_grouped(big, 46340, 46341, 5, 1, 1 << 40, plan) == 0               # 46340 x 46341 = 2^31 - 41708
    assert lib.dfd_boot_plan_grouped(big, 2147483647 // 4099, 4099, 5, 1, 1 << 40, plan) == 0
    assert lib.dfd_boot_plan_grouped(big, 2147483647 // 4099 + 1, 4099, 5, 1, 1 << 40, plan) == EINVAL
    # (n, G, max_size, B, M)
    for bad in ((10, 0, 1, 5, 1), (10, 11, 1, 5, 1), (10, 5, 0, 5, 1), (10, 5, 11, 5, 1), (0, 0, 0, 5, 1), (big + 1, 5, 5, 5, 1), (10, 5, 2, 0, 1),
                (10, 5, 2, 65537, 1), (10, 5, 2, 5, 0), (10, 5, 2, 5, 9)):
        assert lib.dfd_boot_plan_grouped(*bad, 1 << 40, plan) == EINVAL, bad
        with pytest.raises(ValueError):
            K.boot_plan_grouped(*bad)
    assert lib.dfd_boot_plan_grouped(10, 5, 2, 5, 1, 0, None) == EINVAL
    # dfd_boot_stats_grouped(score_ptrs, perm_ptrs, M, is_positive, hit, cuts, group, n, G, max_size, B, seed, ws, ws_bytes, stats, stream)
    ptrs, holes = (ctypes.c_void_p * 2)(one, one), (ctypes.c_void_p * 2)(one, None)
    cuts = (ctypes.c_double * 2)(0.5, float("nan"))
    names = ("s", "p", "M", "pos", "hit", "cuts", "group", "n", "G", "max_size", "B", "seed", "ws", "wsb", "stats", "stream")
    base = dict(s=ptrs, p=ptrs, M=2, pos=one, hit=None, cuts=cuts, group=one, n=10, G=5, max_size=4, B=5, seed=0, ws=None, wsb=0, stats=one,
                stream=None)
    call = lambda **kw: lib.dfd_boot_stats_grouped(*[{**base, **kw}[k] for k in names])
    far = dict(n=n, G=G1, max_size=50)
    for kw in (dict(G=0), dict(G=11), dict(max_size=0), dict(max_size=11), dict(n=big, G=128, max_size=big), dict(B=0), dict(B=65537), dict(M=0),
               dict(M=9), dict(s=None), dict(p=None), dict(s=holes), dict(p=holes), dict(pos=None), dict(group=None), dict(stats=None),
               dict(ws=one, wsb=4 * G1 - 4, **far), dict(ws=None, wsb=1 << 30, **far)):
        assert call(**kw) == EINVAL, kw


def test_front_end_argument_checks_need_no_gpu():
    from deepfakedetection_amd import kernels as K

    s, p, pos, g = torch.zeros(4), torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.uint8), torch.zeros(4, dtype=torch.int32)
    for args, kw in ((([s], [p], pos, g.long(), 2, 2, 5), {}), (([s], [p], pos, g[:3], 2, 2, 5), {}), (([s], [p], pos, g, 0, 2, 5), {}),
                     (([s], [p], pos, g, 5, 1, 5), {}), (([s], [p], pos, g, 2, 0, 5), {}), (([s], [p], pos, g, 2, 5, 5), {}),
                     (([s], [p], pos, g, 2, 2, 0), {}), (([s], [p.long()], pos, g, 2, 2, 5), {}), (([s], [p], pos, g, 2, 2, 5), dict(seed=-1)),
                     (([s], [p], pos, g, 2, 2, 5), dict(cuts=[0.5, 0.5]))):
        with pytest.raises(ValueError):
            K.boot_stats_grouped(*args, **kw)
    rows, t = torch.zeros(4, 2), torch.zeros(4, dtype=torch.int64)
    for args, kw in (((rows.double(), g, t, 2), {}), ((rows, g.long(), t, 2), {}), ((rows, g, t.int(), 2), {}), ((rows, g[:3], t, 2), {}),
                     ((rows, g, t, 0), {}), ((rows, g, t, 5), {}), ((rows, g, t, 2), dict(mode=3)), ((rows, g, t, 2), dict(positive=2))):
        with pytest.raises(ValueError):
            K.group_pool(*args, **kw)
    with pytest.raises(ValueError):
        M.group_pool(rows, g, t, mode="median")
