"""Group pooling (csrc/dfd_group.hip through kernels.group_pool / metrics.group_pool) and the cluster bootstrap
(dfd_boot_stats_grouped through kernels.boot_stats_grouped / metrics.bootstrap(groups=)) against tests/_group_ref.py.  Every
comparison is at tolerance 0: == on integers and on the bits of floats.  Every output is an interior slice of a buffer filled with
the canary -1, the canaries around it must survive, and every case asserts the tier it ran through the plan functions."""

from __future__ import annotations

import json

import numpy as np
import pytest
import torch

from deepfakedetection_amd import kernels as K
from deepfakedetection_amd import metrics as M
from tests import _boot_ref as B
from tests import _group_ref as G

pytestmark = pytest.mark.gpu

GUARD = 32
EDGE = K.BOOT_LDS_MAX_N
MODES = ("mean", "vote", "max")
LAYOUTS = ("sorted", "rotated", "interleaved", "shuffled", "giant", "some_empty")
SPECIAL = np.array([0.0, 1.0, 2.0 ** -33, 3 * 2.0 ** -33, 1 - 2.0 ** -24], dtype=np.float32)


def _guarded(shape, dtype):
    count = int(np.prod(shape))
    big = torch.full((count + 2 * GUARD,), -1, dtype=dtype, device="cuda")
    return big, big[GUARD:GUARD + count].view(*shape)


def _intact(big: torch.Tensor) -> bool:
    host = big.cpu()
    return bool((host[:GUARD] == -1).all() and (host[-GUARD:] == -1).all())


def _lds_limit(J: int) -> int:
    """The largest G whose cells, sizes and target bounds fit the LDS tier."""
    return K.GROUP_LDS_BYTES // (8 * J + 12)


def _tier(n: int, groups: int, J: int) -> int:
    return K.GROUP_TIER_LDS if groups <= _lds_limit(J) else K.GROUP_TIER_GLOBAL


def _ids(n: int, groups: int, layout: str, rng) -> np.ndarray:
    if layout in ("sorted", "rotated"):
        ids = (np.arange(n) * groups) // n                              # runs of n / G, every group present
        return np.roll(ids, 1) if layout == "rotated" else ids
    if layout == "interleaved":
        return np.arange(n) % groups
    if layout == "shuffled":
        return rng.permutation((np.arange(n) * groups) // n)
    if layout == "giant":                                               # groups 1 .. G - 1 are singletons, group 0 takes the rest
        ids = np.zeros(n, dtype=np.int64)
        ids[rng.choice(n, size=groups - 1, replace=False)] = np.arange(1, groups)
        return ids
    return (rng.integers(0, (groups + 1) // 2, size=n) * 2) % groups    # some_empty: the odd groups stay empty


def _probs(n: int, J: int, rng) -> np.ndarray:
    p = rng.random((n, J)).astype(np.float32)
    special = rng.random((n, J)) < 0.4                                   # many exact ties, for the arg max and for the max key
    p[special] = SPECIAL[rng.integers(0, SPECIAL.size, size=int(special.sum()))]
    return p


def _plant(p, ids, targets, groups: int, J: int):
    """Rows that info has to count, and -0.0, which is a valid zero.  Returns what info[0] and info[1] gain."""
    n = p.shape[0]
    if n < 63:
        return 0, 0
    at = np.linspace(1, n - 2, 9).astype(np.int64)                      # nine distinct rows
    for k, value in enumerate((np.nan, -1e-3, 1 + 2.0 ** -23, np.inf)):
        p[at[k], k % J] = value
    p[at[4], 0] = -0.0
    targets[at[5]], targets[at[6]] = -1, J
    ids[at[7]], ids[at[8]] = -1, groups
    return 6, 2


def _pool(p, ids, targets, groups: int, mode: str, positive: int):
    """kernels.group_pool into guarded outputs -> numpy, after the canary check."""
    n, J = p.shape
    bufs = [_guarded((groups, J), torch.float32), _guarded((groups,), torch.int64), _guarded((groups,), torch.int64),
            _guarded((groups,), torch.int32), _guarded((4,), torch.int64)]
    got = K.group_pool(torch.from_numpy(p).cuda(), torch.from_numpy(ids.astype(np.int32)).cuda(), torch.from_numpy(targets).cuda(), groups,
                       G.MODES[mode], positive, out=[b[1] for b in bufs])
    torch.cuda.synchronize()
    assert all(g is b[1] for g, b in zip(got, bufs)) and all(_intact(b[0]) for b in bufs), "a write outside an output"
    return [g.cpu().numpy() for g in got]


def _same(got, want) -> bool:
    probs, preds, targets, sizes, info = got
    return (np.array_equal(probs.view(np.int32), want[0].view(np.int32)) and np.array_equal(preds, want[1]) and
            np.array_equal(targets, want[2]) and np.array_equal(sizes, want[3]) and info.tolist() == want[4])


# ------------------------------------------------------------------ pooling
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 4097])
def test_group_pool_sizes_layouts_and_modes(n):
    """Every (G, J) at this n with every id layout; the mode and the positive class rotate so that every layout meets every mode."""
    rng = np.random.default_rng(n)
    turn = 0
    for groups in sorted({g for g in (1, 2, 3, n) if g <= n}):
        for J in (2, 3, 5):
            plan = K.group_plan(n, groups, J)
            assert plan.tier == _tier(n, groups, J) and plan.workgroups >= 1
            if n == 4097:
                assert plan.workgroups > 1                             # more than one workgroup adds into the workspace
            for k, layout in enumerate(LAYOUTS):
                ids = _ids(n, groups, layout, rng).astype(np.int64)
                p = _probs(n, J, rng)
                targets = (ids % J).astype(np.int64)                    # one target per group
                bad, oob = _plant(p, ids, targets, groups, J)
                mode, positive = MODES[(turn + k) % 3], ((turn + k) // 3) % 2
                got = _pool(p, ids, targets, groups, mode, positive)
                want = G.pool(p, ids, targets, groups, mode, positive)
                assert want[4][:2] == [bad, oob]
                assert _same(got, want), (n, groups, J, layout, mode, positive, got[4], want[4])
            turn += 1


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("J,side", [(2, 0), (2, 1), (5, 0), (5, 1)])
def test_group_pool_on_both_sides_of_the_tier_boundary(J, side, mode):
    """The largest G of the LDS tier and the smallest of the global tier, with every layout; n = 4097 rows in several workgroups."""
    n, groups = 4097, _lds_limit(J) + side
    plan = K.group_plan(n, groups, J)
    assert plan.tier == (K.GROUP_TIER_GLOBAL if side else K.GROUP_TIER_LDS) and plan.workgroups > 1
    assert (plan.lds_bytes == K.group_ws(n, groups, J)) == (side == 0) and K.group_ws(n, groups, J) == groups * (8 * J + 12)
    rng = np.random.default_rng(groups)
    for k, layout in enumerate(LAYOUTS):
        ids = _ids(n, groups, layout, rng).astype(np.int64)
        p = _probs(n, J, rng)
        targets = (ids % J).astype(np.int64)
        _plant(p, ids, targets, groups, J)
        positive = k % 2
        assert _same(_pool(p, ids, targets, groups, mode, positive), G.pool(p, ids, targets, groups, mode, positive)), (layout, mode)


@pytest.mark.parametrize("tier", [K.GROUP_TIER_LDS, K.GROUP_TIER_GLOBAL])
@pytest.mark.parametrize("rotate", [0, 1])
def test_runs_that_end_inside_a_wave_at_its_end_and_across_workgroups(tier, rotate):
    """Sorted runs of 1, 63, 64, 65 and 129 rows (and the same rotated by one row, off the wave grid); in the global tier singleton
    groups follow until G passes the LDS limit, so the wave's segmented scan meets runs of every kind."""
    J = 2
    runs = [1, 63, 64, 65, 129]
    ids = np.repeat(np.arange(len(runs)), runs)
    if tier == K.GROUP_TIER_GLOBAL:
        ids = np.concatenate([ids, np.arange(len(runs), _lds_limit(J) + 1)])
    ids = np.roll(ids, rotate).astype(np.int64)
    n, groups = ids.size, int(ids.max()) + 1
    assert K.group_plan(n, groups, J).tier == tier
    rng = np.random.default_rng(rotate)
    p = _probs(n, J, rng)
    targets = (ids % J).astype(np.int64)
    for mode in MODES:
        for positive in (0, 1):
            got, want = _pool(p, ids, targets, groups, mode, positive), G.pool(p, ids, targets, groups, mode, positive)
            assert _same(got, want), (mode, positive)
            assert got[3][:5].tolist() == runs and got[4].tolist() == [0, 0, 0, 0]


def test_max_takes_the_lowest_index_among_equal_keys():
    """Rows that tie on probs[:, positive] (-0.0 ties with 0.0) differ in the other column: the copy shows which row won."""
    for groups, n in ((3, 300), (_lds_limit(2) + 1, 3 * (_lds_limit(2) + 1))):
        ids = (np.arange(n) % groups).astype(np.int64)
        p = np.zeros((n, 2), dtype=np.float32)
        p[:, 1] = np.where(ids % 3 == 0, 0.75, 0.0)                     # every member of a group ties
        p[ids % 3 == 2, 1] = np.tile(np.array([-0.0, 0.0], dtype=np.float32), n)[: int((ids % 3 == 2).sum())]
        p[:, 0] = (np.arange(n) + 1) / (n + 1)                          # the row's signature
        targets = np.zeros(n, dtype=np.int64)
        got = _pool(p, ids, targets, groups, "max", 1)
        assert _same(got, G.pool(p, ids, targets, groups, "max", 1))
        assert np.array_equal(got[0][:, 0], p[:groups, 0])             # group g first appears at row g


@pytest.mark.parametrize("extra", [0, 1])
def test_a_sum_past_2_53(extra):
    """One group of 2^21 + 3 rows at p = 1 - 2^-24, J = 2: the uint64 sum (2^21 + 3)(2^32 - 256) passes 2^53.  That sum is a
    multiple of 256 and so still an f64; with one more row at p = 2^-32 (q = 1) it is odd, no f64, and the uint64 -> f64 conversion
    has to round (to even) before the division."""
    n, J = (1 << 21) + 3, 2
    q = (1 << 32) - 256                                                 # rint((1 - 2^-24) 2^32)
    total = n * q + extra
    assert total > 1 << 53 and (int(float(total)) != total) == bool(extra)
    p = np.full((n + extra, J), 1 - 2.0 ** -24, dtype=np.float32)
    if extra:
        p[n // 2] = 2.0 ** -32
    n += extra
    ids, targets = np.zeros(n, dtype=np.int64), np.ones(n, dtype=np.int64)
    assert K.group_plan(n, 1, J).tier == K.GROUP_TIER_LDS
    probs, preds, tgt, sizes, info = _pool(p, ids, targets, 1, "mean", 1)
    want = np.float32(np.float64(float(total)) / (np.float64(n) * 4294967296.0))
    assert probs.view(np.int32).tolist() == [[int(want.view(np.int32))] * 2] and preds.tolist() == [0] and tgt.tolist() == [1]
    assert sizes.tolist() == [n] and info.tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("groups,J", [(37, 3), (_lds_limit(2) + 1, 2)])
def test_the_order_of_the_rows_does_not_change_a_bit(groups, J):
    n = 4097
    rng = np.random.default_rng(groups)
    ids = np.sort(rng.integers(0, groups, size=n)).astype(np.int64)
    p = _probs(n, J, rng)
    p[:, 1] = ((rng.permutation(n) + 1) / (n + 2)).astype(np.float32)   # distinct in the positive column: max has one winner
    targets = (ids % J).astype(np.int64)
    order = rng.permutation(n)
    for mode in MODES:
        a = _pool(p, ids, targets, groups, mode, 1)
        b = _pool(p[order], ids[order], targets[order], groups, mode, 1)
        assert _same(a, [b[0], b[1], b[2], b[3], b[4].tolist()]), mode


def test_mixed_targets_are_counted_and_raise_in_metrics():
    p = np.full((6, 2), 0.5, dtype=np.float32)
    ids, targets = np.array([0, 0, 1, 1, 2, 2], dtype=np.int64), np.array([1, 0, 1, 1, 0, 1], dtype=np.int64)
    got = _pool(p, ids, targets, 3, "mean", 1)
    assert _same(got, G.pool(p, ids, targets, 3, "mean", 1)) and got[4].tolist() == [0, 0, 2, 0] and got[2].tolist() == [0, 1, 0]
    with pytest.raises(ValueError, match="different targets"):
        M.group_pool(torch.from_numpy(p).cuda(), torch.from_numpy(ids).cuda(), torch.from_numpy(targets).cuda())
    res = M.group_pool(torch.from_numpy(p).cuda(), torch.from_numpy(ids).cuda(), torch.from_numpy(ids % 2).cuda(), mode="vote", num_groups=4)
    assert res.info == (0, 0, 0, 1) and res.sizes.tolist() == [2, 2, 2, 0] and res.targets.tolist() == [0, 1, 0, -1]
    assert res.probs.tolist() == [[1.0, 0.0]] * 3 + [[0.0, 0.0]]


# ------------------------------------------------------------------ the cluster bootstrap
def _groups_of(sizes, shuffle: bool, rng) -> np.ndarray:
    ids = np.repeat(np.arange(len(sizes)), sizes)
    return rng.permutation(ids) if shuffle else ids


def _scores(n: int, kind: str, rng):
    labels = rng.integers(0, 2, size=n).astype(np.int64)
    if n >= 2:
        labels[:2] = (0, 1)
    if kind == "grid":
        scores = np.clip(rng.integers(0, 5, size=n) + (labels == 1), 0, 4) / 4.0
    elif kind == "equal":
        scores = np.full(n, 0.25)
    else:
        scores = (2 * rng.permutation(n) + (2 * (n // 4) + 1) * labels) / (2.5 * n + 2.0)
    return scores.astype(np.float32), labels


def _run_grouped(members, labels, ids, groups, max_size, replicates, seed=0, cuts=None, hit=None, ws_bytes=None):
    ordered, perms = [], []
    for m in members:
        s, order = torch.sort(torch.from_numpy(m).cuda())
        ordered.append(s.contiguous())
        perms.append(order.to(torch.int32).contiguous())
    is_pos = torch.from_numpy((labels == 1).astype(np.uint8)).cuda()
    hit_d = torch.from_numpy(np.asarray(hit, dtype=np.uint8)).cuda() if hit is not None else None
    big, out = _guarded((len(members), replicates, K.BOOT_STATS_LEN), torch.int64)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda") if ws_bytes is not None else None
    got = K.boot_stats_grouped(ordered, perms, is_pos, torch.from_numpy(np.asarray(ids, dtype=np.int32)).cuda(), groups, max_size,
                               replicates, seed, cuts, hit_d, ws=ws, out=out)
    torch.cuda.synchronize()
    assert got is out and _intact(big), "a write outside stats"
    return out.cpu().numpy()


def _run_plain(members, labels, replicates, seed=0, cuts=None, hit=None):
    ordered, perms = [], []
    for m in members:
        s, order = torch.sort(torch.from_numpy(m).cuda())
        ordered.append(s.contiguous())
        perms.append(order.to(torch.int32).contiguous())
    is_pos = torch.from_numpy((labels == 1).astype(np.uint8)).cuda()
    hit_d = torch.from_numpy(np.asarray(hit, dtype=np.uint8)).cuda() if hit is not None else None
    return K.boot_stats(ordered, perms, is_pos, replicates, seed, cuts, hit_d).cpu().numpy()


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("groups", [1, 2, 5, 64, 65])
def test_cluster_bootstrap_small_group_counts(groups, shuffle):
    """Groups of 1, 7, 64 and 300 samples mixed, every score kind, with a cut, hit flags and three members; the LDS tier."""
    rng = np.random.default_rng(groups * 2 + shuffle)
    sizes = [(1, 7, 64, 300)[k % 4] for k in range(groups)]
    ids = _groups_of(sizes, shuffle, rng)
    n, replicates = ids.size, 4
    for kind in ("grid", "equal", "distinct"):
        cases = [_scores(n, kind, rng) for _ in range(3 if kind == "grid" else 1)]
        labels, members = cases[0][1], [c[0] for c in cases]
        cuts = [float(np.sort(m)[n // 2]) for m in members]
        hit = rng.integers(0, 2, size=n).astype(np.uint8)
        assert K.boot_plan_grouped(n, groups, max(sizes), replicates, len(members)).tier == K.BOOT_TIER_LDS
        got = _run_grouped(members, labels, ids, groups, max(sizes), replicates, seed=groups + 1, cuts=cuts, hit=hit)
        want = G.cluster_stats(members, labels == 1, ids, groups, replicates, groups + 1, cuts, hit)
        assert np.array_equal(got, want), (groups, kind, np.argwhere(got != want)[:5])
        single = _run_grouped(members[:1], labels, ids, groups, max(sizes), replicates, seed=groups + 1)
        assert np.array_equal(single[0][:, [0, 1, 2, 6, 7, 8, 9]], want[0][:, [0, 1, 2, 6, 7, 8, 9]]) and (single[0][:, 3:6] == 0).all()


@pytest.mark.parametrize("groups,tier", [(EDGE, K.BOOT_TIER_LDS), (EDGE + 1, K.BOOT_TIER_GLOBAL)])
def test_cluster_bootstrap_on_both_sides_of_the_tier_boundary(groups, tier):
    """The boundary is on G: n lies a few hundred above it.  The global tier with a workspace for one resample per pass and for all."""
    rng = np.random.default_rng(groups)
    sizes = np.ones(groups, dtype=np.int64)
    sizes[:3] = (7, 64, 300)
    ids = _groups_of(sizes, True, rng)
    n, replicates = ids.size, 3
    scores, labels = _scores(n, "grid", rng)
    hit = (np.arange(n) % 3 == 0).astype(np.uint8)
    plan = K.boot_plan_grouped(n, groups, 300, replicates, 1)
    assert plan.tier == tier and plan.per_pass == replicates and plan.passes == 1
    got = _run_grouped([scores], labels, ids, groups, 300, replicates, seed=5, cuts=[0.5], hit=hit)
    want = G.cluster_stats([scores], labels == 1, ids, groups, replicates, 5, [0.5], hit)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    if tier == K.BOOT_TIER_GLOBAL:
        assert K.boot_ws_grouped(n, groups, replicates) == 4 * groups * replicates
        assert K.boot_plan_grouped(n, groups, 300, replicates, 1, 4 * groups) == K.BootPlan(tier, 1, replicates, (groups + 4095) // 4096)
        for ws_bytes in (4 * groups, 4 * groups * replicates):
            assert np.array_equal(_run_grouped([scores], labels, ids, groups, 300, replicates, seed=5, cuts=[0.5], hit=hit, ws_bytes=ws_bytes), got)
    else:
        assert K.boot_ws_grouped(n, groups, replicates) == 0


@pytest.mark.parametrize("n", [5, 65, 2049, EDGE + 1])
def test_identity_groups_equal_the_plain_bootstrap(n):
    rng = np.random.default_rng(n)
    cases = [_scores(n, kind, rng) for kind in ("grid", "distinct")]
    labels, members = cases[0][1], [c[0] for c in cases]
    hit = rng.integers(0, 2, size=n).astype(np.uint8)
    tier = K.BOOT_TIER_LDS if n <= EDGE else K.BOOT_TIER_GLOBAL
    assert K.boot_plan_grouped(n, n, 1, 5, 2).tier == tier == K.boot_plan(n, 5, 2).tier
    got = _run_grouped(members, labels, np.arange(n), n, 1, 5, seed=3, cuts=[0.5, 0.4], hit=hit)
    assert np.array_equal(got, _run_plain(members, labels, 5, seed=3, cuts=[0.5, 0.4], hit=hit))


def test_ids_out_of_range_count_for_nothing():
    rng = np.random.default_rng(0)
    sizes = [7, 64, 1, 300, 7]
    ids = _groups_of(sizes, True, rng).astype(np.int64)
    n = ids.size
    scores, labels = _scores(n, "grid", rng)
    ids[[3, 50, 200]] = (-1, 5, 1 << 30)
    got = _run_grouped([scores], labels, ids, 5, 300, 6, seed=1, cuts=[0.5])
    assert np.array_equal(got, G.cluster_stats([scores], labels == 1, ids, 5, 6, 1, [0.5]))
    keep = (ids >= 0) & (ids < 5)
    order = np.flatnonzero(keep)
    assert np.array_equal(got, G.cluster_stats([scores[order]], labels[order] == 1, ids[order], 5, 6, 1, [0.5]))


@pytest.mark.parametrize("label", [0, 1])
def test_a_single_class_gives_zero_segments(label):
    rng = np.random.default_rng(label)
    ids = _groups_of([7, 64, 1, 300, 7], True, rng)
    n = ids.size
    scores, _ = _scores(n, "grid", rng)
    labels = np.full(n, label, dtype=np.int64)
    got = _run_grouped([scores], labels, ids, 5, 300, 4, seed=2, cuts=[0.5])
    assert np.array_equal(got, G.cluster_stats([scores], labels == 1, ids, 5, 4, 2, [0.5]))
    assert (got[0, :, label] == 0).all() and (got[0, :, 2] == 0).all() and (got[0, :, 6:] == 0).all()


def test_duplicated_scores_in_groups_equal_the_plain_bootstrap_of_the_groups():
    """G distinct scores, each repeated m = 7 times as one group: every cluster resample has the AUC and the accuracy of the plain
    resample of the G scores under the same seed, as f64 bits (the rational is the same, the division correctly rounded)."""
    groups, m, replicates, seed = 40, 7, 64, 11
    rng = np.random.default_rng(4)
    base, labels = _scores(groups, "distinct", rng)
    ids = np.repeat(np.arange(groups), m)
    cut = float(np.sort(base)[groups // 2])
    plain = _run_plain([base], labels, replicates, seed=seed, cuts=[cut])
    clustered = _run_grouped([base[ids]], labels[ids], ids, groups, m, replicates, seed=seed, cuts=[cut])
    assert np.array_equal(clustered[0, :, :2], m * plain[0, :, :2]) and np.array_equal(clustered[0, :, 2], m * m * plain[0, :, 2])
    for metric in ("auc", "accuracy", "balanced_accuracy", "tpr", "fpr"):
        a, b = M.boot_values(clustered, metric), M.boot_values(plain, metric)
        assert np.array_equal(a.view(np.int64), b.view(np.int64)), metric


# ------------------------------------------------------------------ metrics.bootstrap(groups=)
def test_bootstrap_with_groups_end_to_end_against_the_reference():
    groups, replicates, seed, level = 60, 200, 12, 0.9
    rng = np.random.default_rng(1)
    sizes = rng.integers(1, 12, size=groups)
    ids = rng.permutation(np.repeat(np.arange(groups), sizes))
    n = ids.size
    group_label = (np.arange(groups) % 3 == 0).astype(np.int64)
    labels = group_label[ids]
    centre = rng.standard_normal(groups)                                # the frames of a video share its offset
    a = (np.round((centre[ids] + 0.3 * rng.standard_normal(n)) * 8) / 8 + 1.5 * labels).astype(np.float32)
    b = (centre[ids] + rng.standard_normal(n) + 0.8 * labels).astype(np.float32)
    res = M.bootstrap([torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()], torch.from_numpy(labels).cuda(), cut=[0.75, 0.5],
                      replicates=replicates, seed=seed, level=level, groups=torch.from_numpy(ids).cuda())
    want = G.cluster_stats([a, b], labels == 1, ids, groups, replicates, seed, [0.75, 0.5])
    assert res.clusters == groups and np.array_equal(res.stats, want)
    plain = M.bootstrap([torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()], torch.from_numpy(labels).cuda(), cut=[0.75, 0.5],
                        replicates=replicates, seed=seed, level=level)
    assert plain.clusters is None and plain.point == res.point
    for metric in ("auc", "eer", "accuracy", "balanced_accuracy"):
        values = B.values(want, metric)
        for m in range(2):
            assert res.interval(metric, m) == B.interval(values[m], level)
        d = res.delta(metric, 0, 1)
        assert (d.lo, d.hi, d.p, d.valid) == B.delta(values[0], values[1], level) and d.point == res.point[0][metric] - res.point[1][metric]
    lo, hi = res.interval("auc", 0)
    plo, phi = plain.interval("auc", 0)
    assert hi - lo > phi - plo                                          # correlated frames: the frame bootstrap is too narrow
    with pytest.raises(ValueError):
        M.bootstrap(torch.from_numpy(a).cuda(), torch.from_numpy(labels).cuda(), groups=torch.from_numpy(ids[:-1]).cuda())
    with pytest.raises(ValueError):
        M.bootstrap(torch.from_numpy(a).cuda(), torch.from_numpy(labels).cuda(), groups=torch.from_numpy(ids - 1).cuda())


# ------------------------------------------------------------------ the jobs
FRAME_KEYS = {"model", "split", "accuracy", "timestamp", "roc_auc", "threshold", "confusion_matrix", "eer", "balanced_accuracy"}
GROUP_KEYS = FRAME_KEYS | {"unit", "pool", "groups", "singletons"}


def _spy_on_thresholds(monkeypatch, O):
    """Every _validation_threshold call as (rows of the book, result)."""
    seen, real = [], O._validation_threshold

    def spy(book):
        value = real(book)
        seen.append((book.count, value))
        return value

    monkeypatch.setattr(O, "_validation_threshold", spy)
    return seen


def test_inference_job_writes_group_records_only_when_asked(tmp_path, monkeypatch):
    """A small torch model stands in for the checkpoint: what is under test is the job around it.  Five videos of four frames and
    one loose file per class."""
    import yaml
    from PIL import Image

    from deepfakedetection_amd.orchestration import orchestrator as O

    torch.manual_seed(0)
    stand_in = torch.nn.Sequential(torch.nn.AdaptiveAvgPool2d(2), torch.nn.Flatten(), torch.nn.Linear(12, 2)).eval().cuda()
    monkeypatch.setattr(O, "load_model", lambda *args, **kwargs: stand_in)
    seen = _spy_on_thresholds(monkeypatch, O)
    rng = np.random.default_rng(5)
    videos, frames = 5, 4
    for split in ("val", "test"):
        for shade, cls in ((60, "fake"), (150, "real")):
            for v in range(videos):
                folder = tmp_path / "data" / split / cls / f"v{v}"     # the same video names under both classes
                folder.mkdir(parents=True)
                centre = shade + rng.normal(0, 60)                      # the frames of a video share its brightness
                for i in range(frames):
                    pixels = np.clip(rng.normal(centre, 30, size=(24, 24, 3)), 0, 255).astype(np.uint8)
                    Image.fromarray(pixels).save(folder / f"{i}.png")
            Image.fromarray(np.full((24, 24, 3), shade, dtype=np.uint8)).save(tmp_path / "data" / split / cls / "loose.png")
    n, groups = 2 * (videos * frames + 1), 2 * (videos + 1)
    boot = {"bootstrap": {"replicates": 300, "level": 0.9, "seed": 4}}
    by = {"group_by": {"key": "parent", "pool": "mean"}}
    rows, calls = {}, {}
    for out, extra, val_split in (("plain", {}, "val"), ("grouped", by, "val"), ("both", {**by, **boot}, "val"), ("noval", by, "absent"),
                                  ("boot", boot, "val")):
        infer = {"split": "test", "batch_size": 8, "num_workers": 0, "img_size": 32, "device_metrics": True, **extra}
        cfg = {"seed": 1, "device": "cuda",
               "data": {"root": str(tmp_path / "data"), "val_split": val_split, "test_split": "test", "num_classes": 2, "img_size": 32},
               "models": {"efficientnet_b0": {"output_dir": str(tmp_path / out), "inference": infer}}, "selection": ["efficientnet_b0"]}
        path = tmp_path / f"{out}.yaml"
        path.write_text(yaml.safe_dump(cfg))
        del seen[:]
        O.orchestrate(path, mode="inference")
        calls[out] = list(seen)
        (run,) = [p for p in (tmp_path / out).iterdir() if p.is_dir()]
        rows[out] = [json.loads(s) for s in (run / "logs" / "metrics.jsonl").read_text().splitlines()]
    (plain,) = rows["plain"]
    assert set(plain) == FRAME_KEYS and calls["plain"] == [(n, plain["threshold"])]
    strip = lambda rec, *drop: {k: v for k, v in rec.items() if k not in ("timestamp",) + drop}
    frame, group = rows["grouped"]
    assert strip(frame) == strip(plain)                                 # the frame record is today's
    assert set(group) == GROUP_KEYS and (group["unit"], group["pool"], group["groups"], group["singletons"]) == ("group", "mean", groups, 2)
    assert np.sum(group["confusion_matrix"]) == groups and (group["model"], group["split"]) == (plain["model"], plain["split"])
    assert calls["grouped"] == [(n, frame["threshold"]), (groups, group["threshold"])]       # the pooled validation pass chose it
    frame, group = rows["noval"]
    assert calls["noval"] == [] and frame["threshold"] == group["threshold"] == 0.5
    (only,) = rows["boot"]
    assert set(only) == FRAME_KEYS | {"ci", "bootstrap"} and only["bootstrap"] == {"replicates": 300, "seed": 4, "level": 0.9, "degenerate": 0}
    frame, group = rows["both"]
    assert strip(frame, "ci", "bootstrap") == strip(plain) and strip(group, "ci", "bootstrap") == strip(rows["grouped"][1])
    assert frame["bootstrap"] == {"replicates": 300, "seed": 4, "level": 0.9, "degenerate": frame["bootstrap"]["degenerate"], "cluster": True,
                                  "groups": groups}
    assert set(group["bootstrap"]) == {"replicates", "seed", "level", "degenerate"}         # the plain bootstrap over the pooled scores
    for rec in (frame, group):
        assert set(rec["ci"]) == {"roc_auc", "eer", "accuracy", "balanced_accuracy"}
        for key, (lo, hi) in rec["ci"].items():
            assert lo <= hi and lo - 1e-6 <= rec[key] <= hi + 1e-6, (key, lo, rec[key], hi)
    assert frame["ci"] != only["ci"]                                    # clusters, not frames, were drawn


def test_ensemble_job_judges_the_groups_too(tmp_path, monkeypatch):
    from deepfakedetection_amd.orchestration import orchestrator as O

    seen = _spy_on_thresholds(monkeypatch, O)
    videos, frames = 12, 5
    n, groups = 2 * videos * frames, 2 * videos
    rng = np.random.default_rng(3)
    video_of = np.repeat(np.arange(groups), frames)
    y_np = (video_of >= videos).astype(np.int64)
    y = torch.from_numpy(y_np).cuda()

    def paths(split):
        return [str(tmp_path / split / ("real" if y_np[i] else "fake") / f"v{video_of[i] % videos}" / f"{i}.png") for i in range(n)]

    def member(shift: float, group_by) -> O.MemberScores:
        settings = O.InferenceSettings(name="m", root=tmp_path, split="test", val_split="val", num_classes=2, image_size=32, batch_size=4,
                                       num_workers=0, amp=False, device=torch.device("cuda"), fp8_weights=False, transform=None,
                                       device_metrics=True, calibration=None, robustness=(), cam_limit=None, group_by=group_by)

        def logits():
            centre = rng.standard_normal(groups)[video_of]
            z = torch.from_numpy(np.stack([np.zeros(n), centre + 0.5 * rng.standard_normal(n) + shift * y_np], axis=1).astype(np.float32))
            return z.cuda()

        z, z_val = logits(), logits()
        probs = torch.softmax(z, dim=1)
        preds = (probs[:, 1] >= 0.5).long()
        record = {"accuracy": float((preds == y).float().mean()), "roc_auc": M.binary_roc(probs[:, 1], y).auc, "threshold": 0.5}
        return O.MemberScores(settings=settings, classes=["fake", "real"], paths=paths("test"), val=(z_val, y), val_paths=paths("val"),
                              clean=(z, y), preds=preds.cpu(), levels={}, temperature=None, record=record)

    rows, calls = {}, {}
    for out, group_by, boot in (("plain", None, None), ("grouped", ("parent", None, "vote"), (300, 0.9, 2))):
        rng = np.random.default_rng(3)                                  # the same members in both runs
        members = [member(2.0, group_by), member(1.0, group_by)]
        ens = O.EnsembleSettings(("a", "b"), "logit", "equal", 0.0, tmp_path / out, boot)
        run = O.ensure_run_dirs(tmp_path / out, "now")
        del seen[:]
        O.run_ensemble_job(ens, ["a", "b"], members, run)
        calls[out] = list(seen)
        rows[out] = [json.loads(s) for s in (run.logs / "metrics.jsonl").read_text().splitlines()]
    (plain,) = rows["plain"]
    frame, group = rows["grouped"]
    assert "unit" not in plain and set(frame) == set(plain) | {"ci", "bootstrap"}
    assert {k: v for k, v in frame.items() if k not in ("ci", "bootstrap", "timestamp")} == {k: v for k, v in plain.items() if k != "timestamp"}
    assert frame["bootstrap"]["cluster"] is True and frame["bootstrap"]["groups"] == groups
    assert (group["unit"], group["pool"], group["groups"], group["singletons"], group["model"]) == ("group", "vote", groups, 0, "ensemble")
    assert "cluster" not in group["bootstrap"] and np.sum(group["confusion_matrix"]) == groups
    assert calls["plain"] == [(n, plain["threshold"])] and calls["grouped"] == [(n, frame["threshold"]), (groups, group["threshold"])]
