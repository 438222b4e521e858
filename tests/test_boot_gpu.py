"""The bootstrap kernels (csrc/dfd_boot.hip through kernels.boot_counts / boot_stats and deepfakedetection_amd.metrics.bootstrap)
against the reference of tests/_boot_ref.py, which expands every resample and judges the expansion with tests/_metrics_ref.py.
Every comparison is == on integers, or on floats derived from equal integers.  Every output is an interior slice of a buffer filled
with the canary -1, and the canaries around it must survive."""

from __future__ import annotations

import json

import numpy as np
import pytest
import torch

from deepfakedetection_amd import kernels as K
from deepfakedetection_amd import metrics as M
from tests import _boot_ref as B

pytestmark = pytest.mark.gpu

GUARD = 32
EDGE = K.BOOT_LDS_MAX_N
HIGH_SEED = (0x9E3779B9 << 32) | 7


def _guarded(shape, dtype):
    count = int(np.prod(shape))
    big = torch.full((count + 2 * GUARD,), -1, dtype=dtype, device="cuda")
    return big, big[GUARD:GUARD + count].view(*shape)


def _intact(big: torch.Tensor) -> bool:
    host = big.cpu()
    return bool((host[:GUARD] == -1).all() and (host[-GUARD:] == -1).all())


def _case(n: int, kind: str, seed: int = 0, min_per_class: int = 32):
    """(scores f32 [n], labels int64 [n]) in a random sample order: `grid` = five score values (heavy ties), `equal` = one value,
    `distinct` = no ties.  With n >= 2 * min_per_class both classes have at least min_per_class samples."""
    rng = np.random.default_rng(seed * 1000 + n)
    labels = rng.integers(0, 2, size=n).astype(np.int64)
    if n >= 2 * min_per_class:
        labels[:min_per_class], labels[min_per_class:2 * min_per_class] = 1, 0
    if kind == "grid":
        scores = np.clip(rng.integers(0, 5, size=n) + (labels == 1), 0, 4) / 4.0
    elif kind == "equal":
        scores = np.full(n, 0.25)
    else:
        scores = (2 * rng.permutation(n) + (2 * (n // 4) + 1) * labels) / (2.5 * n + 2.0)     # even / odd numerators: no two are equal
        assert np.unique(scores.astype(np.float32)).size == n
    order = rng.permutation(n)
    return scores.astype(np.float32)[order], labels[order]


def _run(members, labels, replicates, seed=0, cuts=None, hit=None, ws_bytes=None):
    """kernels.boot_stats on the members' unsorted scores -> int64 [M, B, 10] on the host, after the canary check."""
    ordered, perms = [], []
    for m in members:
        s, order = torch.sort(torch.from_numpy(m).cuda())
        ordered.append(s.contiguous())
        perms.append(order.to(torch.int32).contiguous())
    is_pos = torch.from_numpy((labels == 1).astype(np.uint8)).cuda()
    hit_d = torch.from_numpy(np.asarray(hit, dtype=np.uint8)).cuda() if hit is not None else None
    big, out = _guarded((len(members), replicates, K.BOOT_STATS_LEN), torch.int64)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda") if ws_bytes is not None else None
    got = K.boot_stats(ordered, perms, is_pos, replicates, seed, cuts, hit_d, ws=ws, out=out)
    torch.cuda.synchronize()
    assert got is out and _intact(big), "a write outside stats"
    return out.cpu().numpy()


# ------------------------------------------------------------------ the draw
@pytest.mark.parametrize("seed", [0, 1, HIGH_SEED])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 64, 65, 4097])
def test_boot_counts_equal_the_reference_histogram(n, seed):
    for R_ in (1, 3):
        for b0 in (0, 7):
            big, out = _guarded((R_, n), torch.int32)
            K.boot_counts(n, b0, R_, seed, "cuda", out=out)
            torch.cuda.synchronize()
            assert _intact(big)
            got = out.cpu().numpy().astype(np.int64)
            assert np.array_equal(got, B.counts(n, b0, R_, seed)), (n, R_, b0, seed)
            assert (got.sum(axis=1) == n).all()


def test_a_different_seed_or_resample_gives_different_counts():
    base = K.boot_counts(4097, 0, 2, 0, "cuda").cpu()
    assert not torch.equal(base[0], base[1])
    assert not torch.equal(base, K.boot_counts(4097, 0, 2, 1, "cuda").cpu())
    assert not torch.equal(base, K.boot_counts(4097, 0, 2, 1 << 32, "cuda").cpu())
    assert torch.equal(base, K.boot_counts(4097, 0, 2, 0, "cuda").cpu())
    assert torch.equal(base[1:], K.boot_counts(4097, 1, 1, 0, "cuda").cpu())


# ------------------------------------------------------------------ the statistics
def _cuts_for(scores_list, mode):
    if mode == "none":
        return None
    if mode == "score":
        return [float(np.sort(s)[s.size // 2]) for s in scores_list]
    return [{"below": -1.0, "above": 2.0}[mode]] * len(scores_list)


@pytest.mark.parametrize("kind", ["grid", "equal", "distinct"])
@pytest.mark.parametrize("n", [1, 2, 5, 64, 65, 2049])
def test_boot_stats_small_sizes(n, kind):
    """Every B and M, with and without cut and hit, in the LDS tier.  From n = 64 on both classes have 32 samples and no resample
    may lose one."""
    rng = np.random.default_rng(n)
    for replicates, count, cut_mode, with_hit in ((1, 1, "none", False), (2, 3, "score", True), (65, 1, "score", False), (65, 3, "below", True),
                                                  (2, 1, "above", True)):
        if n == 2049 and replicates == 65 and count == 3:
            replicates = 9                                              # the reference expands every (resample, member)
        cases = [_case(n, kind, seed=k) for k in range(count)]
        labels = cases[0][1]
        members = [c[0] for c in cases]
        cuts = _cuts_for(members, cut_mode)
        hit = rng.integers(0, 2, size=n).astype(np.uint8) if with_hit else None
        assert K.boot_plan(n, replicates, count).tier == K.BOOT_TIER_LDS
        got = _run(members, labels, replicates, seed=n + 1, cuts=cuts, hit=hit)
        want = B.stats(members, labels == 1, replicates, n + 1, cuts, hit)
        assert np.array_equal(got, want), (n, kind, replicates, count, cut_mode, np.argwhere(got != want)[:5])
        assert (got[..., 0] + got[..., 1] == n).all()
        if n >= 64:
            res = M.BootstrapResult(got, replicates, n + 1, 0.95, [])
            assert all(res.degenerate(m) == 0 for m in range(count))


@pytest.mark.parametrize("n,tier", [(EDGE, K.BOOT_TIER_LDS), (EDGE + 1, K.BOOT_TIER_GLOBAL)])
def test_boot_stats_on_both_sides_of_the_tier_boundary(n, tier):
    cases = [_case(n, kind, seed=k) for k, kind in enumerate(("grid", "distinct", "equal"))]
    labels, members = cases[0][1], [c[0] for c in cases]
    hit = (np.arange(n) % 3 == 0).astype(np.uint8)
    cuts = _cuts_for(members, "score")
    plan = K.boot_plan(n, 2, 3)
    assert plan.tier == tier and plan.per_pass == 2 and plan.passes == 1
    got = _run(members, labels, 2, seed=HIGH_SEED, cuts=cuts, hit=hit)
    want = B.stats(members, labels == 1, 2, HIGH_SEED, cuts, hit)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    res = M.BootstrapResult(got, 2, HIGH_SEED, 0.95, [])
    assert all(res.degenerate(m) == 0 for m in range(3))
    for replicates, member in ((1, members[1]), (65, members[0])):      # M = 1 at B = 1 (no ties) and at B = 65 (five tie groups)
        assert K.boot_plan(n, replicates, 1).tier == tier
        got = _run([member], labels, replicates, seed=6, cuts=[0.5])
        assert np.array_equal(got, B.stats([member], labels == 1, replicates, 6, [0.5]))


def test_global_tier_passes_give_the_bits_of_one_pass():
    """B = 65 in the global tier with a workspace for all 65 resamples, for 3 (22 passes, the last one partial) and for 1."""
    n, replicates = EDGE + 1, 65
    (scores, labels), (other, _) = _case(n, "grid", 3), _case(n, "distinct", 4)
    cut = [0.5, float(np.median(other))]
    hit = (np.arange(n) % 2).astype(np.uint8)
    full = _run([scores, other], labels, replicates, seed=5, cuts=cut, hit=hit, ws_bytes=K.boot_ws(n, replicates))
    assert K.boot_plan(n, replicates, 2, K.boot_ws(n, replicates)) == K.BootPlan(K.BOOT_TIER_GLOBAL, 65, 1, (n + 4095) // 4096)
    for per_pass, passes in ((3, 22), (1, 65)):
        assert K.boot_plan(n, replicates, 2, 4 * n * per_pass) == K.BootPlan(K.BOOT_TIER_GLOBAL, per_pass, passes, (n + 4095) // 4096)
        assert np.array_equal(_run([scores, other], labels, replicates, seed=5, cuts=cut, hit=hit, ws_bytes=4 * n * per_pass), full)
    default = _run([scores, other], labels, replicates, seed=5, cuts=cut, hit=hit)
    assert np.array_equal(default, full)
    for b in (0, 1, 64):                                                # the first, one inside the first pass of three, the last
        c = B.counts(n, b, 1, 5)[0]
        for m, member in enumerate((scores, other)):
            assert full[m, b].tolist() == B.resample_stats(member, labels == 1, c, cut[m], hit), (m, b)
    with pytest.raises(ValueError):
        _run([scores], labels, 2, ws_bytes=4 * n - 1)


# ------------------------------------------------------------------ degenerate inputs
@pytest.mark.parametrize("n", [65, EDGE + 1])
@pytest.mark.parametrize("label", [0, 1])
def test_one_class_only(n, label):
    scores, _ = _case(n, "grid")
    labels = np.full(n, label, dtype=np.int64)
    replicates = 3
    hit = (np.arange(n) % 4 == 0).astype(np.uint8)
    got = _run([scores], labels, replicates, seed=2, cuts=[0.5], hit=hit)
    want = B.stats([scores], labels == 1, replicates, 2, [0.5], hit)
    assert np.array_equal(got, want)
    assert (got[0, :, 1 - label] == n).all() and (got[0, :, label] == 0).all() and (got[0, :, 2] == 0).all() and (got[0, :, 6:] == 0).all()
    res = M.BootstrapResult(got, replicates, 2, 0.95, [])
    assert res.degenerate(0) == replicates
    for metric in M.BOOT_METRICS:
        values = res.values(metric)
        assert np.isnan(values).all() == (metric != "hit_rate") and np.array_equal(values, B.values(got, metric), equal_nan=True)
        assert (res.interval(metric) is None) == (metric != "hit_rate")


def test_two_samples_one_of_each():
    scores, labels = np.array([0.25, 0.75], dtype=np.float32), np.array([1, 0], dtype=np.int64)
    got = _run([scores, -scores], labels, 65, seed=9, cuts=[0.5, -0.5])
    want = B.stats([scores, -scores], labels == 1, 65, 9, [0.5, -0.5])
    assert np.array_equal(got, want)
    seen = {tuple(row[:2]) for row in got[0].tolist()}
    assert seen == {(0, 2), (1, 1), (2, 0)}                             # 65 resamples of two samples meet all three
    res = M.BootstrapResult(got, 65, 9, 0.95, [])
    assert res.degenerate(0) == sum(1 for row in got[0].tolist() if row[0] != 1)
    both = got[0, :, 0] == 1
    assert (res.values("auc")[0][both] == 0.0).all() and (res.values("auc")[1][both] == 1.0).all()
    assert (res.values("eer")[0][both] == 1.0).all() and (res.values("eer")[1][both] == 0.0).all()


# ------------------------------------------------------------------ structure
@pytest.mark.parametrize("n", [2049, EDGE + 1])
def test_structure_of_the_rows(n):
    scores, labels = _case(n, "grid", 7)
    other, _ = _case(n, "distinct", 8)
    replicates = 5
    got = _run([scores, scores.copy(), -scores, other], labels, replicates, seed=3, cuts=[0.5, 0.5, None, None])
    assert np.array_equal(got[0], got[1])                               # identical members, identical rows
    P, N = got[0, :, 0], got[0, :, 1]
    assert np.array_equal(got[2, :, 2], 2 * P * N - got[0, :, 2])       # negated scores reflect the rank statistic
    assert np.array_equal(got[2, :, :2], got[0, :, :2]) and np.array_equal(got[3, :, :2], got[0, :, :2])     # shared resamples
    assert (got[2:, :, 3:6] == 0).all()                                 # no cut, no hit
    again = _run([scores, scores.copy(), -scores, other], labels, replicates, seed=3, cuts=[0.5, 0.5, None, None])
    assert np.array_equal(got, again)
    reseeded = _run([scores], labels, replicates, seed=4, cuts=[0.5])
    assert not np.array_equal(reseeded[0], got[0])
    counts = K.boot_counts(n, 0, replicates, 3, "cuda").cpu().numpy().astype(np.int64)         # both tiers draw what boot_counts draws
    assert np.array_equal(counts @ (labels == 1).astype(np.int64), P)


# ------------------------------------------------------------------ metrics.bootstrap
def test_bootstrap_end_to_end_against_the_reference():
    n, replicates, seed, level = 300, 200, 12, 0.9
    rng = np.random.default_rng(1)
    labels = (np.arange(n) % 5 == 0).astype(np.int64)[rng.permutation(n)]
    a = (np.round(rng.standard_normal(n) * 8) / 8 + 1.5 * labels).astype(np.float32)
    b = (rng.standard_normal(n) + 0.8 * labels).astype(np.float32)
    hits = (a >= 0.75) == (labels == 1)
    res = M.bootstrap([torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()], torch.from_numpy(labels).cuda(), cut=[0.75, 0.5],
                      hits=torch.from_numpy(hits).cuda(), replicates=replicates, seed=seed, level=level)
    want = B.stats([a, b], labels == 1, replicates, seed, [0.75, 0.5], hits)
    assert res.stats.dtype == np.int64 and np.array_equal(res.stats, want)
    assert (res.replicates, res.seed, res.level) == (replicates, seed, level) and res.degenerate(0) == res.degenerate(1) == 0
    full = np.ones(n, dtype=np.int64)
    for m, (scores, cut) in enumerate(((a, 0.75), (b, 0.5))):
        point = B.resample_stats(scores, labels == 1, full, cut, hits)
        for metric in M.BOOT_METRICS:
            assert res.point[m][metric] == B.value(point, metric), (m, metric)
    for metric in M.BOOT_METRICS:
        values = B.values(want, metric)
        assert np.array_equal(res.values(metric), values), metric
        for m in range(2):
            lo, hi = res.interval(metric, m)
            assert (lo, hi) == B.interval(values[m], level) and lo <= hi
        d = res.delta(metric, 0, 1)
        assert (d.lo, d.hi, d.p, d.valid) == B.delta(values[0], values[1], level) and d.point == res.point[0][metric] - res.point[1][metric]
    assert res.values("accuracy")[0].tolist() == res.values("hit_rate")[0].tolist()          # the hits are member 0's right predictions
    lo, hi = res.interval("auc", 0)
    assert lo < res.point[0]["auc"] < hi and res.delta("auc", 0, 1).lo > 0 and res.delta("auc", 0, 1).p < 0.05
    single = M.bootstrap(torch.from_numpy(a).cuda(), torch.from_numpy(labels).cuda(), cut=0.75, replicates=replicates, seed=seed, level=level)
    assert np.array_equal(single.stats[0, :, [0, 1, 2, 3, 4, 6, 7, 8, 9]], res.stats[0, :, [0, 1, 2, 3, 4, 6, 7, 8, 9]]) and (single.stats[0, :, 5] == 0).all()
    assert single.point[0]["hit_rate"] is None
    with pytest.raises(ValueError, match="NaN or infinite"):
        M.bootstrap(torch.tensor([0.1, float("nan"), 0.3], device="cuda"), torch.tensor([0, 1, 1], device="cuda"))


# ------------------------------------------------------------------ the ensemble job
def test_ensemble_job_compares_the_ensemble_with_its_members(tmp_path):
    from deepfakedetection_amd.orchestration import orchestrator as O

    n = 240
    rng = np.random.default_rng(3)
    y = torch.from_numpy((np.arange(n) % 3 == 0).astype(np.int64)).cuda()
    settings = O.InferenceSettings(name="m", root=tmp_path, split="test", val_split="val", num_classes=2, image_size=32, batch_size=4,
                                   num_workers=0, amp=False, device=torch.device("cuda"), fp8_weights=False, transform=None,
                                   device_metrics=True, calibration=None, robustness=(), cam_limit=None)

    def member(shift: float) -> O.MemberScores:
        z = torch.from_numpy(rng.standard_normal((n, 2)).astype(np.float32)).cuda()
        z[:, 1] += shift * y
        probs = torch.softmax(z, dim=1)
        roc = M.binary_roc(probs[:, 1], y)
        preds = (probs[:, 1] >= 0.5).long()
        record = {"accuracy": float((preds == y).float().mean()), "roc_auc": roc.auc, "threshold": 0.5}
        return O.MemberScores(settings=settings, classes=["fake", "real"], paths=[str(i) for i in range(n)], val=None, val_paths=[],
                              clean=(z, y), preds=preds.cpu(), levels={}, temperature=None, record=record)

    members = [member(2.0), member(1.0)]
    docs, rows = {}, {}
    for out, boot in (("plain", None), ("boot", (300, 0.9, 2))):
        ens = O.EnsembleSettings(("a", "b"), "logit", "equal", 0.0, tmp_path / out, boot)
        paths = O.ensure_run_dirs(tmp_path / out, "now")
        O.run_ensemble_job(ens, ["a", "b"], members, paths)
        docs[out] = json.loads((paths.run_dir / "ensemble.json").read_text())
        rows[out] = [json.loads(s) for s in (paths.logs / "metrics.jsonl").read_text().splitlines()]
    assert "vs_members" not in docs["plain"] and set(docs["boot"]) == set(docs["plain"]) | {"vs_members"}
    assert {k: v for k, v in docs["boot"].items() if k != "vs_members"} == docs["plain"]
    (plain,), (boot,) = rows["plain"], rows["boot"]
    assert set(boot) == set(plain) | {"ci", "bootstrap"} and boot["bootstrap"] == {"replicates": 300, "seed": 2, "level": 0.9, "degenerate": 0}
    for key, (lo, hi) in boot["ci"].items():
        assert lo <= hi and lo - 1e-6 <= boot[key] <= hi + 1e-6, (key, lo, boot[key], hi)
    versus = docs["boot"]["vs_members"]
    assert set(versus) == {"a", "b"}
    for name in ("a", "b"):
        assert set(versus[name]) == {"auc", "accuracy"}
        for metric, d in versus[name].items():
            assert set(d) == {"metric", "point", "lo", "hi", "p", "valid"} and d["metric"] == metric and d["valid"] == 300
            assert d["lo"] <= d["hi"] and 0.0 < d["p"] <= 1.0
        assert versus[name]["auc"]["point"] == docs["boot"]["clean"]["ensemble"]["roc_auc"] - docs["boot"]["clean"][name]["roc_auc"]
    assert versus["b"]["auc"]["lo"] > 0 and versus["b"]["auc"]["p"] < 0.05          # the ensemble beats its weak member beyond the noise


# ------------------------------------------------------------------ the inference job
def test_inference_job_writes_intervals_only_when_asked(tmp_path, monkeypatch):
    """A small torch model stands in for the checkpoint: what is under test is the job around it."""
    import yaml
    from PIL import Image

    from deepfakedetection_amd.orchestration import orchestrator as O

    torch.manual_seed(0)
    stand_in = torch.nn.Sequential(torch.nn.AdaptiveAvgPool2d(2), torch.nn.Flatten(), torch.nn.Linear(12, 2)).eval().cuda()
    monkeypatch.setattr(O, "load_model", lambda *args, **kwargs: stand_in)
    rng = np.random.default_rng(5)
    for split in ("val", "test"):
        for shade, cls in ((60, "fake"), (150, "real")):                # overlapping brightness: neither perfect nor chance
            folder = tmp_path / "data" / split / cls
            folder.mkdir(parents=True)
            for i in range(12):
                pixels = np.clip(rng.normal(shade + rng.normal(0, 60), 30, size=(24, 24, 3)), 0, 255).astype(np.uint8)
                Image.fromarray(pixels).save(folder / f"{cls}_{i}.png")
    rows = {}
    for out, extra in (("plain", {}), ("boot", {"bootstrap": {"replicates": 300, "level": 0.9, "seed": 4}})):
        infer = {"split": "test", "batch_size": 8, "num_workers": 0, "img_size": 32, "device_metrics": True, **extra}
        cfg = {"seed": 1, "device": "cuda",
               "data": {"root": str(tmp_path / "data"), "val_split": "val", "test_split": "test", "num_classes": 2, "img_size": 32},
               "models": {"efficientnet_b0": {"output_dir": str(tmp_path / out), "inference": infer}}, "selection": ["efficientnet_b0"]}
        path = tmp_path / f"{out}.yaml"
        path.write_text(yaml.safe_dump(cfg))
        O.orchestrate(path, mode="inference")
        (run,) = [p for p in (tmp_path / out).iterdir() if p.is_dir()]
        rows[out] = [json.loads(s) for s in (run / "logs" / "metrics.jsonl").read_text().splitlines()]
    (plain,), (boot,) = rows["plain"], rows["boot"]
    assert set(plain) == {"model", "split", "accuracy", "timestamp", "roc_auc", "threshold", "confusion_matrix", "eer", "balanced_accuracy"}
    assert set(boot) == set(plain) | {"ci", "bootstrap"}
    assert {k: v for k, v in boot.items() if k not in ("ci", "bootstrap", "timestamp")} == {k: v for k, v in plain.items() if k != "timestamp"}
    assert boot["bootstrap"] == {"replicates": 300, "seed": 4, "level": 0.9, "degenerate": 0}
    assert set(boot["ci"]) == {"roc_auc", "eer", "accuracy", "balanced_accuracy"}
    for key, (lo, hi) in boot["ci"].items():
        # (the record's accuracy is a float32 mean: it may sit one float32 rounding off the exact ratio the interval is made of)
        assert lo <= hi and lo - 1e-6 <= boot[key] <= hi + 1e-6, (key, lo, boot[key], hi)
