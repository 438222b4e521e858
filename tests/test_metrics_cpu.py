"""No-GPU checks of the evaluation metrics: the numpy / integer reference (tests/_metrics_ref.py) against brute force, sklearn
and scipy; the host half of deepfakedetection_amd.metrics (EER, best threshold, ScoreBook, gather_scores under gloo); the config
switches; and the argument checks of the new entry points."""

from __future__ import annotations

import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from deepfakedetection_amd import _lib
from deepfakedetection_amd import metrics as M
from tests import _metrics_ref as R


def _case(seed: int, n: int, grid: int | None = 50, p_pos: float = 0.3):
    """n f32 scores (from `grid` values, so ties are everywhere; None: continuous) and 0/1 labels."""
    rng = np.random.default_rng(seed)
    labels = (rng.random(n) < p_pos).astype(np.int64)
    raw = rng.normal(size=n) + 0.8 * labels
    scores = 1.0 / (1.0 + np.exp(-raw))
    if grid is not None:
        scores = np.round(scores * (grid - 1)) / (grid - 1)
    return scores.astype(np.float32), labels


def _brute_two_u(scores, labels, positive=1) -> int:
    total = 0
    for s, l in zip(scores.tolist(), labels.tolist()):
        if l != positive:
            continue
        for t, m in zip(scores.tolist(), labels.tolist()):
            if m != positive:
                total += 2 if t < s else (1 if t == s else 0)
    return total


@pytest.mark.parametrize("n,grid", [(1, 50), (2, 50), (17, 5), (100, 50), (300, 50), (300, None), (257, 2)])
def test_reference_equals_brute_force(n, grid):
    scores, labels = _case(n, n, grid)
    want = _brute_two_u(scores, labels)
    assert R.two_u(scores, labels) == want == R.two_u_by_groups(scores, labels)
    thr, cum_pos, cum_neg, stats = R.groups(scores, labels)
    assert stats == [int(labels.sum()), int(n - labels.sum()), len(np.unique(scores)), 0, want]
    assert np.array_equal(thr, np.unique(scores)) and cum_pos[-1] == stats[0] and cum_neg[-1] == stats[1]
    fps, tps, thresholds = R.roc_counts(scores, labels)
    for f, t, cut in zip(fps.tolist(), tps.tolist(), thresholds.tolist()):
        assert t == int(((scores >= np.float32(cut)) & (labels == 1)).sum()) and f == int(((scores >= np.float32(cut)) & (labels == 0)).sum())
    cuts = np.linspace(0.0, 1.0, 501)
    tp, fp = R.sweep(scores, labels, cuts)
    pred = scores[None, :] >= cuts[:, None]                         # numpy promotes the float32 scores to float64
    assert np.array_equal(tp, (pred & (labels == 1)[None]).sum(1)) and np.array_equal(fp, (pred & (labels == 0)[None]).sum(1))


def test_reference_with_three_classes_and_another_positive():
    rng = np.random.default_rng(3)
    scores = (rng.integers(0, 20, size=200) / 19).astype(np.float32)
    labels = rng.integers(0, 3, size=200).astype(np.int64)
    for positive in (0, 2):
        assert R.two_u(scores, labels, positive) == _brute_two_u(scores, labels, positive) == R.groups(scores, labels, positive)[3][4]


@pytest.mark.parametrize("n,grid", [(50, 7), (500, 50), (2000, 50), (2000, None)])
def test_reference_equals_sklearn(n, grid):
    sk = pytest.importorskip("sklearn.metrics")
    scores, labels = _case(100 + n, n, grid)
    # the trapezoid sums at most n f64 terms: n * 2^-52 < 1e-12 for n <= 2000
    assert abs(R.auc(scores, labels) - sk.roc_auc_score(labels, scores)) < 1e-12
    fpr, tpr, thresholds = sk.roc_curve(labels, scores, drop_intermediate=False)
    fps, tps, thr = R.roc_counts(scores, labels)
    assert np.array_equal(thr, thresholds[1:])
    assert np.array_equal(fps / fps[-1], fpr[1:]) and np.array_equal(tps / tps[-1], tpr[1:])
    assert fps[-1] == int((labels == 0).sum()) and tps[-1] == int((labels == 1).sum())


def test_best_threshold_equals_the_orchestrators_with_ties_at_the_maximum():
    from deepfakedetection_amd.orchestration.orchestrator import best_balanced_accuracy_threshold

    cuts = np.linspace(0.0, 1.0, 501)
    # two clusters far apart: every cut between them has balanced accuracy 1, the first of them wins
    scores = np.asarray([0.1, 0.1, 0.12, 0.2, 0.8, 0.8, 0.9, 0.95], dtype=np.float32)
    labels = np.asarray([0, 0, 0, 0, 1, 1, 1, 1], dtype=np.int64)
    want = best_balanced_accuracy_threshold(scores, labels)
    assert R.best_threshold(scores, labels, cuts) == want and 0.2 < want <= 0.202 + 1e-12
    for seed in range(6):
        scores, labels = _case(seed, 400, grid=11)
        want = best_balanced_accuracy_threshold(scores, labels)
        assert R.best_threshold(scores, labels, cuts) == want
        tp, fp = R.sweep(scores, labels, cuts)
        res = M.RocResult(auc=None, two_u=0, n_pos=int(labels.sum()), n_neg=int((labels == 0).sum()), groups=0, nonfinite=0,
                          cuts=cuts, tp=tp, fp=fp)
        assert res.best_balanced_accuracy_threshold() == want


def _eer_both(scores, labels):
    fps, tps, _ = R.roc_counts(scores, labels)
    got = M.eer_from_curve(fps, tps, int((labels == 1).sum()), int((labels == 0).sum()))
    want = R.eer(scores, labels)
    assert abs(got - want) < 1e-12            # a handful of f64 roundings of values <= 1 against the rational rounded once
    return want


def test_eer_on_hand_worked_cases():
    labels = np.asarray([0, 0, 1, 1], dtype=np.int64)
    assert _eer_both(np.asarray([0.1, 0.2, 0.8, 0.9], dtype=np.float32), labels) == 0.0              # perfect separation
    assert _eer_both(np.full(4, 0.5, dtype=np.float32), labels) == 0.5                               # one point: the diagonal
    # scores 0.9 (+), 0.7 (-), 0.6 (+), 0.2 (-): the curve is (0,0) (0,.5) (.5,.5) (.5,1) (1,1); fpr + tpr - 1 is -.5 at the second
    # point and 0 at the third, so the crossing is that vertex: fpr = 0.5 = 1 - tpr
    assert _eer_both(np.asarray([0.9, 0.7, 0.6, 0.2], dtype=np.float32), np.asarray([1, 0, 1, 0], dtype=np.int64)) == 0.5
    # a tie of one positive and one negative at the top: (0,0) (.5,.5) ...: the crossing is at the first vertex again
    assert _eer_both(np.asarray([0.9, 0.9, 0.3, 0.1], dtype=np.float32), np.asarray([1, 0, 1, 0], dtype=np.int64)) == 0.5
    # three negatives, one positive tied with the middle negative: (0,0) (1/3,0) (2/3,1) (1,1); fpr + tpr - 1 runs -2/3 -> 2/3 on
    # the second segment, crossing in its middle: fpr = 1/2
    assert abs(_eer_both(np.asarray([0.9, 0.5, 0.5, 0.1], dtype=np.float32), np.asarray([0, 0, 1, 0], dtype=np.int64)) - 0.5) < 1e-15
    assert M.eer_from_curve(np.asarray([3]), np.asarray([0]), 0, 3) is None and R.eer(np.ones(3, np.float32), np.zeros(3, np.int64)) is None


def test_eer_equals_scipys_root():
    opt, interp = pytest.importorskip("scipy.optimize"), pytest.importorskip("scipy.interpolate")
    for seed, grid in ((40, None), (41, None), (42, 50), (43, 11), (44, None)):
        scores, labels = _case(seed, 600, grid)
        fps, tps, _ = R.roc_counts(scores, labels)
        fpr, tpr = np.concatenate([[0.0], fps / fps[-1]]), np.concatenate([[0.0], tps / tps[-1]])
        # (fpr ascends with repeats where the curve rises vertically; assume_sorted keeps the points in curve order.  Where the
        # anti-diagonal crosses such a rise the function jumps through zero there and brentq closes in on the jump: the same fpr)
        curve = interp.interp1d(fpr, tpr, assume_sorted=True)
        want = opt.brentq(lambda x: 1.0 - x - float(curve(x)), 0.0, 1.0, xtol=1e-13)
        assert abs(_eer_both(scores, labels) - want) < 1e-9


def test_score_book_appends_at_host_offsets_and_overflows_loudly():
    book = M.ScoreBook(5, 2, "cpu")
    probs = torch.rand(3, 2)
    book.append(probs, torch.tensor([0, 1, 1]), torch.tensor([1, 1, 0]))
    book.append(probs[:2], None, torch.tensor([0, 0]))
    assert book.count == 5 and torch.equal(book.probs[:3], probs) and torch.equal(book.probs[3:], probs[:2])
    assert book.targets.tolist() == [1, 1, 0, 0, 0] and book.preds[:3].tolist() == [0, 1, 1]
    with pytest.raises(ValueError, match="overflow"):
        book.append(probs[:1], None, torch.tensor([0]))
    book.reset()
    assert book.count == 0 and book.probs.shape == (0, 2)
    with pytest.raises(ValueError, match="shape"):
        book.append(torch.rand(2, 3), None, torch.tensor([0, 0]))


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _gather_worker(rank: int, world: int, port: int, out_dir: str) -> None:
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        # unequal counts: 3 rows on rank 0 and 5 on rank 1, then 4 and none
        for trip, counts in enumerate(((3, 5), (4, 0))):
            n = counts[rank]
            scores = torch.arange(n * 2, dtype=torch.float32).reshape(n, 2) + 100 * rank
            labels = torch.arange(n, dtype=torch.int64) + 10 * rank
            got_s, got_l = M.gather_scores(scores, labels)
            torch.save((got_s, got_l), os.path.join(out_dir, f"trip{trip}_rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_gather_scores_two_gloo_ranks_of_unequal_counts(tmp_path):
    mp.spawn(_gather_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    for trip, counts in enumerate(((3, 5), (4, 0))):
        want_s = torch.cat([torch.arange(n * 2, dtype=torch.float32).reshape(n, 2) + 100 * r for r, n in enumerate(counts)])
        want_l = torch.cat([torch.arange(n, dtype=torch.int64) + 10 * r for r, n in enumerate(counts)])
        for rank in range(2):
            got_s, got_l = torch.load(tmp_path / f"trip{trip}_rank{rank}.pt")
            assert torch.equal(got_s, want_s) and torch.equal(got_l, want_l), (trip, rank)


def test_gather_scores_is_the_identity_without_a_process_group():
    scores, labels = torch.rand(4), torch.arange(4)
    got = M.gather_scores(scores, labels)
    assert got[0] is scores and got[1] is labels


def test_config_keys_parse_and_both_switches_default_to_off(tmp_path, monkeypatch):
    from deepfakedetection_amd.orchestration.orchestrator import RunPaths, build_env_overrides
    from deepfakedetection_amd.trainers import _engine

    for var in ("VAL_AUC", "SELECT_METRIC"):
        monkeypatch.delenv(var, raising=False)
    assert _engine.metric_settings() == _engine.MetricSettings(val_auc=False, select="acc")
    run_paths = RunPaths(*(tmp_path / n for n in ("run", "checkpoints", "logs", "plots")))
    model_cfg = {"name": "efficientnet_b0", "output_dir": str(tmp_path / "runs"), "training": {}}
    env = build_env_overrides(config={}, model_cfg=model_cfg, run_paths=run_paths, training=True)
    assert "VAL_AUC" not in env and "SELECT_METRIC" not in env
    model_cfg["training"] = {"val_auc": True, "select_metric": "auc"}
    env = build_env_overrides(config={}, model_cfg=model_cfg, run_paths=run_paths, training=True)
    assert env["VAL_AUC"] == "True" and env["SELECT_METRIC"] == "auc"
    monkeypatch.setenv("VAL_AUC", env["VAL_AUC"])
    assert _engine.metric_settings() == _engine.MetricSettings(val_auc=True, select="acc")
    monkeypatch.delenv("VAL_AUC")
    monkeypatch.setenv("SELECT_METRIC", "auc")
    assert _engine.metric_settings() == _engine.MetricSettings(val_auc=True, select="auc")          # selecting by AUC computes it
    monkeypatch.setenv("SELECT_METRIC", "f1")
    with pytest.raises(ValueError, match="SELECT_METRIC"):
        _engine.metric_settings()
    assert _engine.EvalResult(acc=0.5, total=2, correct=1).auc is None
    import inspect

    assert "metric_settings()" in inspect.getsource(_engine.run)


def test_selection_follows_the_chosen_metric():
    from deepfakedetection_amd.trainers._engine import EvalResult, improves, selection_value

    a = EvalResult(acc=0.80, total=10, correct=8, auc=0.70)
    b = EvalResult(acc=0.70, total=10, correct=7, auc=0.90)
    assert improves(selection_value(a, "acc"), selection_value(b, "acc")) and not improves(selection_value(b, "acc"), selection_value(a, "acc"))
    assert improves(selection_value(b, "auc"), selection_value(a, "auc")) and not improves(selection_value(a, "auc"), selection_value(b, "auc"))
    for bad in (None, float("nan")):
        assert not improves(selection_value(EvalResult(acc=0.99, total=10, correct=9, auc=bad), "auc"), -1.0)
    assert not improves(0.70005, 0.7) and improves(0.7002, 0.7)                                      # today's 1e-4 margin


def test_inference_switch_defaults_to_off_and_warns_off_device():
    import io

    from rich.console import Console

    from deepfakedetection_amd.orchestration import orchestrator as O

    config = {"device": "cpu", "data": {"root": "data", "num_classes": 2}}
    for infer, want_warning in (({}, False), ({"device_metrics": False}, False), ({"device_metrics": True}, True)):
        text = io.StringIO()
        settings = O.inference_settings(config, {"name": "efficientnet_b0", "inference": infer}, Console(file=text, width=200))
        assert settings.device_metrics is False and settings.device == torch.device("cpu")
        assert ("inference.device_metrics ignored" in text.getvalue()) == want_warning


@pytest.fixture(scope="module")
def lib():
    if not _lib.LIB_PATH.exists():
        from deepfakedetection_amd.build import build

        build()
    return _lib.load()


def test_abi_and_sources(lib):
    from deepfakedetection_amd.build import SOURCES

    assert lib.dfd_version() >= 146 and "dfd_metrics.hip" in SOURCES
    header = (_lib.LIB_PATH.parents[1] / "include" / "dfd_hip.h").read_text()
    for name, value in (("DFD_ROC_TILE", _lib.ROC_TILE), ("DFD_ROC_SCAN_WIDTH", _lib.ROC_SCAN_WIDTH), ("DFD_ROC_MAX_CUTS", _lib.ROC_MAX_CUTS),
                        ("DFD_ROC_STATS_LEN", _lib.ROC_STATS_LEN), ("DFD_CONFUSION_LDS_MAX_J", _lib.CONFUSION_LDS_MAX_J),
                        ("DFD_CONFUSION_MAX_J", _lib.CONFUSION_MAX_J)):
        assert f"#define {name} {value}\n" in header, name
    assert "#define DFD_ROC_MAX_N (1 << 28)" in header and _lib.ROC_MAX_N == 1 << 28
    assert _lib.CONFUSION_LDS_MAX_J ** 2 * 4 <= 64 * 1024 < (_lib.CONFUSION_LDS_MAX_J + 1) ** 2 * 4     # the LDS tier's budget


def test_bad_arguments_are_rejected_without_a_gpu(lib):
    EINVAL = -1
    one = 0x1000                                                    # a non-null address: rejected calls launch nothing
    assert lib.dfd_roc_ws(-1) == 0 and lib.dfd_roc_ws(_lib.ROC_MAX_N + 1) == 0
    assert lib.dfd_roc_ws(0) > 0 and lib.dfd_roc_ws(_lib.ROC_TILE + 1) == 2 * lib.dfd_roc_ws(_lib.ROC_TILE)
    assert lib.dfd_roc_curve(one, one, _lib.ROC_MAX_N + 1, 1, one, 1 << 30, one, one, one, one, None) == EINVAL
    assert lib.dfd_roc_curve(one, one, -1, 1, one, 64, one, one, one, one, None) == EINVAL
    for hole in range(7):                                           # score, label, ws, thr, cum_pos, cum_neg, stats
        ptrs = [one] * 7
        ptrs[hole] = None
        assert lib.dfd_roc_curve(ptrs[0], ptrs[1], 8, 1, ptrs[2], 64, ptrs[3], ptrs[4], ptrs[5], ptrs[6], None) == EINVAL, hole
    assert lib.dfd_roc_curve(one, one, 8, 1, one, 4, one, one, one, one, None) == -4                 # DFD_EWORKSPACE
    assert lib.dfd_roc_sweep(one, one, one, one, 8, one, _lib.ROC_MAX_CUTS + 1, one, one, None) == EINVAL
    assert lib.dfd_roc_sweep(one, one, one, one, 8, one, 0, one, one, None) == EINVAL
    for hole in range(7):                                           # thr, cum_pos, cum_neg, stats, cuts, tp, fp
        ptrs = [one] * 7
        ptrs[hole] = None
        assert lib.dfd_roc_sweep(ptrs[0], ptrs[1], ptrs[2], ptrs[3], 8, ptrs[4], 4, ptrs[5], ptrs[6], None) == EINVAL, hole
    assert lib.dfd_confusion(one, one, 8, _lib.CONFUSION_MAX_J + 1, one, one, None) == EINVAL
    assert lib.dfd_confusion(one, one, 8, 0, one, one, None) == EINVAL and lib.dfd_confusion(one, one, -1, 2, one, one, None) == EINVAL
    for hole in range(4):                                           # truth, pred, counts, oob
        ptrs = [one] * 4
        ptrs[hole] = None
        assert lib.dfd_confusion(ptrs[0], ptrs[1], 8, 2, ptrs[2], ptrs[3], None) == EINVAL, hole
