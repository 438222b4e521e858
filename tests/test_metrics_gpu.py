"""The device metrics (csrc/dfd_metrics.hip through kernels.roc_curve / roc_sweep / confusion_counts and
deepfakedetection_amd.metrics) against the integer reference of tests/_metrics_ref.py.  Every comparison is == on integers, or on
floats derived from equal integers.  Every output is an interior slice of a buffer filled with a canary (-1 for the integer
outputs, NaN for thr): the canaries around it must survive, and so must the entries of the compacted arrays past G."""

from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image

from deepfakedetection_amd import kernels as K
from deepfakedetection_amd import metrics as M
from tests import _metrics_ref as R

pytestmark = pytest.mark.gpu

GUARD = 32
TILE, SCAN = K.ROC_TILE, K.ROC_SCAN_WIDTH
LDS_J = K.CONFUSION_LDS_MAX_J


def _guarded(n: int, dtype, canary):
    big = torch.full((n + 2 * GUARD,), canary, dtype=dtype, device="cuda")
    return big, big[GUARD:GUARD + n]


def _intact(big: torch.Tensor, n: int, used: int | None = None) -> bool:
    """The canaries in front of and behind the n-element interior, and inside it from `used` on, are what they were."""
    host = big.cpu()
    rest = torch.cat([host[:GUARD], host[GUARD + (n if used is None else used):]])
    return bool(torch.isnan(rest).all()) if big.dtype.is_floating_point else bool((rest == -1).all())


def _grid_case(seed: int, n: int, values: int = 50, classes: int = 2):
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, classes, size=n).astype(np.int64)
    scores = (np.clip(rng.integers(0, values, size=n) + 6 * (labels == 1), 0, values - 1) / (values - 1)).astype(np.float32)
    return scores, labels


def _ascending(scores: np.ndarray, labels: np.ndarray, seed: int = 0):
    """The pair sorted by score, in a random order inside every run of equal scores (NaN last)."""
    perm = np.random.default_rng(seed).permutation(scores.size)
    order = perm[np.argsort(scores[perm], kind="stable")]
    return scores[order], labels[order]


def _curve(scores: np.ndarray, labels: np.ndarray, positive: int = 1, seed: int = 0):
    """dfd_roc_curve on the sorted pair -> (thr[:G], cum_pos[:G], cum_neg[:G], stats) as numpy / list, after the canary checks."""
    s, l = _ascending(scores, labels, seed)
    n = s.size
    thr_big, thr = _guarded(n, torch.float32, float("nan"))
    pos_big, pos = _guarded(n, torch.int64, -1)
    neg_big, neg = _guarded(n, torch.int64, -1)
    st_big, st = _guarded(K.ROC_STATS_LEN, torch.int64, -1)
    K.roc_curve(torch.from_numpy(s).cuda(), torch.from_numpy(l).cuda(), positive, out=(thr, pos, neg, st))
    torch.cuda.synchronize()
    stats = st.cpu().tolist()
    G = stats[2]
    assert 0 <= G <= n and _intact(st_big, K.ROC_STATS_LEN)
    assert _intact(thr_big, n, G) and _intact(pos_big, n, G) and _intact(neg_big, n, G), "a write outside thr / cum_pos / cum_neg [0, G)"
    return thr[:G].cpu().numpy(), pos[:G].cpu().numpy(), neg[:G].cpu().numpy(), stats


def _check(scores: np.ndarray, labels: np.ndarray, positive: int = 1, seed: int = 0):
    got = _curve(scores, labels, positive, seed)
    # (the reference sorts stably, so it sees the pairs in the kernel's order: every NaN is a group of its own, and which label sits
    # in which of them is the order of the input; inside a real tie group the order changes nothing)
    want = R.groups(*_ascending(scores, labels, seed), positive)
    assert got[3] == want[3], (got[3], want[3])
    assert np.array_equal(got[0], want[0], equal_nan=True) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    return got


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, SCAN * TILE + 1])
def test_roc_curve_sizes(n):
    """(the last size has one tile more than the scan's block has threads: the smallest that takes the scan loop's second trip)"""
    scores, labels = _grid_case(n, n)
    stats = _check(scores, labels)[3]
    assert stats[4] == R.two_u(scores, labels) and stats[0] + stats[1] == n


def test_all_scores_equal():
    n = TILE + 5
    labels = (np.arange(n) % 3 == 0).astype(np.int64)
    stats = _check(np.full(n, 0.25, dtype=np.float32), labels)[3]
    assert stats[2] == 1 and stats[4] == stats[0] * stats[1]
    res = M.binary_roc(torch.full((n,), 0.25, device="cuda"), torch.from_numpy(labels).cuda())
    assert res.auc == 0.5 and res.groups == 1 and res.eer == 0.5


@pytest.mark.parametrize("lo,hi,n", [(TILE - 3, TILE + 3, 2 * TILE), (TILE, 4 * TILE, 5 * TILE), (TILE - 1, 4 * TILE + 1, 5 * TILE + 7)])
def test_tie_group_across_tile_boundaries(lo, hi, n):
    """One tie group [lo, hi) among distinct scores: straddling one tile edge, covering three whole tiles, and both."""
    scores = np.arange(n, dtype=np.float32)
    scores[lo:hi] = scores[lo]
    labels = np.random.default_rng(n).integers(0, 2, size=n).astype(np.int64)
    thr, _, _, stats = _check(scores, labels)
    assert stats[2] == n - (hi - lo) + 1 and thr[lo] == scores[lo] and stats[4] == R.two_u(scores, labels)


def test_perfect_and_inverted_separation():
    n = TILE + 100
    labels = (np.arange(n) >= n // 3).astype(np.int64)
    scores = np.arange(n, dtype=np.float32) / n
    _check(scores, labels)
    _check(scores, 1 - labels)
    dev = torch.from_numpy(scores).cuda()
    up, down = M.binary_roc(dev, torch.from_numpy(labels).cuda()), M.binary_roc(dev, torch.from_numpy(1 - labels).cuda())
    assert up.auc == 1.0 and down.auc == 0.0 and up.eer == 0.0 and down.eer == 1.0


def test_signed_zeros_are_one_group_and_subnormals_are_not_zero():
    tiny = np.float32(1e-45)                                          # the smallest subnormal
    assert tiny > 0 and tiny == np.float32(2 ** -149)
    scores = np.asarray([-0.0, 0.0, -0.0, 0.0, 0.0, -0.0, 0.5, -0.5], dtype=np.float32)
    labels = np.asarray([1, 0, 0, 1, 1, 0, 1, 0], dtype=np.int64)
    for seed in range(4):                                             # either zero may end the group
        thr, _, _, stats = _check(scores, labels, seed=seed)
        assert stats[2] == 3 and thr[1] == 0.0
    scores = np.asarray([0.0, tiny, -tiny, 0.0, np.float32(1e-40), tiny, -0.0, np.float32(-1e-40)], dtype=np.float32)
    labels = np.asarray([0, 1, 0, 1, 1, 0, 1, 0], dtype=np.int64)
    thr, _, _, stats = _check(scores, labels)
    assert stats[2] == 5 and thr.tolist() == [np.float32(-1e-40), -tiny, 0.0, tiny, np.float32(1e-40)]


def test_one_class_absent():
    scores, labels = _grid_case(7, TILE + 9)
    for only in (0, 1):
        stats = _check(scores, np.full_like(labels, only))[3]
        assert stats[1 - only] == scores.size and stats[only] == 0 and stats[4] == 0       # stats = P, N, ...: label 0 fills N
        res = M.binary_roc(torch.from_numpy(scores).cuda(), torch.full((scores.size,), only, dtype=torch.int64, device="cuda"))
        assert res.auc is None and res.eer is None and res.groups == stats[2]
    assert M.ovr_auc(torch.rand(40, 3, device="cuda"), torch.randint(0, 2, (40,), device="cuda"), 3) is None


@pytest.mark.parametrize("bad", [1, 2, "all"])
def test_nonfinite_scores_are_counted(bad):
    n = TILE + 40
    scores, labels = _grid_case(11, n)
    k = n if bad == "all" else bad
    scores[np.random.default_rng(bad if bad != "all" else 9).choice(n, size=k, replace=False)] = \
        np.resize(np.asarray([np.nan, np.inf, -np.inf], dtype=np.float32), k)
    stats = _check(scores, labels)[3]
    assert stats[3] == k
    dev, truth = torch.from_numpy(scores).cuda(), torch.from_numpy(labels).cuda()
    with pytest.raises(ValueError, match="NaN or infinite"):
        M.binary_roc(dev, truth)
    loose = M.binary_roc(dev, truth, strict=False)
    assert loose.nonfinite == k and np.isnan(loose.auc) and np.isnan(loose.eer)


def test_order_inside_tie_groups_does_not_matter():
    scores, labels = _grid_case(21, 2 * TILE + 300, values=9)
    first = _curve(scores, labels, seed=1)
    for seed in (2, 3):
        again = _curve(scores, labels, seed=seed)
        assert first[3] == again[3] and all(np.array_equal(a, b) for a, b in zip(first[:3], again[:3]))


def test_another_positive_id_among_three_classes():
    scores, labels = _grid_case(31, TILE + 77, classes=3)
    for positive in (0, 2):
        stats = _check(scores, labels, positive)[3]
        assert stats[0] == int((labels == positive).sum()) and stats[4] == R.two_u(scores, labels, positive)
    probs = torch.softmax(torch.randn(500, 3, generator=torch.Generator().manual_seed(2)), dim=1)
    truth = torch.arange(500) % 3
    want = sum(R.auc(probs[:, j].numpy(), truth.numpy(), j) for j in range(3)) / 3
    assert M.ovr_auc(probs.cuda(), truth.cuda(), 3) == want


def test_empty_input_leaves_zeros():
    assert _curve(np.zeros(0, np.float32), np.zeros(0, np.int64))[3] == [0, 0, 0, 0, 0]
    res = M.binary_roc(torch.zeros(0, device="cuda"), torch.zeros(0, dtype=torch.int64, device="cuda"), cuts=[0.5])
    assert res.auc is None and res.groups == 0 and res.tp.tolist() == [0] and res.fp.tolist() == [0] and res.curve()[0].size == 0


def test_binary_roc_on_unsorted_scores():
    scores, labels = _grid_case(41, 3 * TILE + 123)
    res = M.binary_roc(torch.from_numpy(scores).cuda(), torch.from_numpy(labels).cuda())
    assert res.two_u == R.two_u(scores, labels) and res.auc == R.auc(scores, labels)
    assert (res.n_pos, res.n_neg, res.groups, res.nonfinite) == (int(labels.sum()), int((labels == 0).sum()), len(np.unique(scores)), 0)
    fps, tps, thresholds = R.roc_counts(scores, labels)
    got = res.curve()
    assert np.array_equal(got[0], fps) and np.array_equal(got[1], tps) and np.array_equal(got[2], thresholds)
    assert res.eer == M.eer_from_curve(fps, tps, res.n_pos, res.n_neg) and abs(res.eer - R.eer(scores, labels)) < 1e-12


# ------------------------------------------------------------------ dfd_roc_sweep
def _sweep(scores: np.ndarray, labels: np.ndarray, cuts: np.ndarray):
    s, l = _ascending(scores, labels)
    curve = K.roc_curve(torch.from_numpy(s).cuda(), torch.from_numpy(l).cuda())
    T = cuts.size
    tp_big, tp = _guarded(T, torch.int64, -1)
    fp_big, fp = _guarded(T, torch.int64, -1)
    K.roc_sweep(*curve, torch.from_numpy(cuts).cuda(), out=(tp, fp))
    torch.cuda.synchronize()
    assert _intact(tp_big, T) and _intact(fp_big, T)
    return tp.cpu().numpy(), fp.cpu().numpy()


def _sweep_case():
    """Scores that hold float32(cut) for every cut of the orchestrator's grid (241 of them below their cut, 255 above: an f32
    comparison counts them wrong), exactly 0 and 1, and a grid of ties."""
    cuts = np.linspace(0.0, 1.0, 501, dtype=np.float64)
    on_cuts = cuts.astype(np.float32)
    assert (on_cuts.astype(np.float64) < cuts).sum() == 241 and (on_cuts.astype(np.float64) > cuts).sum() == 255
    extra, _ = _grid_case(51, 1500)
    scores = np.concatenate([on_cuts, on_cuts, extra, np.asarray([0.0, 1.0, 0.0, 1.0], dtype=np.float32)])
    labels = np.random.default_rng(52).integers(0, 2, size=scores.size).astype(np.int64)
    return scores, labels, cuts


def test_sweep_on_the_orchestrators_grid_compares_in_f64():
    from deepfakedetection_amd.orchestration.orchestrator import best_balanced_accuracy_threshold

    scores, labels, cuts = _sweep_case()
    tp, fp = _sweep(scores, labels, cuts)
    want_tp, want_fp = R.sweep(scores, labels, cuts)
    assert np.array_equal(tp, want_tp) and np.array_equal(fp, want_fp)
    as_f32 = R.sweep(scores, labels, cuts.astype(np.float32))
    assert not np.array_equal(as_f32[0], want_tp)                     # the data does tell an f32 comparison apart
    res = M.binary_roc(torch.from_numpy(scores).cuda(), torch.from_numpy(labels).cuda(), cuts=cuts)
    assert np.array_equal(res.tp, want_tp) and np.array_equal(res.fp, want_fp)
    assert res.best_balanced_accuracy_threshold() == best_balanced_accuracy_threshold(scores, labels) == R.best_threshold(scores, labels, cuts)


@pytest.mark.parametrize("T", [1, K.ROC_MAX_CUTS])
def test_sweep_with_one_cut_and_with_the_most(T):
    scores, labels, _ = _sweep_case()
    cuts = np.asarray([0.37]) if T == 1 else np.linspace(-0.1, 1.1, T)
    tp, fp = _sweep(scores, labels, cuts)
    want = R.sweep(scores, labels, cuts)
    assert np.array_equal(tp, want[0]) and np.array_equal(fp, want[1])
    if T > 1:
        assert tp[0] == labels.sum() and tp[-1] == 0 and fp[0] == (labels == 0).sum() and fp[-1] == 0


def test_sweep_of_an_empty_curve():
    tp, fp = _sweep(np.zeros(0, np.float32), np.zeros(0, np.int64), np.linspace(0.0, 1.0, 501))
    assert not tp.any() and not fp.any()


# ------------------------------------------------------------------ dfd_confusion
def _confusion(truth: np.ndarray, pred: np.ndarray, J: int):
    big, counts = _guarded(J * J, torch.int64, -1)
    oob_big, oob = _guarded(1, torch.int64, -1)
    K.confusion_counts(torch.from_numpy(truth).cuda(), torch.from_numpy(pred).cuda(), J, out=(counts.view(J, J), oob))
    torch.cuda.synchronize()
    assert _intact(big, J * J) and _intact(oob_big, 1)
    return counts.view(J, J).cpu().numpy(), int(oob.item())


@pytest.mark.parametrize("n", [100, 20000])                           # one workgroup, several
@pytest.mark.parametrize("J", [2, 3, 10, LDS_J, LDS_J + 1, K.CONFUSION_MAX_J])
def test_confusion_counts(J, n):
    rng = np.random.default_rng(J * 7 + n)
    truth, pred = rng.integers(0, J, size=n), rng.integers(0, J, size=n)
    pred[: n // 2] = truth[: n // 2]                                  # a heavy diagonal
    got, oob = _confusion(truth, pred, J)
    want, _ = R.confusion(truth, pred, J)
    assert oob == 0 and np.array_equal(got, want) and got.sum() == n
    assert torch.equal(M.confusion(torch.from_numpy(truth).cuda(), torch.from_numpy(pred).cuda(), J).cpu(), torch.from_numpy(want))


@pytest.mark.parametrize("J", [3, LDS_J, LDS_J + 1])
def test_confusion_all_samples_in_one_cell(J):
    n = 20000
    got, oob = _confusion(np.full(n, J - 1, dtype=np.int64), np.full(n, 1, dtype=np.int64), J)
    assert oob == 0 and got[J - 1, 1] == n and got.sum() == n


@pytest.mark.parametrize("J", [2, LDS_J, LDS_J + 1])
def test_confusion_leaves_out_of_range_labels_out(J):
    n = 9000
    rng = np.random.default_rng(J)
    truth, pred = rng.integers(0, J, size=n), rng.integers(0, J, size=n)
    truth[::7], pred[3::11], truth[5::13], pred[1::17] = -1, J, J + 1000, -(2 ** 40)
    got, oob = _confusion(truth, pred, J)
    want, want_oob = R.confusion(truth, pred, J)
    assert want_oob > 1000 and oob == want_oob and np.array_equal(got, want) and got.sum() == n - want_oob
    with pytest.raises(ValueError, match="outside"):
        M.confusion(torch.from_numpy(truth).cuda(), torch.from_numpy(pred).cuda(), J)
    got, oob = _confusion(np.full(n, -5, dtype=np.int64), np.zeros(n, dtype=np.int64), J)
    assert oob == n and not got.any()


# ------------------------------------------------------------------ end to end
def _write_pngs(root: Path, classes=("fake", "real")) -> None:
    rng = np.random.default_rng(5)
    for split in ("val", "test"):
        for cls in classes:
            folder = root / split / cls
            folder.mkdir(parents=True)
            for i in range(4):
                Image.fromarray(rng.integers(0, 256, size=(24, 24, 3), dtype=np.uint8)).save(folder / f"{cls}_{i}.png")


def _config(tmp_path: Path, out: str, device_metrics: bool, num_classes: int = 2) -> Path:
    import yaml

    infer = {"split": "test", "batch_size": 8, "num_workers": 0, "img_size": 64, "gpu_resize": True, "robustness": {"blur_sigma": [2]}}
    if device_metrics:
        infer["device_metrics"] = True
    cfg = {"seed": 1, "device": "cuda",
           "data": {"root": str(tmp_path / "data"), "val_split": "val", "test_split": "test", "num_classes": num_classes, "img_size": 64},
           "models": {"efficientnet_b0": {"output_dir": str(tmp_path / out), "inference": infer}}, "selection": ["efficientnet_b0"]}
    path = tmp_path / f"{out}.yaml"
    path.write_text(yaml.safe_dump(cfg))
    return path


def _rows(base: Path) -> list[dict]:
    (run,) = [p for p in base.iterdir() if p.is_dir()]
    return [{k: v for k, v in json.loads(s).items() if k != "timestamp"} for s in (run / "logs" / "metrics.jsonl").read_text().splitlines()]


def test_inference_with_device_metrics(tmp_path, monkeypatch):
    from deepfakedetection_amd.orchestration import orchestrator as O

    _write_pngs(tmp_path / "data")
    O.orchestrate(_config(tmp_path, "plain", False), mode="inference")
    books = []
    real = O._split_metrics_device
    monkeypatch.setattr(O, "_split_metrics_device",
                        lambda name, split, book, J, thr: (books.append((book.probs.cpu().numpy().copy(), book.targets.cpu().numpy().copy())),
                                                           real(name, split, book, J, thr))[1])
    sweeps = []
    real_sweep = O._device_threshold
    monkeypatch.setattr(O, "_device_threshold", lambda book: (sweeps.append(real_sweep(book)), sweeps[-1])[1])
    O.orchestrate(_config(tmp_path, "device", True), mode="inference")
    plain, rows = _rows(tmp_path / "plain"), _rows(tmp_path / "device")
    keys = {"model", "split", "accuracy", "threshold", "confusion_matrix"}
    assert len(plain) == len(rows) == 2 == len(books)
    for before, after, (probs, truth) in zip(plain, rows, books):
        assert set(before) - {"roc_auc", "perturbation"} == keys                       # the plain rows keep their shape
        assert set(after) - {"perturbation"} == keys | {"roc_auc", "eer", "balanced_accuracy"}
        assert before.get("perturbation") == after.get("perturbation")
        for key in ("accuracy", "threshold", "confusion_matrix"):
            assert after[key] == before[key], key
        assert after["roc_auc"] == R.auc(probs[:, 1], truth)
        if "roc_auc" in before:                                                         # sklearn is present: its trapezoid, 8 terms
            assert abs(before["roc_auc"] - after["roc_auc"]) < 1e-12
        assert 0.0 <= after["eer"] <= 1.0 and 0.0 <= after["balanced_accuracy"] <= 1.0
        cm = np.asarray(after["confusion_matrix"])
        assert cm.shape == (2, 2) and after["balanced_accuracy"] == float(np.mean(np.diag(cm) / cm.sum(1)))
    assert len(sweeps) == 1 and sweeps[0] == rows[0]["threshold"]                      # the validation sweep ran on the device
    (run,) = [p for p in (tmp_path / "device").iterdir() if p.is_dir()]
    assert (run / "plots" / "roc_curve.png").exists()


def test_three_class_inference_agrees_between_host_and_device(tmp_path, monkeypatch):
    """Above two classes there is no threshold and no validation pass; the AUC is the macro one-vs-rest mean."""
    from deepfakedetection_amd.orchestration import orchestrator as O

    _write_pngs(tmp_path / "data", classes=("a", "b", "c"))
    O.orchestrate(_config(tmp_path, "plain", False, 3), mode="inference")
    books = []
    real = O._split_metrics_device
    monkeypatch.setattr(O, "_split_metrics_device",
                        lambda name, split, book, J, thr: (books.append((book.probs.cpu().numpy().copy(), book.targets.cpu().numpy().copy())),
                                                           real(name, split, book, J, thr))[1])
    O.orchestrate(_config(tmp_path, "device", True, 3), mode="inference")
    plain, rows = _rows(tmp_path / "plain"), _rows(tmp_path / "device")
    assert len(plain) == len(rows) == 2 == len(books)
    for before, after, (probs, truth) in zip(plain, rows, books):
        assert "threshold" not in before and "threshold" not in after
        assert before.get("perturbation") == after.get("perturbation")
        for key in ("accuracy", "confusion_matrix"):
            assert after[key] == before[key], key
        assert probs.shape == (12, 3) and sorted(set(truth.tolist())) == [0, 1, 2]      # every class occurs: the AUC is defined
        assert after["roc_auc"] == sum(R.auc(probs[:, j], truth, positive=j) for j in range(3)) / 3
        assert after["eer"] is not None and after["balanced_accuracy"] is not None
    assert rows[1]["perturbation"] == {"blur_sigma": 2.0} and "perturbation" not in rows[0]


class _Recording(torch.nn.Module):
    def __init__(self) -> None:
        super().__init__()
        self.net = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(3 * 8 * 8, 2))
        self.seen: list = []

    def forward(self, x):
        logits = self.net(x)
        self.seen.append(logits.detach().clone())
        return logits


def test_evaluate_reports_the_exact_auc(monkeypatch):
    from torch.utils.data import DataLoader, TensorDataset

    from deepfakedetection_amd.trainers._engine import evaluate

    monkeypatch.setenv("GRAPH_STEP", "0")                                               # a plain torch module: no graphed forward
    torch.manual_seed(3)
    model = _Recording().cuda()
    y = torch.arange(100) % 4 == 0                                                      # a 1:3 split
    x = torch.randn(100, 3, 8, 8) + 0.05 * y[:, None, None, None]
    loader = DataLoader(TensorDataset(x, y.long()), batch_size=32)
    off = evaluate(model, loader, "cuda")
    model.seen.clear()
    on = evaluate(model, loader, "cuda", val_auc=True)
    assert off.auc is None and off.eer is None
    assert (on.acc, on.total, on.correct) == (off.acc, off.total, off.correct) and on.total == 100
    assert [t.shape[0] for t in model.seen] == [32, 32, 32, 4]
    scores = torch.cat([torch.softmax(t.float(), dim=1) for t in model.seen])[:, 1].cpu().numpy()
    assert on.auc == R.auc(scores, y.long().numpy()) and 0.0 < on.auc < 1.0
    assert abs(on.eer - R.eer(scores, y.long().numpy())) < 1e-12


def test_selection_step_where_accuracy_and_auc_disagree():
    from deepfakedetection_amd.trainers._engine import EvalResult, improves, selection_value

    truth = torch.tensor([0] * 8 + [1] * 2, device="cuda")
    # a: everything called negative but ranked perfectly; b: one more sample right at 0.5, ranked worse
    a = torch.tensor([0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.2, 0.3, 0.4], device="cuda")
    b = torch.tensor([0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.45, 0.05, 0.9], device="cuda")
    results = []
    for scores in (a, b):
        correct = int(((scores >= 0.5).long() == truth).sum())
        results.append(EvalResult(acc=correct / 10, total=10, correct=correct, auc=M.binary_roc(scores, truth).auc))
    ra, rb = results
    assert (ra.acc, rb.acc) == (0.8, 0.9) and ra.auc == 1.0 and rb.auc == R.auc(b.cpu().numpy(), truth.cpu().numpy()) < 1.0
    assert improves(selection_value(rb, "acc"), selection_value(ra, "acc")) and not improves(selection_value(rb, "auc"), selection_value(ra, "auc"))
    assert improves(selection_value(ra, "auc"), selection_value(rb, "auc")) and not improves(selection_value(ra, "acc"), selection_value(rb, "acc"))
