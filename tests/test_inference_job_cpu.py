"""The inference job end to end on the host, through orchestrate(path, mode="inference") alone.  The networks run on a HIP device
only, so a small torch model with weights set by hand stands in for the checkpoint: what is under test is the job around it.  Every
expected value is computed here from the stand-in's own outputs on the transformed pictures, batch by batch as the job feeds them."""

from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml
from PIL import Image

from deepfakedetection_amd import data as D
from deepfakedetection_amd.orchestration import orchestrator as O

SIZE, PER_CLASS, BATCH = 24, 4, 5                   # 8 or 12 pictures in batches of 5: the last batch is short
LEVELS = {"a_dark": 70, "b_mid": 128, "c_bright": 186}
ORDER = ["model", "split", "accuracy", "timestamp", "roc_auc", "threshold", "confusion_matrix"]


class _StandIn(torch.nn.Module):
    """AdaptiveAvgPool2d(1) -> Flatten -> Linear(3, J), row j = linspace(-1, 1, J)[j], no bias: the brighter the picture, the
    higher the class.  Keeps every batch it is handed."""

    def __init__(self, J: int) -> None:
        super().__init__()
        self.net = torch.nn.Sequential(torch.nn.AdaptiveAvgPool2d(1), torch.nn.Flatten(), torch.nn.Linear(3, J))
        with torch.no_grad():
            self.net[2].weight.copy_(torch.linspace(-1.0, 1.0, J)[:, None].expand(J, 3))
            self.net[2].bias.zero_()
        self.seen: list[torch.Tensor] = []

    def forward(self, x):
        self.seen.append(x.detach().clone())
        return self.net(x)


def _write_split(folder: Path, classes, rng, per_class: int = PER_CLASS) -> None:
    """Flat pictures whose brightness is the class's level plus one offset in -70..70 per picture: the classes overlap."""
    for cls in classes:
        (folder / cls).mkdir(parents=True)
        for i in range(per_class):
            value = int(np.clip(LEVELS[cls] + rng.integers(-70, 71), 0, 255))
            pixels = np.clip(value + rng.integers(-3, 4, size=(SIZE, SIZE, 3)), 0, 255).astype(np.uint8)
            Image.fromarray(pixels).save(folder / cls / f"{cls}_{i}.png")


def _job(tmp_path: Path, monkeypatch, classes, *, val="both"):
    """Write the data (val: "both" classes, "one" class, or None for no validation directory) and the YAML, run the job and
    return (the stand-in, the run directory)."""
    rng = np.random.default_rng(11)
    root = tmp_path / "data"
    _write_split(root / "test", classes, rng)
    if val == "both":
        _write_split(root / "val", classes, rng)
    elif val == "one":
        _write_split(root / "val", classes[:1], rng)
        (root / "val" / classes[1]).mkdir()
    stand_in = _StandIn(len(classes)).eval()
    monkeypatch.setattr(O, "load_model", lambda *args, **kwargs: stand_in)
    infer = {"split": "test", "batch_size": BATCH, "num_workers": 0, "img_size": SIZE}
    cfg = {"seed": 1, "device": "cpu",
           "data": {"root": str(root), "val_split": "val", "test_split": "test", "num_classes": len(classes), "img_size": SIZE},
           "models": {"efficientnet_b0": {"output_dir": str(tmp_path / "out"), "inference": infer}}, "selection": ["efficientnet_b0"]}
    path = tmp_path / "job.yaml"
    path.write_text(yaml.safe_dump(cfg))
    O.orchestrate(path, mode="inference")
    (run,) = [p for p in (tmp_path / "out").iterdir() if p.is_dir()]
    return stand_in, run


def _batches(folder: Path) -> list[torch.Tensor]:
    """The split's transformed pictures in the batches the job's loader makes of them."""
    dataset = D.ImageFolder(folder, transform=O.build_eval_transforms(SIZE))
    return list(torch.stack([dataset[i][0] for i in range(len(dataset))]).split(BATCH))


def _expected(stand_in: _StandIn, folder: Path):
    """(softmax probabilities, targets) of the split from the stand-in's own outputs."""
    with torch.inference_mode():
        probs = torch.cat([torch.softmax(stand_in.net(x), dim=1) for x in _batches(folder)])
    return probs, torch.tensor(D.ImageFolder(folder).targets)


def _confusion(truth: np.ndarray, pred: np.ndarray) -> list[list[int]]:
    labels = sorted(set(truth.tolist()) | set(pred.tolist()))
    return [[int(np.sum((truth == t) & (pred == p))) for p in labels] for t in labels]


def _rows(run: Path) -> list[dict]:
    return [json.loads(s) for s in (run / "logs" / "metrics.jsonl").read_text().splitlines()]


def _check_binary(stand_in: _StandIn, run: Path, root: Path, threshold: float) -> None:
    (row,) = _rows(run)
    assert list(row) == [k for k in ORDER if k in row] and set(ORDER) - set(row) <= {"roc_auc"}  # the key set and its order
    probs, truth = _expected(stand_in, root / "test")
    assert set(truth.tolist()) == {0, 1}                                                        # both classes occur in the split
    preds = (probs[:, 1] >= threshold).long()
    assert row["threshold"] == threshold
    assert row["accuracy"] == (preds == truth).float().mean().item()
    assert row["confusion_matrix"] == _confusion(truth.numpy(), preds.numpy())
    if "roc_auc" in row:
        assert 0.0 < row["roc_auc"] <= 1.0
    assert (run / "plots" / "confusion_matrix.png").exists() and not (run / "calibration.json").exists() and not (run / "cam").exists()


def test_binary_job_sweeps_its_threshold_on_the_validation_split(tmp_path, monkeypatch):
    stand_in, run = _job(tmp_path, monkeypatch, ["a_dark", "c_bright"])
    probs, truth = _expected(stand_in, tmp_path / "data" / "val")
    threshold = O.best_balanced_accuracy_threshold(probs[:, 1].numpy(), truth.numpy())
    assert threshold != 0.5 and 0.0 < threshold < 1.0                                           # the sweep is what sets it
    _check_binary(stand_in, run, tmp_path / "data", threshold)
    want = _batches(tmp_path / "data" / "val") + _batches(tmp_path / "data" / "test")           # one validation pass, then the split
    assert len(stand_in.seen) == len(want) and all(torch.equal(a, b) for a, b in zip(stand_in.seen, want))


@pytest.mark.parametrize("val", ["one", None])
def test_binary_job_keeps_one_half_without_a_usable_validation_split(tmp_path, monkeypatch, val):
    stand_in, run = _job(tmp_path, monkeypatch, ["a_dark", "c_bright"], val=val)
    _check_binary(stand_in, run, tmp_path / "data", 0.5)


def test_three_class_job_runs_no_validation_pass(tmp_path, monkeypatch):
    stand_in, run = _job(tmp_path, monkeypatch, ["a_dark", "b_mid", "c_bright"])
    want = _batches(tmp_path / "data" / "test")
    assert [tuple(x.shape) for x in want] == [(5, 3, SIZE, SIZE), (5, 3, SIZE, SIZE), (2, 3, SIZE, SIZE)]
    assert len(stand_in.seen) == len(want) and all(torch.equal(a, b) for a, b in zip(stand_in.seen, want))  # the split's batches only
    (row,) = _rows(run)
    assert list(row) == [k for k in ORDER if k in row] and set(ORDER) - set(row) <= {"roc_auc", "threshold"} and "threshold" not in row
    probs, truth = _expected(stand_in, tmp_path / "data" / "test")
    preds = probs.argmax(1)
    assert len(set(preds.tolist())) >= 2                                                        # not one class for everything
    assert row["accuracy"] == (preds == truth).float().mean().item()
    labels = sorted(set(truth.tolist()) | set(preds.tolist()))
    cm = np.asarray(row["confusion_matrix"])
    assert labels == [0, 1, 2] and cm.shape == (3, 3) and cm.tolist() == _confusion(truth.numpy(), preds.numpy())
    if "roc_auc" in row:
        assert 0.5 < row["roc_auc"] <= 1.0


def test_a_split_without_images_writes_nothing(tmp_path, monkeypatch, capsys):
    root = tmp_path / "data"
    for cls in ("a_dark", "c_bright"):
        (root / "test" / cls).mkdir(parents=True)
    monkeypatch.setattr(O, "load_model", lambda *args, **kwargs: _StandIn(2).eval())
    cfg = {"seed": 1, "device": "cpu", "data": {"root": str(root), "test_split": "test", "num_classes": 2, "img_size": SIZE},
           "models": {"efficientnet_b0": {"output_dir": str(tmp_path / "out"), "inference": {"num_workers": 0}}},
           "selection": ["efficientnet_b0"]}
    path = tmp_path / "job.yaml"
    path.write_text(yaml.safe_dump(cfg))
    O.orchestrate(path, mode="inference")
    (run,) = [p for p in (tmp_path / "out").iterdir() if p.is_dir()]
    assert "No images found" in capsys.readouterr().out and not (run / "logs" / "metrics.jsonl").exists()


def test_a_missing_split_exits_with_status_one(tmp_path, monkeypatch, capsys):
    (tmp_path / "data").mkdir()
    monkeypatch.setattr(O, "load_model", lambda *args, **kwargs: _StandIn(2).eval())
    cfg = {"seed": 1, "device": "cpu", "data": {"root": str(tmp_path / "data"), "test_split": "test", "num_classes": 2, "img_size": SIZE},
           "models": {"efficientnet_b0": {"output_dir": str(tmp_path / "out"), "inference": {"num_workers": 0}}},
           "selection": ["efficientnet_b0"]}
    path = tmp_path / "job.yaml"
    path.write_text(yaml.safe_dump(cfg))
    with pytest.raises(SystemExit) as exit_info:
        O.orchestrate(path, mode="inference")
    assert exit_info.value.code == 1 and "Split not found" in capsys.readouterr().out
