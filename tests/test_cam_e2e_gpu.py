"""GradCam end to end on the HIP models against the CPU oracle, and the orchestrator / CLI integration.

Per family (EfficientNet-B0 timm, EfficientNet-B3 lukemelas, EfficientFormerV2-S1, FasterViT-0; batch 8, non-degenerate
BatchNorm statistics as in the existing hook tests): the oracle's target-layer activation and gradient, captured through
the same hooks, go through the numpy restatement (tests/_cam_ref.py); the engine's heatmap and overlay must agree with it
and with its own batch-1 results, and the fused path must be back after the context exits."""

from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _cam_ref as R

pytestmark = pytest.mark.gpu

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def _calibrate(ref, x):
    bns = [m for m in ref.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    for m in bns:
        m.momentum = 1.0
    ref.train()
    with torch.no_grad():
        ref(x)


def _family(kind, x):
    """(oracle, HIP model, the oracle's target module) for one family, both in eval mode."""
    last = lambda m: [c for c in m.modules() if isinstance(c, torch.nn.Conv2d)][-1]     # noqa: E731
    if kind in ("b0", "b3"):
        from tests.test_model_gpu import make_pair

        ref, hip = make_pair(kind, "timm" if kind == "b0" else "lukemelas", 2)
        _calibrate(ref, x)
        hip.load_state_dict(ref.state_dict())
        target = ref.conv_head if kind == "b0" else ref._conv_head
    elif kind == "s1":
        from tests.test_efformer_gpu import make_pair

        ref, hip = make_pair("s1", 2, 224, seed=4)
        fc2 = ref.stages[3].blocks[-1].mlp.fc2

        def via_module(t):            # the oracle's ConvBN calls F.conv2d on the weights: route the target through the module
            y = fc2.conv(t)
            return F.batch_norm(y, fc2.bn.running_mean, fc2.bn.running_var, fc2.bn.weight, fc2.bn.bias, False, 0.0, fc2.bn.eps)

        fc2.forward = via_module
        target = fc2.conv
    else:
        from tests.test_fastervit_gpu import make_pair

        ref, hip = make_pair("0", 2, seed=6)
        target = last(ref)
    ref.eval(); hip.eval()
    return ref, hip, target


def _oracle_cam(ref, target, x, lut):
    kept = {}

    def hook(module, inputs, output):
        kept["act"] = output
        output.register_hook(lambda g: kept.__setitem__("grad", g))

    h = target.register_forward_hook(hook)
    try:
        logits = ref(x)
        preds = logits.argmax(1)
        logits.gather(1, preds.view(-1, 1)).sum().backward()
    finally:
        h.remove()
    act, grad = kept["act"].detach(), kept["grad"].detach()
    N, C, hh, ww = act.shape
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(N, hh * ww, C).numpy()        # noqa: E731
    cam = R.gradcam_map_f32(flat(act), flat(grad)).reshape(N, hh, ww)
    heat, over = R.render(cam, x.numpy(), MEAN, STD, lut, x.shape[2], x.shape[3])
    return preds, heat, over


@pytest.mark.parametrize("kind,size", [("b0", 128), ("b3", 128), ("s1", 224), ("fv0", 224)])
def test_gradcam_matches_the_oracle(kind, size):
    from deepfakedetection_amd.cam import GradCam, default_lut

    x = torch.randn(8, 3, size, size, generator=torch.Generator().manual_seed(17))
    ref, hip, target = _family(kind, x)
    lut = default_lut()
    want_preds, want_heat, want_over = _oracle_cam(ref, target, x, lut)

    xd = x.cuda()
    with torch.inference_mode():
        before = hip(xd).clone()
    with GradCam(hip, batch_size=8) as cam:
        got = cam(xd, overlay=True)
    with GradCam(hip, batch_size=1) as cam:
        single = cam(xd)
    with torch.inference_mode():
        after = hip(xd)
    assert torch.equal(before, after), "fused eval path not restored after the context exit"

    assert torch.equal(got.preds.cpu(), want_preds)
    assert torch.equal(got.preds, single.preds)
    heat = got.heatmap.cpu().numpy()
    over = got.overlay.cpu().numpy()
    assert heat.shape == (8, size, size) and over.shape == (8, size, size, 3) and over.dtype == np.uint8
    heat_err = float(np.abs(heat - want_heat).max())
    diff = np.abs(over.astype(np.int16) - want_over.astype(np.int16))
    within = float((diff <= 2).mean())
    batch_err = float((got.heatmap - single.heatmap).abs().max())
    print(f"[cam {kind}] heat max abs err {heat_err:.2e}, overlay max diff {int(diff.max())}, "
          f"within 2 levels {within:.5f}, batch-8 vs batch-1 {batch_err:.2e}")
    assert (want_heat.reshape(8, -1).max(1) > 0.5).sum() >= 4, "degenerate case: most maps are empty"
    # observed on the MI355X: heat <= 1.9e-5, overlay at most 3 levels apart and 99.999 % within 2 (issue bound: 1e-2 / 99.5 %)
    assert heat_err <= 1e-4
    assert int(diff.max()) <= 8 and within >= 0.999
    assert batch_err <= 1e-5


def _write_jpegs(root: Path, n_per_class: int = 4) -> None:
    from PIL import Image

    rng = np.random.default_rng(5)
    for cls in ("fake", "real"):
        folder = root / "test" / cls
        folder.mkdir(parents=True)
        for i in range(n_per_class):
            arr = rng.integers(0, 256, size=(int(rng.integers(60, 90)), int(rng.integers(60, 90)), 3), dtype=np.uint8)
            Image.fromarray(arr).save(folder / f"{cls}_{i}.jpg", quality=90)


def _config(tmp_path: Path, out: str, cam: bool, models=("efficientnet_b0",)) -> Path:
    import yaml

    entry = lambda name: {"output_dir": str(tmp_path / out / name), "inference": {      # noqa: E731
        "split": "test", "batch_size": 4, "num_workers": 0, "img_size": 224, **({"cam": {"limit": 5}} if cam else {})}}
    cfg = {"seed": 1, "device": "cuda", "data": {"root": str(tmp_path / "data"), "test_split": "test", "num_classes": 2,
                                                 "img_size": 224},
           "models": {name: entry(name) for name in models}, "selection": list(models)}
    path = tmp_path / f"{out}.yaml"
    path.write_text(yaml.safe_dump(cfg))
    return path


def _run_dir(base: Path) -> Path:
    (run,) = [p for p in base.iterdir() if p.is_dir()]
    return run


def test_orchestrator_writes_cam_overlays_and_leaves_metrics_alone(tmp_path):
    from deepfakedetection_amd.orchestration.orchestrator import orchestrate

    _write_jpegs(tmp_path / "data")
    orchestrate(_config(tmp_path, "plain", cam=False), mode="inference")
    orchestrate(_config(tmp_path, "cam", cam=True), mode="inference")
    plain = _run_dir(tmp_path / "plain" / "efficientnet_b0")
    run = _run_dir(tmp_path / "cam" / "efficientnet_b0")
    assert not (plain / "cam").exists()
    pngs = sorted((run / "cam").rglob("*.png"))
    lines = [json.loads(line) for line in (run / "cam" / "index.jsonl").read_text().splitlines()]
    assert len(pngs) == 5 and len(lines) == 5
    for line in lines:
        png = run / line["png"]
        assert png.exists() and png.parent.name == line["truth"]
        assert f"__pred-{line['prediction']}_" in png.name and 0.0 <= line["probability"] <= 1.0
    from PIL import Image

    with Image.open(pngs[0]) as im:
        assert im.size == (224, 224) and im.mode == "RGB"
    strip = lambda p: [{k: v for k, v in json.loads(s).items() if k != "timestamp"}                     # noqa: E731
                       for s in (p / "logs" / "metrics.jsonl").read_text().splitlines()]
    assert strip(run) == strip(plain)


def test_cli_writes_one_panel_per_selected_model(tmp_path):
    from PIL import Image

    from deepfakedetection_amd.cam import main

    _write_jpegs(tmp_path / "data", 1)
    models = ("efficientnet_b0", "efficientnet_b3")
    img = next((tmp_path / "data" / "test" / "fake").glob("*.jpg"))
    main(["--config", str(_config(tmp_path, "cli", cam=False, models=models)), "--out", str(tmp_path / "png"), str(img)])
    (png,) = list((tmp_path / "png").glob("*.png"))
    with Image.open(png) as im:
        assert im.size == (len(models) * 224, 224)
