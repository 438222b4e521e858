"""Grad-CAM without a GPU: the numpy restatement of the map and render arithmetic (tests/_cam_ref.py) on hand-computed
cases, the default colour map, target resolution on the three families, the `inference.cam` key, argument checks of the
two entry points and of the GradCam front end."""

from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest
import torch

from tests import _cam_ref as R

ROOT = Path(__file__).resolve().parents[1]


def test_resize_2x2_to_4x4_by_hand():
    # half-pixel centres: columns sample at -0.25 (clamped), 0.25, 0.75, 1.25 (clamped); rows the same
    img = np.array([[0.0, 4.0], [8.0, 12.0]], np.float32)
    want = np.array([[0, 1, 3, 4], [2, 3, 5, 6], [6, 7, 9, 10], [8, 9, 11, 12]], np.float32)
    got = R.resize_linear(img, 4, 4)
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, want)


def test_resize_clamps_at_the_edges():
    img = np.array([[1.0, 5.0, 3.0]], np.float32)
    got = R.resize_linear(img, 2, 7)                   # 1x3 -> 2x7: one source row, every output row equals it
    assert got.shape == (2, 7)
    np.testing.assert_array_equal(got[0], got[1])
    assert got[0, 0] == 1.0 and got[0, -1] == 3.0      # outermost samples fall before the first / after the last centre
    assert got.min() >= 1.0 and got.max() <= 5.0
    # interior sample: dx = 3 -> fx = 3.5 * 3/7 - 0.5 = 1.0 exactly -> the middle source value
    assert got[0, 3] == 5.0


def test_resize_1x1_is_constant():
    got = R.resize_linear(np.array([[0.37]], np.float32), 5, 9)
    np.testing.assert_array_equal(got, np.full((5, 9), np.float32(0.37)))


@pytest.mark.parametrize("cam", [np.full((7, 7), 3.25, np.float32), np.zeros((7, 7), np.float32)])
def test_constant_map_gives_a_zero_heatmap(cam):
    heat = R.heatmap(cam, 224, 224)
    assert heat.dtype == np.float32
    np.testing.assert_array_equal(heat, np.zeros((224, 224), np.float32))


def test_all_negative_map_gives_a_zero_heatmap():
    rng = np.random.default_rng(0)
    act = rng.random((1, 49, 16), dtype=np.float32)
    grad = -rng.random((1, 49, 16), dtype=np.float32)                # every weight negative, every activation positive
    cam = R.gradcam_map_f32(act, grad).reshape(1, 7, 7)
    np.testing.assert_array_equal(cam, 0)
    np.testing.assert_array_equal(R.heatmap(cam[0], 32, 32), 0)


def test_heatmap_spans_zero_to_one():
    rng = np.random.default_rng(1)
    heat = R.heatmap(rng.random((14, 14), dtype=np.float32), 224, 224)
    assert heat.min() == 0.0 and 0.999 < heat.max() <= 1.0


def test_default_lut_runs_dark_blue_to_dark_red():
    from deepfakedetection_amd.cam import default_lut

    lut = default_lut()
    assert lut.shape == (256, 3) and lut.dtype == np.uint8
    r, g, b = (int(v) for v in lut[0])
    assert r == 0 and g == 0 and 100 <= b <= 160                     # dark blue
    r, g, b = (int(v) for v in lut[-1])
    assert 100 <= r <= 160 and g == 0 and b == 0                     # dark red


def test_overlay_reference_blends_and_rescales():
    lut = np.zeros((256, 3), np.uint8)
    lut[:, 0] = 255
    img = np.full((2, 2, 3), 0.5, np.float32)
    out = R.overlay(img, np.zeros((2, 2), np.float32), lut)
    # 0.5 * (1, 0, 0) + 0.5 * 0.5 = (0.75, 0.25, 0.25); / 0.75 -> (1, 1/3, 1/3) -> (255, 85, 85)
    np.testing.assert_array_equal(out[0, 0], [255, 85, 85])


def _names(model):
    return {id(m): n for n, m in model.named_modules()}


@pytest.mark.parametrize("family,args,want", [
    ("efficientnet", ("b0", "timm", 2), "conv_head"),
    ("efficientnet", ("b3", "lukemelas", 2), "_conv_head"),
    ("efficientformer_v2", ("s1", 2, 224), "stages.3.blocks.5.mlp.fc2.conv"),
    ("fastervit", ("0", 2, 224), "levels.2.global_tokenizer.pos_embed"),
])
def test_target_resolution_on_the_three_families(family, args, want):
    from deepfakedetection_amd.cam import resolve_target

    if family == "efficientnet":
        from deepfakedetection_amd.efficientnet import HipEfficientNet as M
    elif family == "efficientformer_v2":
        from deepfakedetection_amd.efficientformer_v2 import HipEfficientFormerV2 as M
    else:
        from deepfakedetection_amd.fastervit import HipFasterViT as M
    model = M(*args)
    assert _names(model)[id(resolve_target(model))] == want


def test_cam_key_is_off_by_default():
    from deepfakedetection_amd.orchestration.orchestrator import cam_limit, load_config

    config = load_config(ROOT / "config" / "inference_mi355x.yaml")
    for cfg in config["models"].values():
        assert cam_limit(cfg.get("inference") or {}) is None
    assert cam_limit({}) is None and cam_limit({"cam": None}) is None and cam_limit({"cam": False}) is None
    assert cam_limit({"cam": {"limit": 0}}) is None and cam_limit({"cam": {"enabled": False, "limit": 8}}) is None
    assert cam_limit({"cam": {"limit": 64}}) == 64 and cam_limit({"cam": 5}) == 5
    assert cam_limit({"cam": {"limit": "all"}}) >= 2**31 and cam_limit({"cam": True}) >= 2**31


def test_cam_key_survives_config_validation(tmp_path):
    from deepfakedetection_amd.orchestration.orchestrator import cam_limit, load_config

    text = (ROOT / "config" / "inference_mi355x.yaml").read_text().replace(
        "      split: test\n      batch_size: 256\n      num_workers: 8\n      img_size: 224\n",
        "      split: test\n      batch_size: 256\n      num_workers: 8\n      img_size: 224\n      cam: {limit: 64}\n", 1)
    assert "cam: {limit: 64}" in text
    path = tmp_path / "inference.yaml"
    path.write_text(text)
    config = load_config(path)
    assert cam_limit(config["models"]["efficientnet_b3"]["inference"]) == 64
    assert cam_limit(config["models"]["efficientnet_b0"]["inference"]) is None


@pytest.fixture(scope="module")
def lib():
    from deepfakedetection_amd import _lib

    if not _lib.LIB_PATH.exists():
        from deepfakedetection_amd.build import build

        build()
    return _lib.load()


def test_entry_points_reject_bad_arguments_without_a_gpu(lib):
    # every call below is refused before anything is launched
    assert lib.dfd_gradcam_map(None, None, 0, 1, 49, 64, None, None) == -1
    assert lib.dfd_cam_render(None, 1, 7, 7, 224, 224, None, None, None, 0.5, None, None, None, 0, None) == -1
    assert lib.dfd_cam_render_ws(0, 7, 7, 224, 224) == 0
    assert lib.dfd_cam_render_ws(4, 7, 7, 224, 224) == 4 * 7 * 224 * 4
    assert lib.dfd_version() >= 136


def test_gradcam_refuses_a_cpu_model_and_training_mode():
    from deepfakedetection_amd.cam import GradCam
    from deepfakedetection_amd.efficientnet import HipEfficientNet

    model = HipEfficientNet("b0", "timm", 2).eval()
    x = torch.zeros(1, 3, 32, 32)
    with GradCam(model) as cam, pytest.raises(RuntimeError, match="no CPU fallback"):
        cam(x)
    model.train()
    with GradCam(model) as cam, pytest.raises(RuntimeError, match="eval mode"):
        cam(x)
    with pytest.raises(RuntimeError, match="context manager"):
        GradCam(model.eval())(x)
    assert not model.conv_head._forward_hooks                       # every hook removed on exit


def test_entry_points_are_declared_in_the_header():
    header = (ROOT / "include" / "dfd_hip.h").read_text()
    for name in ("dfd_gradcam_map", "dfd_cam_render", "dfd_cam_render_ws"):
        assert f" {name}(" in header
    assert "web_ui.py:275-282" in header
    from deepfakedetection_amd.build import SOURCES

    assert "dfd_cam.hip" in SOURCES
