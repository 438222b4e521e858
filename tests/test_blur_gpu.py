"""Gaussian-blur augmentation on the device (csrc/dfd_blur.hip, dfd_blur_u8) against tests/_blur_ref.py — which
tests/test_blur_cpu.py pins against Pillow — through the whole input tail against the PIL pipeline itself, and through the
robustness pass of the inference orchestrator.  Every comparison is byte for byte."""

from __future__ import annotations

import json
import random
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image, ImageFilter

from deepfakedetection_amd import _lib
from deepfakedetection_amd import data as D
from tests import _blur_ref as B

pytestmark = pytest.mark.gpu

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
SIZES = [(1, 1), (1, 9), (9, 1), (5, 7), (63, 65), (228, 228)]          # (H, W); 63 x 65: wave tails in both directions
GUARD = 4096


def _k():
    from deepfakedetection_amd import kernels as K

    return K


def _seed(s: int) -> None:
    torch.manual_seed(s); random.seed(s); np.random.seed(s)


def _jobs(outside: int) -> list[list[int]]:
    """Copy-through; r = 0 identity; sigma 0.3 (r = 0, fw > 0); sigma 3; sigma 16 (r = 15); a radius outside the range with
    otherwise valid weights (copied)."""
    r3, ww3, fw3 = D.blur_plan(3.0)
    jobs = [[0, 0, 0, 0], [0, 1 << 24, 0, 0], [*D.blur_plan(0.3), 0], [r3, ww3, fw3, 0], [*D.blur_plan(16.0), 0], [outside, ww3, fw3, 0]]
    assert jobs[2][0] == 0 and jobs[2][2] > 0 and jobs[4][0] == 15
    return jobs


def _want(arr: np.ndarray, job: list[int]) -> np.ndarray:
    r, ww, fw, _ = job
    return arr if ww == 0 or not 0 <= r <= _lib.BLUR_MAX_RADIUS else B.blur_planned(arr, r, ww, fw)


@pytest.mark.parametrize("size", SIZES)
def test_kernel_equals_the_reference(size):
    """One call of six mixed jobs per input: random bytes and 0/255 noise alternate over the batch, and a second call swaps them, so
    every job meets both.  The output is an interior slice of a buffer filled with 0xAA whose bands must stay intact, and the
    source must not change."""
    K = _k()
    h, w = size
    rng = np.random.default_rng(h * 1000 + w)
    noise = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(6)]
    binary = [(rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8) for _ in range(6)]
    for swap, outside in ((0, _lib.BLUR_MAX_RADIUS + 1), (1, -1)):
        pictures = [(binary if (i + swap) % 2 else noise)[i] for i in range(6)]
        jobs = _jobs(outside)
        host = np.stack(pictures)
        src = torch.from_numpy(host).cuda()
        big = torch.full((src.numel() + 2 * GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
        jobs_dev = torch.tensor(jobs, dtype=torch.int32).cuda()
        code = K._L().dfd_blur_u8(src.data_ptr(), jobs_dev.data_ptr(), big.data_ptr() + GUARD, 6, h, w,
                                  torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert code == 0
        out = big.cpu()
        assert bool((out[:GUARD] == 0xAA).all()) and bool((out[GUARD + src.numel():] == 0xAA).all())
        assert np.array_equal(src.cpu().numpy(), host)
        got = out[GUARD:GUARD + src.numel()].view(6, h, w, 3).numpy()
        for i in range(6):
            want = _want(pictures[i], jobs[i])
            assert np.array_equal(got[i], want), (size, swap, i, jobs[i], int((got[i] != want).sum()), np.argwhere(got[i] != want)[:4].tolist())
        assert np.array_equal(K.blur_u8(src, torch.tensor(jobs, dtype=torch.int32)).cpu().numpy(), got)      # the wrapper: same bytes


def test_a_picture_one_pixel_too_large_is_refused_before_any_launch():
    K = _k()
    w = _lib.BLUR_MAX_PIXELS + 1
    src = torch.zeros((1, 1, w, 3), dtype=torch.uint8, device="cuda")
    out = torch.full((1, 1, w, 3), 0xAA, dtype=torch.uint8, device="cuda")
    jobs_dev = torch.tensor([[*D.blur_plan(1.0), 0]], dtype=torch.int32).cuda()
    code = K._L().dfd_blur_u8(src.data_ptr(), jobs_dev.data_ptr(), out.data_ptr(), 1, 1, w, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert code == -1 and bool((out == 0xAA).all())                        # DFD_EINVAL, nothing written
    with pytest.raises(ValueError, match="at most"):
        K.blur_u8(src, torch.zeros((1, 4), dtype=torch.int32))
    with pytest.raises(ValueError, match="host int32"):
        K.blur_u8(src[:, :, :8].contiguous(), jobs_dev)


@pytest.mark.parametrize("with_jpeg", [True, False])
def test_whole_tail_equals_the_pil_pipeline_under_one_seed(with_jpeg, monkeypatch):
    """Rotation, flip, jitter, RandAugment, blur and the compression on 8 pictures at 40 x 40: the EfficientNet trainer's PIL pipeline
    with RandomBlur and RandomJpeg in front of ToTensor, seed for seed and picture by picture."""
    jpeg = dict(jpeg=(0.5, 60, 100)) if with_jpeg else {}
    tail = D.GpuInputTail(MEAN, STD, flip_p=0.5, rotate_degrees=10, jitter=(0.2, 0.2, 0.2, 0.05), rand_augment=(2, 9), blur=(0.5, 0, 3),
                          **jpeg)
    pil = D.Compose([D.RandomRotation(10), D.RandomHorizontalFlip(0.5), D.ColorJitter(0.2, 0.2, 0.2, 0.05), D.RandAugment(2, 9),
                     D.RandomBlur(0.5, (0, 3)), *([D.RandomJpeg(0.5, (60, 100))] if with_jpeg else []), D.ToTensor(),
                     D.Normalize(MEAN, STD)])
    batch = np.random.default_rng(8).integers(0, 256, (8, 40, 40, 3), dtype=np.uint8)
    seed = 3
    _seed(seed)
    want = torch.stack([pil(Image.fromarray(arr)) for arr in batch])
    after = torch.get_rng_state()
    _seed(seed)
    blurred = int((tail._draw_all(8, 40, 40)[5][:, 1] > 0).sum())
    assert 0 < blurred < 8
    _seed(seed)
    got = tail(torch.from_numpy(batch), "cuda").cpu()
    assert torch.equal(torch.get_rng_state(), after)
    for i in range(8):
        assert torch.equal(got[i], want[i]), (i, float((got[i] - want[i]).abs().max()))


@pytest.mark.parametrize("with_jpeg", [False, True])
def test_tail_without_a_policy_blurs_before_the_flip(with_jpeg, monkeypatch):
    """No policy: rotation and jitter in dfd_augment_u8, the blur of the selected pictures, and the flip where it is without
    blur: in dfd_image_prep, or with the compression on in dfd_jpeg_u8 — against Pillow's own flip, blur, JPEG round trip,
    ToTensor and Normalize on what the first kernel gave, with the draws of the seed: augment jobs, the flips of the batch, the
    blur's draws, then the compression's."""
    import io

    K = _k()
    kw = dict(flip_p=0.5, rotate_degrees=10, jitter=(0.2, 0.2, 0.2, 0.05))
    tail = D.GpuInputTail(MEAN, STD, blur=(0.5, 0, 3), jpeg=(0.5, 60, 100) if with_jpeg else None, **kw)
    batch = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (8, 40, 40, 3), dtype=np.uint8))
    seed = 21
    _seed(seed)
    aug = D.GpuInputTail(MEAN, STD, **kw).sample_augment(8, 40, 40)
    flips = [1 if D._rand() < 0.5 else 0 for _ in range(8)]
    sigmas = [D._uniform(0.0, 3.0) if D._rand() < 0.5 else None for _ in range(8)]
    qualities = [int(torch.randint(60, 101, (1,))) if D._rand() < 0.5 else 0 for _ in range(8)] if with_jpeg else [0] * 8
    after = torch.get_rng_state()
    assert 0 < sum(flips) < 8 and 0 < sum(s is not None for s in sigmas) < 8
    front = K.augment_u8(batch.cuda(), aug.cuda()).cpu().numpy()
    finish = D.Compose([D.ToTensor(), D.Normalize(MEAN, STD)])
    want = []
    for i in range(8):
        img = Image.fromarray(front[i])
        if flips[i]:
            img = img.transpose(Image.FLIP_LEFT_RIGHT)                      # the PIL pipeline's place for it: in front of the blur
        if sigmas[i] is not None:
            img = img.filter(ImageFilter.GaussianBlur(radius=sigmas[i]))
        if qualities[i]:
            buf = io.BytesIO()
            img.save(buf, "JPEG", quality=qualities[i])
            buf.seek(0)
            img = Image.open(buf).convert("RGB")
        want.append(finish(img))
    seen = []
    real = K.image_prep
    monkeypatch.setattr(K, "image_prep", lambda dev, mean, std, flip, erase: (seen.append(flip), real(dev, mean, std, flip, erase))[1])
    _seed(seed)
    got = tail(batch, "cuda").cpu()
    assert torch.equal(torch.get_rng_state(), after) and len(seen) == 1
    if with_jpeg:
        assert seen[0] is None and 0 < sum(q > 0 for q in qualities) < 8                           # dfd_jpeg_u8 flipped
    else:
        assert seen[0] is not None and seen[0].cpu().tolist() == flips                             # dfd_image_prep still gets the flip
    for i in range(8):
        assert torch.equal(got[i], want[i]), (i, float((got[i] - want[i]).abs().max()))


def _write_pngs(root: Path) -> None:
    rng = np.random.default_rng(5)
    for cls in ("fake", "real"):
        folder = root / "test" / cls
        folder.mkdir(parents=True)
        for i in range(4):
            Image.fromarray(rng.integers(0, 256, size=(24, 24, 3), dtype=np.uint8)).save(folder / f"{cls}_{i}.png")


def _config(tmp_path: Path, out: str, robustness: dict | None, gpu_resize: bool = True) -> Path:
    import yaml

    infer = {"split": "test", "batch_size": 8, "num_workers": 0, "img_size": 64, "gpu_resize": gpu_resize}
    if robustness is not None:
        infer["robustness"] = robustness
    cfg = {"seed": 1, "device": "cuda", "data": {"root": str(tmp_path / "data"), "test_split": "test", "num_classes": 2, "img_size": 64},
           "models": {"efficientnet_b0": {"output_dir": str(tmp_path / out), "inference": infer}}, "selection": ["efficientnet_b0"]}
    path = tmp_path / f"{out}.yaml"
    path.write_text(yaml.safe_dump(cfg))
    return path


def _rows(base: Path) -> list[dict]:
    (run,) = [p for p in base.iterdir() if p.is_dir()]
    return [{k: v for k, v in json.loads(s).items() if k != "timestamp"} for s in (run / "logs" / "metrics.jsonl").read_text().splitlines()]


def test_robustness_pass_appends_one_line_per_level(tmp_path, capsys):
    from deepfakedetection_amd.orchestration.orchestrator import orchestrate

    _write_pngs(tmp_path / "data")
    orchestrate(_config(tmp_path, "plain", None), mode="inference")
    plain_text = capsys.readouterr().out
    orchestrate(_config(tmp_path, "robust", {"blur_sigma": [0, 2], "jpeg_quality": [100, 50]}), mode="inference")
    robust_text = capsys.readouterr().out
    plain, rows = _rows(tmp_path / "plain"), _rows(tmp_path / "robust")
    assert len(plain) == 1 and "perturbation" not in plain[0] and "Robustness" not in plain_text
    assert len(rows) == 5 and rows[0] == plain[0]
    assert [row["perturbation"] for row in rows[1:]] == [{"blur_sigma": 0.0}, {"blur_sigma": 2.0}, {"jpeg_quality": 100}, {"jpeg_quality": 50}]
    for row in rows[1:]:
        assert set(row) == set(plain[0]) | {"perturbation"} and row["threshold"] == plain[0]["threshold"]
        assert 0.0 <= row["accuracy"] <= 1.0 and np.asarray(row["confusion_matrix"]).sum() == 8
    clean = {k: v for k, v in rows[1].items() if k != "perturbation"}
    assert clean == plain[0]                                                # sigma 0 is the identity in bytes: the clean pass again
    assert robust_text.count("Robustness") == 4
    # without the device pipeline the pass is skipped with one warning line
    orchestrate(_config(tmp_path, "skipped", {"blur_sigma": [2]}, gpu_resize=False), mode="inference")
    assert "inference.robustness skipped" in capsys.readouterr().out and len(_rows(tmp_path / "skipped")) == 1
