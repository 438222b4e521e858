"""JPEG-compression augmentation on the device (csrc/dfd_jpeg.hip, dfd_jpeg_u8) against tests/_jpeg_ref.py — which
tests/test_jpeg_cpu.py pins against Pillow — and, through the whole input tail, against the PIL pipeline itself.  Every
comparison is byte for byte."""

from __future__ import annotations

import random

import numpy as np
import pytest
import torch
from PIL import Image

from deepfakedetection_amd import data as D
from tests import _jpeg_ref as J

pytestmark = pytest.mark.gpu

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
SIZES = [(5, 5), (8, 33), (16, 16), (17, 19), (24, 40), (30, 40), (37, 45), (228, 201)]      # (H, W); (224, 224) has its own test
MIX = [(q, f) for q in (0, 1, 50, 75, 100) for f in (0, 1)]


def _k():
    from deepfakedetection_amd import kernels as K

    return K


def _seed(s: int) -> None:
    torch.manual_seed(s); random.seed(s); np.random.seed(s)


def _check(pictures, jobs, ws=None):
    got = _k().jpeg_u8(torch.from_numpy(np.stack(pictures)).cuda(), torch.tensor(jobs, dtype=torch.int32), ws).cpu().numpy()
    for i, (arr, (q, f)) in enumerate(zip(pictures, jobs)):
        want = J.device_jpeg(arr, q, f)
        assert np.array_equal(got[i], want), (i, arr.shape[:2], q, f, int((got[i] != want).sum()), np.argwhere(got[i] != want)[:4].tolist())


@pytest.mark.parametrize("size", SIZES)
def test_kernel_equals_the_reference(size):
    """One batch per size: ten different noise pictures at qualities 0 (copy), 1, 50, 75, 100, each read straight and mirrored, so
    that every picture differs from its neighbour in the batch; 0/255 binary noise at quality 1 (the inverse DCT saturates); a
    constant picture; smoothed noise; and a picture whose only detail is its last row and column (padding)."""
    h, w = size
    rng = np.random.default_rng(h * 1000 + w)
    pictures = [J.pictures(h, w, rng)["noise"] for _ in MIX]
    jobs = list(MIX)
    special = J.pictures(h, w, rng)
    for name, cases in (("binary", [(1, 0), (1, 1), (100, 0)]), ("constant", [(50, 0), (1, 1)]), ("smooth", [(75, 0), (95, 1)]),
                        ("edge", [(1, 0), (1, 1), (75, 0), (75, 1), (100, 0), (100, 1), (0, 1)])):
        for job in cases:
            pictures.append(special[name])
            jobs.append(job)
    _check(pictures, jobs)


def test_kernel_equals_the_reference_at_the_training_size():
    h = w = 224
    rng = np.random.default_rng(224)
    pictures = [J.pictures(h, w, rng)["noise"] for _ in range(4)]
    _check(pictures, [(1, 1), (50, 0), (75, 1), (100, 0)])
    _check(pictures, [(0, 1), (60, 0), (0, 0), (90, 1)])                 # copies between compressed pictures


def test_workspace_query_covers_every_byte_touched():
    """The workspace and the output sit inside larger buffers filled with a pattern: the bands around them stay intact, and the
    caller's own workspace gives the same pictures as one allocated by the wrapper."""
    K = _k()
    n, h, w = 3, 37, 45
    guard = 4096
    rng = np.random.default_rng(7)
    pictures = [J.pictures(h, w, rng)["noise"] for _ in range(n)]
    jobs = [(75, 1), (0, 1), (1, 0)]
    src = torch.from_numpy(np.stack(pictures)).cuda()
    need = K._L().dfd_jpeg_ws(n, h, w)
    assert need == n * (h * w + 2 * 19 * 23)
    big_ws = torch.full((need + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")
    big_out = torch.full((src.numel() + 2 * guard,), 0x5A, dtype=torch.uint8, device="cuda")
    jobs_dev = torch.tensor(jobs, dtype=torch.int32).cuda()
    code = K._L().dfd_jpeg_u8(src.data_ptr(), jobs_dev.data_ptr(), big_ws.data_ptr() + guard, big_out.data_ptr() + guard, n, h, w,
                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert code == 0
    ws_host, out_host = big_ws.cpu(), big_out.cpu()
    assert bool((ws_host[:guard] == 0xA5).all()) and bool((ws_host[guard + need:] == 0xA5).all())
    assert bool((out_host[:guard] == 0x5A).all()) and bool((out_host[guard + src.numel():] == 0x5A).all())
    got = out_host[guard:guard + src.numel()].view(n, h, w, 3).numpy()
    for i in range(n):
        assert np.array_equal(got[i], J.device_jpeg(pictures[i], *jobs[i])), i
    _check(pictures, jobs, ws=torch.empty(need + 100, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="ws must"):
        K.jpeg_u8(src, torch.tensor(jobs, dtype=torch.int32), ws=torch.empty(need - 1, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="host int32"):
        K.jpeg_u8(src, jobs_dev)


def test_whole_tail_equals_the_pil_pipeline_under_one_seed():
    """Rotation, flip, jitter, RandAugment and the compression on a batch of 8 at 32 x 32: the EfficientNet trainer's PIL pipeline
    with RandomJpeg in front of ToTensor, seed for seed; a second replay of a seed gives the same bytes."""
    tail = D.GpuInputTail(MEAN, STD, flip_p=0.5, rotate_degrees=10, jitter=(0.2, 0.2, 0.2, 0.05), rand_augment=(2, 9), jpeg=(0.5, 60, 100))
    pil = D.Compose([D.RandomRotation(10), D.RandomHorizontalFlip(0.5), D.ColorJitter(0.2, 0.2, 0.2, 0.05), D.RandAugment(2, 9),
                     D.RandomJpeg(0.5, (60, 100)), D.ToTensor(), D.Normalize(MEAN, STD)])
    batch = np.random.default_rng(8).integers(0, 256, (8, 32, 32, 3), dtype=np.uint8)
    selected = 0
    for seed in (3, 4, 5):
        _seed(seed)
        want = torch.stack([pil(Image.fromarray(arr)) for arr in batch])
        after = torch.get_rng_state()
        _seed(seed)
        selected += int((tail._draw(8, 32, 32)[4][:, 0] > 0).sum())
        _seed(seed)
        got = tail(torch.from_numpy(batch), "cuda").cpu()
        assert torch.equal(got, want), (seed, float((got - want).abs().max()))
        assert torch.equal(torch.get_rng_state(), after)
        _seed(seed)
        assert torch.equal(tail(torch.from_numpy(batch), "cuda").cpu(), got)
    assert 0 < selected < 24


def test_tail_without_a_policy_hands_the_flip_to_the_compression():
    """No policy: rotation and jitter in dfd_augment_u8, then the flip INSIDE dfd_jpeg_u8 (also for the pictures it only copies),
    and dfd_image_prep flips nothing."""
    K = _k()
    tail = D.GpuInputTail(MEAN, STD, flip_p=0.5, erase_p=0.5, rotate_degrees=10, jitter=(0.2, 0.2, 0.2, 0.05), jpeg=(0.5, 60, 100))
    batch = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (8, 40, 40, 3), dtype=np.uint8))
    _seed(21)
    aug, policy, flip, erase, jpeg = tail._draw(8, 40, 40)
    after = torch.get_rng_state()
    assert policy is None and flip is None and 0 < int(jpeg[:, 1].sum()) < 8 and 0 < int((jpeg[:, 0] > 0).sum()) < 8
    front = K.augment_u8(batch.cuda(), aug.cuda()).cpu().numpy()
    mid = np.stack([J.device_jpeg(front[i], int(jpeg[i, 0]), int(jpeg[i, 1])) for i in range(8)])
    want = K.image_prep(torch.from_numpy(mid).cuda(), MEAN, STD, None, erase.cuda()).cpu()
    _seed(21)
    got = tail(batch, "cuda").cpu()
    assert torch.equal(got, want) and torch.equal(torch.get_rng_state(), after)
    # and with the compression off the tail launches no such kernel
    calls = []
    real = K.jpeg_u8
    K.jpeg_u8 = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        D.GpuInputTail(MEAN, STD, flip_p=0.5, rotate_degrees=10, jitter=(0.2, 0.2, 0.2, 0.05))(batch, "cuda")
        assert not calls
        tail(batch, "cuda")
        assert calls == [1]
    finally:
        K.jpeg_u8 = real
    torch.cuda.synchronize()
