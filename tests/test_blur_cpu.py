"""Gaussian-blur augmentation without a GPU: the numpy reference against Pillow, byte for byte; the plan (the only floating point);
RandomBlur's draws; settings, placement in the pipelines, the tail's draw order, and that nothing changes with blur off."""

from __future__ import annotations

import ctypes
import random

import numpy as np
import pytest
import torch
from PIL import Image, ImageFilter

from deepfakedetection_amd import data as D
from tests import _blur_ref as B

ENV = ("BLUR_P", "BLUR_SIGMA_MIN", "BLUR_SIGMA_MAX", "JPEG_P", "JPEG_QUALITY_MIN", "JPEG_QUALITY_MAX", "RAND_AUGMENT_OPS",
       "RAND_AUGMENT_MAGNITUDE", "TRIVIAL_AUGMENT", "TRANSFORMS")
SIZES = ((1, 1), (1, 7), (7, 1), (2, 3), (3, 200), (5, 7), (63, 65), (228, 228))
SIGMAS = (0, 0.01, 0.1, 0.3, 0.5, 0.577, 0.9, 1, 1.5, 2, 2.5, 3, 4.7, 8, 16)


def _seed(s: int) -> None:
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def _pillow(arr: np.ndarray, sigma: float) -> np.ndarray:
    return np.asarray(Image.fromarray(arr).filter(ImageFilter.GaussianBlur(radius=float(sigma))))


def _pictures(rng, h: int, w: int):
    yield rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yield (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)            # 0 / 255 noise: the largest steps a tap can meet


@pytest.mark.parametrize("size", SIZES)
def test_reference_equals_pillow_byte_for_byte(size):
    h, w = size
    rng = np.random.default_rng(h * 1000 + w)
    sigmas = list(SIGMAS) + rng.uniform(0, 3, 10).tolist()
    for sigma in sigmas:                                                    # sigma 4.7, 8, 16: radii beyond the small pictures
        for arr in _pictures(rng, h, w):
            assert np.array_equal(B.blur(arr, sigma), _pillow(arr, sigma)), (size, sigma)


def test_blur_plan_equals_pillow_on_a_dense_sweep():
    rng = np.random.default_rng(5)
    arr = rng.integers(0, 256, (9, 9, 3), dtype=np.uint8)
    sigmas = np.concatenate([np.linspace(0.0, 16.0, 257), rng.uniform(0, 16, 64), rng.uniform(0, 1, 32)])
    for sigma in sigmas.tolist():
        plan = D.blur_plan(sigma)
        assert plan == B.plan(sigma), sigma
        r, ww, fw = plan
        assert 0 <= r <= 15 and ww > 0 and fw >= 0 and (2 * r + 1) * ww + 2 * fw <= 1 << 24
        assert np.array_equal(B.blur_planned(arr, *plan), _pillow(arr, sigma)), sigma
    assert D.blur_plan(0) == (0, 1 << 24, 0)                               # the identity
    assert D.blur_plan(0.3)[0] == 0 and D.blur_plan(0.3)[2] > 0            # no whole neighbours, fractional ones only
    assert D.blur_plan(16)[0] == 15


def test_constant_pictures_stay_constant_and_sigma_0_is_the_identity():
    rng = np.random.default_rng(2)
    for value in (0, 255):
        arr = np.full((11, 13, 3), value, dtype=np.uint8)
        for sigma in (0, 0.3, 1, 3, 16):
            assert np.array_equal(B.blur(arr, sigma), arr)
    arr = rng.integers(0, 256, (11, 13, 3), dtype=np.uint8)
    assert np.array_equal(B.blur(arr, 0), arr)


def test_blur_commutes_with_the_horizontal_flip():
    rng = np.random.default_rng(3)
    for h, w in ((9, 9), (12, 31), (5, 2)):
        for arr in _pictures(rng, h, w):
            for sigma in (0.3, 1, 2.2, 3, 8):
                assert np.array_equal(np.flip(B.blur(arr, sigma), axis=1), B.blur(np.ascontiguousarray(np.flip(arr, axis=1)), sigma))
                assert np.array_equal(np.flip(_pillow(arr, sigma), axis=1), _pillow(np.ascontiguousarray(np.flip(arr, axis=1)), sigma))


def test_random_blur_draws_and_computes(monkeypatch):
    calls = []
    real_rand, real_uniform = D._rand, D._uniform
    monkeypatch.setattr(D, "_rand", lambda: (calls.append("rand"), real_rand())[1])
    monkeypatch.setattr(D, "_uniform", lambda lo, hi: (calls.append(("uniform", lo, hi)), real_uniform(lo, hi))[1])
    img = Image.fromarray(np.random.default_rng(0).integers(0, 256, (12, 10, 3), dtype=np.uint8))
    op = D.RandomBlur(0.5, (0.5, 2.5))
    blurred = 0
    for seed in range(12):
        _seed(seed)
        calls.clear()
        got = op(img)
        _seed(seed)
        selected = float(torch.rand(1).item()) < 0.5
        if selected:
            sigma = float(torch.empty(1).uniform_(0.5, 2.5).item())
            assert calls == ["rand", ("uniform", 0.5, 2.5)]
            assert np.array_equal(np.asarray(got), _pillow(np.asarray(img), sigma))
            assert np.array_equal(np.asarray(got), B.blur(np.asarray(img), sigma))
            blurred += 1
        else:
            assert calls == ["rand"] and got is img
    assert 0 < blurred < 12
    for seed in range(6):
        _seed(seed)
        calls.clear()
        assert D.RandomBlur(0.0)(img) is img and calls == ["rand"]                     # p = 0 never blurs
        calls.clear()
        assert D.RandomBlur(1.0, (1.0, 3.0))(img) is not img and calls == ["rand", ("uniform", 1.0, 3.0)]   # p = 1 always does
    grey = Image.fromarray(np.random.default_rng(1).integers(0, 256, (8, 8), dtype=np.uint8))
    assert D.RandomBlur(1.0)(grey).mode == "RGB"


def test_check_blur_errors():
    assert D.check_blur(0.5, 0, 3) == (0.5, 0.0, 3.0) and D.check_blur(1, 2, 2) == (1.0, 2.0, 2.0) and D.check_blur(0, 0, 16)[2] == 16.0
    for bad in ((-0.1, 0, 3), (1.5, 0, 3), (0.5, -1, 3), (0.5, 2, 1), (0.5, 0, 16.5), (0.5, 17, 18)):
        with pytest.raises(ValueError):
            D.check_blur(*bad)
    with pytest.raises(ValueError):
        D.RandomBlur(0.5, (3, 1))
    with pytest.raises(ValueError):
        D.GpuInputTail([0.0] * 3, [1.0] * 3, blur=(2.0, 0, 3))


def test_blur_settings_from_the_environment(monkeypatch):
    from deepfakedetection_amd.trainers._inputs import blur_settings, build_transforms

    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    assert blur_settings() is None
    monkeypatch.setenv("BLUR_P", "0")
    assert blur_settings() is None
    monkeypatch.setenv("BLUR_P", "0.5")
    assert blur_settings() == (0.5, 0.0, 3.0)
    monkeypatch.setenv("BLUR_SIGMA_MIN", "0.5")
    monkeypatch.setenv("BLUR_SIGMA_MAX", "2")
    assert blur_settings() == (0.5, 0.5, 2.0)
    monkeypatch.setenv("BLUR_SIGMA_MAX", "0.25")
    with pytest.raises(ValueError, match="sigma"):
        blur_settings()
    with pytest.raises(ValueError, match="sigma"):
        build_transforms(224)
    monkeypatch.setenv("BLUR_SIGMA_MAX", "2")
    monkeypatch.setenv("BLUR_P", "1.5")
    with pytest.raises(ValueError, match="p must"):
        blur_settings()


def test_engine_validates_the_settings_at_start_up():
    import inspect

    from deepfakedetection_amd.trainers import _engine

    assert "blur_settings()" in inspect.getsource(_engine.run)


def test_env_round_trip_through_build_env_overrides(tmp_path):
    from deepfakedetection_amd.orchestration.orchestrator import RunPaths, build_env_overrides
    from deepfakedetection_amd.trainers._inputs import blur_settings

    names = ("BLUR_P", "BLUR_SIGMA_MIN", "BLUR_SIGMA_MAX")
    model_cfg = {"name": "efficientnet_b0", "output_dir": str(tmp_path / "runs"),
                 "training": {"blur_p": 0.25, "blur_sigma_min": 0.5, "blur_sigma_max": 2.5}}
    run_paths = RunPaths(*(tmp_path / n for n in ("run", "checkpoints", "logs", "plots")))
    env = build_env_overrides(config={}, model_cfg=model_cfg, run_paths=run_paths, training=True)
    assert [env[v] for v in names] == ["0.25", "0.5", "2.5"]
    with pytest.MonkeyPatch.context() as mp:
        for var in names:
            mp.setenv(var, env[var])
        assert blur_settings() == (0.25, 0.5, 2.5)
    env = build_env_overrides(config={}, model_cfg={**model_cfg, "training": {}}, run_paths=run_paths, training=True)
    assert not set(names) & set(env)
    env = build_env_overrides(config={}, model_cfg=model_cfg, run_paths=run_paths, training=False)
    assert "BLUR_P" not in env


def test_build_transforms_places_the_blur(monkeypatch):
    from deepfakedetection_amd.trainers._inputs import build_transforms

    for var in ENV:
        monkeypatch.delenv(var, raising=False)

    def kinds(compose):
        return [type(op).__name__ for op in compose.ops]

    # off: no pipeline and no tail knows of it
    assert "RandomBlur" not in kinds(build_transforms(224)[0])
    for kw in ({}, {"gpu_resize": True}):
        train, val, train_tail, val_tail = build_transforms(224, gpu_tail=True, **kw)
        assert train_tail.blur is None and val_tail.blur is None and "RandomBlur" not in kinds(train)
    monkeypatch.setenv("BLUR_P", "0.5")
    monkeypatch.setenv("JPEG_P", "0.5")
    monkeypatch.setenv("RAND_AUGMENT_OPS", "2")
    # branch 1, PIL only: behind the policy, in front of the compression; never in validation
    for kw in ({}, dict(rotation_default=False, erasing_default=False, rotation_after_flip=True)):
        train, val = build_transforms(224, **kw)
        k = kinds(train)
        assert k[k.index("RandAugment") + 1:k.index("RandAugment") + 4] == ["RandomBlur", "RandomJpeg", "ToTensor"]
        assert "RandomBlur" not in kinds(val)
    op = train.ops[k.index("RandomBlur")]
    assert (op.p, op.lo, op.hi) == (0.5, 0.0, 3.0)
    monkeypatch.delenv("RAND_AUGMENT_OPS")
    k = kinds(build_transforms(224)[0])
    assert k[k.index("ColorJitter") + 1:k.index("ColorJitter") + 3] == ["RandomBlur", "RandomJpeg"]
    # branch 2, PIL head + GPU tail: on the device while one picture fits, with and without a policy
    for ops in ("2", None):
        monkeypatch.setenv("RAND_AUGMENT_OPS", ops) if ops else monkeypatch.delenv("RAND_AUGMENT_OPS")
        train, val, train_tail, val_tail = build_transforms(224, gpu_tail=True)
        assert "RandomBlur" not in kinds(train) + kinds(val) and kinds(train)[-1] == "ToUint8HWC"
        assert train_tail.blur == (0.5, 0.0, 3.0) and train_tail.jpeg == (0.5, 60, 100) and val_tail.blur is None
        # ... and in the workers, behind the policy and in front of ToUint8HWC, when it does not
        train, val, train_tail, val_tail = build_transforms(256, gpu_tail=True)
        k = kinds(train)
        assert k[-2:] == ["RandomBlur", "ToUint8HWC"] and k[-3] == ("RandAugment" if ops else "ColorJitter")
        assert train_tail.blur is None and train_tail.jpeg == (0.5, 60, 100) and "RandomBlur" not in kinds(val)
        # branch 3, everything on the device: behind the policy and in front of the compression inside the tail
        train, val, train_tail, val_tail = build_transforms(224, gpu_tail=True, gpu_resize=True)
        assert kinds(train)[-1] == "PlanGeometry" and "RandomBlur" not in kinds(train) + kinds(val)
        assert train_tail.blur == (0.5, 0.0, 3.0) and train_tail.jpeg == (0.5, 60, 100) and val_tail.blur is None
        assert train_tail.policy == ("rand" if ops else None)
    # blur counts like rotation, jitter and a policy: alone it keeps a picture too large for the LDS off the device plan
    monkeypatch.setenv("TRANSFORMS", '{"train_random_rotation": false, "train_color_jitter": false}')
    train, val, train_tail, val_tail = build_transforms(256, gpu_tail=True, gpu_resize=True)
    assert kinds(train)[-2:] == ["RandomBlur", "ToUint8HWC"] and train_tail.blur is None
    train, val, train_tail, val_tail = build_transforms(256, gpu_tail=True, gpu_resize=True, blur=None)
    assert kinds(train)[-1] == "PlanGeometry"
    monkeypatch.delenv("TRANSFORMS")
    # an explicit argument wins over the environment
    assert build_transforms(224, gpu_tail=True, gpu_resize=True, blur=None)[2].blur is None
    assert "RandomBlur" not in kinds(build_transforms(224, blur=None)[0])
    assert build_transforms(224, gpu_tail=True, blur=(1.0, 1, 2))[2].blur == (1.0, 1.0, 2.0)


KW = dict(flip_p=0.5, erase_p=0.5, rotate_degrees=10, jitter=(0.2, 0.2, 0.2, 0.05))


def _jobs_of(sigmas) -> list[list[int]]:
    return [[*D.blur_plan(s), 0] if s is not None else [0, 0, 0, 0] for s in sigmas]


def test_tail_with_a_policy_draws_in_the_pil_pipelines_order(monkeypatch):
    """Angle, flip, jitter, policy, blur, compression, picture by picture: the same generator state, sigmas and qualities as the
    EfficientNet PIL pipeline with RandomBlur and RandomJpeg appended."""
    n, h, w = 6, 16, 16
    tail = D.GpuInputTail([0.0] * 3, [1.0] * 3, flip_p=0.5, rotate_degrees=10, jitter=(0.2, 0.2, 0.2, 0.05), rand_augment=(2, 9),
                          blur=(0.5, 0, 3), jpeg=(0.5, 60, 100))
    pil = D.Compose([D.RandomRotation(10), D.RandomHorizontalFlip(0.5), D.ColorJitter(0.2, 0.2, 0.2, 0.05), D.RandAugment(2, 9),
                     D.RandomBlur(0.5, (0, 3)), D.RandomJpeg(0.5, (60, 100))])
    order = []
    real_blur, real_jpeg = D._blur_draw, D._jpeg_draw
    monkeypatch.setattr(D, "_blur_draw", lambda *a: (order.append(("blur", real_blur(*a))), order[-1][1])[1])
    monkeypatch.setattr(D, "_jpeg_draw", lambda *a: (order.append(("jpeg", real_jpeg(*a))), order[-1][1])[1])
    img = Image.fromarray(np.random.default_rng(0).integers(0, 256, (h, w, 3), dtype=np.uint8))
    some = False
    for seed in (1, 2, 3):
        _seed(seed)
        order.clear()
        for _ in range(n):
            pil(img)
        after, want = torch.get_rng_state(), list(order)
        assert [k for k, _ in want] == ["blur", "jpeg"] * n
        _seed(seed)
        order.clear()
        aug, policy, flip, erase, jpeg, blur = tail._draw_all(n, h, w)
        assert torch.equal(torch.get_rng_state(), after) and order == want
        assert aug is None and flip is None and erase is None and tuple(policy.shape) == (n, D.AA_JOB_WORDS)
        sigmas = [v for k, v in want if k == "blur"]
        assert blur.dtype == torch.int32 and blur.tolist() == _jobs_of(sigmas)
        assert jpeg[:, 0].tolist() == [v for k, v in want if k == "jpeg"] and jpeg[:, 1].tolist() == [0] * n
        some |= 0 < sum(s is not None for s in sigmas) < n
        # the five- and two-valued forms the existing callers unpack are the same draws
        _seed(seed)
        five = tail._draw(n, h, w)
        assert len(five) == 5 and torch.equal(five[1], policy) and torch.equal(five[4], jpeg)
        _seed(seed)
        two = tail._sample_policy(n, h, w)
        assert len(two) == 2 and torch.equal(two[0], policy) and torch.equal(two[1], jpeg)
    assert some


@pytest.mark.parametrize("with_jpeg", [False, True])
def test_tail_without_a_policy_draws_after_the_flips_and_before_the_compression(with_jpeg):
    n, h, w = 16, 24, 24
    tail = D.GpuInputTail([0.0] * 3, [1.0] * 3, blur=(0.5, 0, 3), jpeg=(0.5, 60, 100) if with_jpeg else None, **KW)
    plain = D.GpuInputTail([0.0] * 3, [1.0] * 3, **KW)
    _seed(9)
    aug = plain.sample_augment(n, h, w)
    flips = [1 if D._rand() < 0.5 else 0 for _ in range(n)]
    sigmas = [D._uniform(0.0, 3.0) if D._rand() < 0.5 else None for _ in range(n)]
    qualities = [int(torch.randint(60, 101, (1,))) if D._rand() < 0.5 else 0 for _ in range(n)] if with_jpeg else None
    erase = plain._sample_erase(n, h, w)
    after = torch.get_rng_state()
    _seed(9)
    got = tail._draw_all(n, h, w)
    assert torch.equal(torch.get_rng_state(), after) and len(got) == 6
    assert torch.equal(got[0], aug) and got[1] is None and torch.equal(got[3], erase)
    assert got[5].tolist() == _jobs_of(sigmas)
    if with_jpeg:
        assert got[2] is None and got[4].tolist() == [[q, f] for q, f in zip(qualities, flips)]      # the flip goes with the qualities
    else:
        assert got[4] is None and got[2].tolist() == flips                                             # the flip stays with dfd_image_prep
    assert 0 < sum(flips) < n and 0 < sum(s is not None for s in sigmas) < n


# GpuInputTail(jpeg=(0.5, 60, 100), flip_p=0.5, erase_p=0.5, rotate_degrees=10, jitter=(0.2, 0.2, 0.2, 0.05))._draw(4, 24, 24) after
# torch.manual_seed(11), recorded from the commit before blur existed
RECORDED_AUG = [[1, 65045, 8009, -53682, -8009, 65045, 130515, 3, 1, 0, 2, 1065632003, 1066002827, 1062859704, 2, 15],
                [1, 65515, -1650, 51979, 1650, 65515, 14035, 3, 2, 1, 0, 1065361356, 1066249559, 1065106469, 250, 15],
                [1, 64906, 9064, -64226, -9064, 64906, 144249, 1, 2, 3, 0, 1065628442, 1066597761, 1066101665, 9, 15],
                [1, 65076, -7748, 127151, 7748, 65076, -51044, 1, 2, 3, 0, 1063089111, 1063757192, 1065789661, 10, 15]]
RECORDED_ERASE = [[18, 9, 5, 9], [9, 8, 7, 16], [15, 15, 8, 9], [0, 0, 0, 0]]
RECORDED_JPEG = [[0, 1], [79, 1], [75, 0], [0, 1]]
RECORDED_NEXT = 192864752               # int(torch.randint(0, 1 << 30, (1,))) straight after: the generator stands where it stood


def test_tail_without_blur_draws_what_it_drew_before():
    tail = D.GpuInputTail([0.0] * 3, [1.0] * 3, jpeg=(0.5, 60, 100), **KW)
    assert tail.blur is None
    torch.manual_seed(11)
    got = tail._draw(4, 24, 24)
    assert len(got) == 5
    aug, policy, flip, erase, jpeg = got
    assert aug.tolist() == RECORDED_AUG and policy is None and flip is None
    assert erase.tolist() == RECORDED_ERASE and jpeg.tolist() == RECORDED_JPEG
    assert int(torch.randint(0, 1 << 30, (1,))) == RECORDED_NEXT
    torch.manual_seed(11)
    assert tail._draw_all(4, 24, 24)[5] is None
    # and with a policy (recorded likewise, 3 pictures): the same five values, the pair of _sample_policy, no blur jobs
    tail = D.GpuInputTail([0.0] * 3, [1.0] * 3, jpeg=(0.5, 60, 100), rand_augment=(2, 9), **KW)
    torch.manual_seed(11)
    aug, policy, flip, erase, jpeg = tail._draw(3, 24, 24)
    assert aug is None and flip is None and policy[:, :7].tolist() == [[1, 65045, 8009, -53682, -8009, 65045, 130515],
                                                                        [1, 65536, -55, 33406, 55, 65536, 32130],
                                                                        [1, 65468, -2975, 67752, 2975, 65468, -662]]
    assert erase.tolist() == [[0, 10, 12, 9], [5, 14, 13, 8], [0, 2, 9, 16]] and jpeg.tolist() == [[86, 0], [62, 0], [68, 0]]
    assert int(torch.randint(0, 1 << 30, (1,))) == 651445531
    torch.manual_seed(11)
    pair = tail._sample_policy(3, 24, 24)
    assert len(pair) == 2 and torch.equal(pair[0], policy) and torch.equal(pair[1], jpeg)
    # a tail with blur at p = 0 selects nothing
    off = D.GpuInputTail([0.0] * 3, [1.0] * 3, blur=(0.0, 0, 3), **KW)._draw_all(4, 24, 24)
    assert off[5].tolist() == [[0, 0, 0, 0]] * 4


def test_tail_launches_nothing_new_with_blur_off(monkeypatch):
    from deepfakedetection_amd import kernels as K

    launched = []
    for name in ("augment_u8", "augment_policy_u8", "blur_u8", "jpeg_u8"):
        monkeypatch.setattr(K, name, lambda dev, jobs, _n=name: (launched.append(_n), dev)[1])
    monkeypatch.setattr(K, "image_prep", lambda dev, mean, std, flip, erase: (launched.append(("image_prep", flip is not None)), dev)[1])
    batch = torch.zeros((4, 8, 8, 3), dtype=torch.uint8)
    _seed(0)
    D.GpuInputTail([0.0] * 3, [1.0] * 3, jpeg=(0.5, 60, 100), **KW)(batch, "cpu")
    assert launched == ["augment_u8", "jpeg_u8", ("image_prep", False)]
    launched.clear()
    D.GpuInputTail([0.0] * 3, [1.0] * 3, blur=(0.5, 0, 3), jpeg=(0.5, 60, 100), **KW)(batch, "cpu")
    assert launched == ["augment_u8", "blur_u8", "jpeg_u8", ("image_prep", False)]
    launched.clear()
    D.GpuInputTail([0.0] * 3, [1.0] * 3, blur=(0.5, 0, 3), **KW)(batch, "cpu")
    assert launched == ["augment_u8", "blur_u8", ("image_prep", True)]       # the blur commutes with the flip: it stays in the last kernel
    launched.clear()
    D.GpuInputTail([0.0] * 3, [1.0] * 3, blur=(0.5, 0, 3), jpeg=(0.5, 60, 100), rand_augment=(2, 9), **KW)(batch, "cpu")
    assert launched == ["augment_policy_u8", "blur_u8", "jpeg_u8", ("image_prep", False)]


def test_robustness_levels_and_tails():
    from deepfakedetection_amd.orchestration import orchestrator as O

    assert O.robustness_levels({}) == [] and O.robustness_levels({"robustness": None}) == []
    assert O.robustness_levels({"robustness": {"blur_sigma": [1, 2.5], "jpeg_quality": [90, 50]}}) == \
        [("blur_sigma", 1.0), ("blur_sigma", 2.5), ("jpeg_quality", 90), ("jpeg_quality", 50)]
    assert O.robustness_levels({"robustness": {"jpeg_quality": [70]}}) == [("jpeg_quality", 70)]
    for bad in ({"blur_sigma": [17]}, {"blur_sigma": [-1]}, {"jpeg_quality": [0]}, {"jpeg_quality": [101]}):
        with pytest.raises(ValueError):
            O.robustness_levels({"robustness": bad})
    tail = O.robustness_tail("blur_sigma", 2.0)
    assert tail.blur == (1.0, 2.0, 2.0) and tail.jpeg is None and tail.flip_p == 0 and tail.erase_p == 0 and not tail.augments
    _seed(0)
    assert tail._draw_all(3, 8, 8)[5].tolist() == [[*D.blur_plan(2.0), 0]] * 3        # every picture, the one level, under any seed
    tail = O.robustness_tail("jpeg_quality", 70)
    assert tail.jpeg == (1.0, 70, 70) and tail.blur is None
    assert tail._draw(3, 8, 8)[4].tolist() == [[70, 0]] * 3
    import inspect

    assert inspect.signature(O.class_probabilities).parameters["tail"].default is None


def test_abi_144_entry_point_checks_its_arguments_without_a_gpu():
    from deepfakedetection_amd import _lib
    from deepfakedetection_amd.build import SOURCES

    lib = _lib.load()
    assert lib.dfd_version() >= 144 and "dfd_blur.hip" in SOURCES
    assert _lib.BLUR_MAX_PIXELS >= 228 * 228 and _lib.BLUR_MAX_RADIUS >= D.blur_plan(D.BLUR_MAX_SIGMA)[0]
    header = (_lib.LIB_PATH.parent.parent / "include" / "dfd_hip.h").read_text()
    assert f"#define DFD_BLUR_MAX_RADIUS {_lib.BLUR_MAX_RADIUS}\n" in header and "#define DFD_BLUR_MAX_PIXELS (78 * 1024)\n" in header
    assert _lib.BLUR_MAX_PIXELS == 78 * 1024
    jobs = (ctypes.c_int32 * 4)()
    buf, out = (ctypes.c_uint8 * 768)(), (ctypes.c_uint8 * 768)()
    j, s, o = (ctypes.addressof(b) for b in (jobs, buf, out))
    for args in ((None, j, o), (s, None, o), (s, j, None)):
        assert lib.dfd_blur_u8(*args, 1, 16, 16, None) == -1                           # DFD_EINVAL: a null pointer
    assert lib.dfd_blur_u8(s, j, s, 1, 16, 16, None) == -1                             # src == out
    for n, h, w in ((0, 16, 16), (1, 0, 16), (1, 16, 0), (-1, 16, 16)):
        assert lib.dfd_blur_u8(s, j, o, n, h, w, None) == -1
    assert lib.dfd_blur_u8(s, j, o, 1, 1, _lib.BLUR_MAX_PIXELS + 1, None) == -1        # one pixel too many
    assert lib.dfd_blur_u8(s, j, o, 1, 65536, 65536, None) == -1                       # H * W does not wrap


def test_kernel_wrapper_checks_its_arguments_without_a_gpu():
    from deepfakedetection_amd import _lib
    from deepfakedetection_amd import kernels as K

    src = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    jobs = torch.zeros((2, 4), dtype=torch.int32)
    for bad_src in (src.float(), src[0], src[..., :2], src.permute(0, 2, 1, 3)[:, :, ::2]):
        with pytest.raises(ValueError, match="contiguous uint8"):
            K.blur_u8(bad_src, jobs)
    for bad_jobs in (jobs.long(), jobs[:1], torch.zeros((2, 3), dtype=torch.int32), torch.zeros((4, 4), dtype=torch.int32)[::2]):
        with pytest.raises(ValueError, match="host int32"):
            K.blur_u8(src, bad_jobs)
    with pytest.raises(ValueError, match="at most"):
        K.blur_u8(torch.zeros((1, 1, _lib.BLUR_MAX_PIXELS + 1, 3), dtype=torch.uint8), jobs[:1])
