"""JPEG-compression augmentation without a GPU: the numpy restatement of csrc/dfd_jpeg.hip's arithmetic against Pillow byte for
byte, data.RandomJpeg's draws and pixels, and the plumbing (settings, pipelines, the tail's draw order, ABI)."""

from __future__ import annotations

import ctypes
import random

import numpy as np
import pytest
import torch
from PIL import Image, features

from deepfakedetection_amd import data as D
from tests import _jpeg_ref as J

needs_libjpeg = pytest.mark.skipif(not features.check("jpg"), reason="this Pillow was built without libjpeg: there is no JPEG codec to compare with")

SIZES = [(5, 5), (8, 33), (16, 16), (17, 19), (24, 40), (30, 40), (37, 45), (228, 201), (224, 224)]      # (H, W)
QUALITIES = (1, 10, 50, 75, 95, 100)
ENV = ("TRANSFORMS", "RAND_AUGMENT_OPS", "RAND_AUGMENT_MAGNITUDE", "TRIVIAL_AUGMENT", "JPEG_P", "JPEG_QUALITY_MIN", "JPEG_QUALITY_MAX")


def _seed(s: int) -> None:
    torch.manual_seed(s); random.seed(s); np.random.seed(s)


@needs_libjpeg
@pytest.mark.parametrize("size", SIZES)
def test_reference_equals_pillow_byte_for_byte(size):
    h, w = size
    pics = J.pictures(h, w, np.random.default_rng(h * 1000 + w))
    for name in ("noise", "smooth", "binary", "constant"):
        for q in QUALITIES:
            got, want = J.roundtrip(pics[name], q), J.pil_roundtrip(pics[name], q)
            assert np.array_equal(got, want), (size, name, q, int((got != want).sum()))


@needs_libjpeg
def test_reference_padding_cases_equal_pillow():
    """Detail only in the last row and column, at heights and widths on every side of the 8 / 16 block edges, and the mirrored read."""
    rng = np.random.default_rng(5)
    for h, w in ((1, 5), (2, 6), (7, 9), (9, 15), (15, 17), (18, 31), (32, 33), (33, 47), (10, 65)):
        arr = J.pictures(h, w, rng)["edge"]
        for q in (1, 50, 100):
            assert np.array_equal(J.roundtrip(arr, q), J.pil_roundtrip(arr, q)), (h, w, q)
            assert np.array_equal(J.device_jpeg(arr, q, 1), J.pil_roundtrip(np.ascontiguousarray(arr[:, ::-1]), q)), (h, w, q)
        assert np.array_equal(J.device_jpeg(arr, 0, 1), arr[:, ::-1]) and np.array_equal(J.device_jpeg(arr, 0, 0), arr)
    with pytest.raises(ValueError):
        J.roundtrip(np.zeros((8, 4, 3), dtype=np.uint8), 50)


def test_quantisation_tables():
    assert J.quant_table(J.LUMA, 50).ravel().tolist() == list(J.LUMA) and J.quant_table(J.CHROMA, 50).ravel().tolist() == list(J.CHROMA)
    assert (J.quant_table(J.LUMA, 100) == 1).all() and (J.quant_table(J.CHROMA, 1) == 255).all()
    assert J.quant_table(J.LUMA, 75)[0, :4].tolist() == [8, 6, 5, 8] and J.quant_table(J.LUMA, 10)[0, :4].tolist() == [80, 55, 50, 80]


@needs_libjpeg
def test_random_jpeg_draws_and_computes(monkeypatch):
    """Per picture: torch.rand(1) < p, and only for a selected picture torch.randint(lo, hi + 1, (1,)); nothing else is drawn.  The
    result is the reference's round trip at that quality, the untouched picture otherwise."""
    calls = []
    real_rand, real_randint = torch.rand, torch.randint
    monkeypatch.setattr(torch, "rand", lambda *a, **k: (calls.append("rand"), real_rand(*a, **k))[1])
    monkeypatch.setattr(torch, "randint", lambda *a, **k: (calls.append(("randint", a[0], a[1])), real_randint(*a, **k))[1])
    tf = D.RandomJpeg(0.5, quality=(30, 90))
    arr = np.random.default_rng(1).integers(0, 256, (21, 27, 3), dtype=np.uint8)
    img = Image.fromarray(arr)
    _seed(11)
    outs = [np.array(tf(img)) for _ in range(40)]
    after = torch.get_rng_state()
    drawn, calls[:] = list(calls), []
    _seed(11)
    want_calls, qualities = [], []
    for _ in range(40):
        want_calls.append("rand")
        if float(real_rand(1)) < 0.5:
            want_calls.append(("randint", 30, 91))
            qualities.append(int(real_randint(30, 91, (1,))))
        else:
            qualities.append(0)
    assert drawn == want_calls and torch.equal(torch.get_rng_state(), after)
    assert 10 < sum(q > 0 for q in qualities) < 30 and all(q == 0 or 30 <= q <= 90 for q in qualities)
    assert len({q for q in qualities if q}) > 5
    for out, q in zip(outs, qualities):
        assert np.array_equal(out, J.roundtrip(arr, q) if q else arr), q
    assert all(np.array_equal(np.array(D.RandomJpeg(0.0)(img)), arr) for _ in range(5))
    _seed(3)
    one = D.RandomJpeg(1.0, quality=(77, 77))(img)
    assert one.mode == "RGB" and np.array_equal(np.array(one), J.roundtrip(arr, 77))
    narrow = np.random.default_rng(2).integers(0, 256, (9, 3, 3), dtype=np.uint8)       # the PIL transform has no width limit
    assert np.array(D.RandomJpeg(1.0, (50, 50))(Image.fromarray(narrow))).shape == (9, 3, 3)


def test_check_jpeg_errors():
    assert D.check_jpeg(0.5, 60, 100) == (0.5, 60, 100) and D.check_jpeg(1, 1, 1) == (1.0, 1, 1) and D.check_jpeg(0, 100, 100) == (0.0, 100, 100)
    for bad in ((-0.1, 60, 100), (1.1, 60, 100), (0.5, 0, 100), (0.5, 60, 101), (0.5, 80, 60), (0.5, 60.5, 100)):
        with pytest.raises(ValueError, match="RandomJpeg"):
            D.check_jpeg(*bad)
    with pytest.raises(ValueError):
        D.RandomJpeg(0.5, (0, 50))
    with pytest.raises(ValueError):
        D.GpuInputTail([0.0] * 3, [1.0] * 3, jpeg=(2.0, 60, 100))


def test_jpeg_settings_from_the_environment(monkeypatch):
    from deepfakedetection_amd.trainers._inputs import build_transforms, jpeg_settings

    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    assert jpeg_settings() is None
    monkeypatch.setenv("JPEG_P", "0")
    assert jpeg_settings() is None
    monkeypatch.setenv("JPEG_P", "0.5")
    assert jpeg_settings() == (0.5, 60, 100)
    monkeypatch.setenv("JPEG_QUALITY_MIN", "30")
    monkeypatch.setenv("JPEG_QUALITY_MAX", "95")
    assert jpeg_settings() == (0.5, 30, 95)
    monkeypatch.setenv("JPEG_QUALITY_MAX", "20")
    with pytest.raises(ValueError, match="quality"):
        jpeg_settings()
    with pytest.raises(ValueError, match="quality"):
        build_transforms(224)
    monkeypatch.setenv("JPEG_QUALITY_MAX", "95")
    monkeypatch.setenv("JPEG_P", "1.5")
    with pytest.raises(ValueError, match="p must"):
        jpeg_settings()


def test_engine_validates_the_settings_at_start_up():
    import inspect

    from deepfakedetection_amd.trainers import _engine

    assert "jpeg_settings()" in inspect.getsource(_engine.run)


def test_env_round_trip_through_build_env_overrides(tmp_path):
    from deepfakedetection_amd.orchestration.orchestrator import RunPaths, build_env_overrides
    from deepfakedetection_amd.trainers._inputs import jpeg_settings

    model_cfg = {"name": "efficientnet_b0", "output_dir": str(tmp_path / "runs"),
                 "training": {"jpeg_p": 0.25, "jpeg_quality_min": 40, "jpeg_quality_max": 90}}
    run_paths = RunPaths(*(tmp_path / n for n in ("run", "checkpoints", "logs", "plots")))
    env = build_env_overrides(config={}, model_cfg=model_cfg, run_paths=run_paths, training=True)
    assert env["JPEG_P"] == "0.25" and env["JPEG_QUALITY_MIN"] == "40" and env["JPEG_QUALITY_MAX"] == "90"
    with pytest.MonkeyPatch.context() as mp:
        for var in ("JPEG_P", "JPEG_QUALITY_MIN", "JPEG_QUALITY_MAX"):
            mp.setenv(var, env[var])
        assert jpeg_settings() == (0.25, 40, 90)
    env = build_env_overrides(config={}, model_cfg={**model_cfg, "training": {}}, run_paths=run_paths, training=True)
    assert not {"JPEG_P", "JPEG_QUALITY_MIN", "JPEG_QUALITY_MAX"} & set(env)
    env = build_env_overrides(config={}, model_cfg=model_cfg, run_paths=run_paths, training=False)
    assert "JPEG_P" not in env


def test_build_transforms_places_the_compression(monkeypatch):
    from deepfakedetection_amd.trainers._inputs import build_transforms

    for var in ENV:
        monkeypatch.delenv(var, raising=False)

    def kinds(compose):
        return [type(op).__name__ for op in compose.ops]

    # off: no pipeline and no tail knows of it
    assert "RandomJpeg" not in kinds(build_transforms(224)[0])
    for kw in ({}, {"gpu_resize": True}):
        train, val, train_tail, val_tail = build_transforms(224, gpu_tail=True, **kw)
        assert train_tail.jpeg is None and val_tail.jpeg is None and "RandomJpeg" not in kinds(train)
    monkeypatch.setenv("JPEG_P", "0.5")
    # PIL only: directly in front of ToTensor, behind ColorJitter and the policy's slot; never in validation
    train, val = build_transforms(224)
    k = kinds(train)
    assert k[k.index("ColorJitter") + 1] == "RandomJpeg" and k[k.index("RandomJpeg") + 1] == "ToTensor" and "RandomJpeg" not in kinds(val)
    op = train.ops[k.index("RandomJpeg")]
    assert (op.p, op.lo, op.hi) == (0.5, 60, 100)
    monkeypatch.setenv("RAND_AUGMENT_OPS", "2")
    k = kinds(build_transforms(224)[0])
    assert k[k.index("ColorJitter") + 1:k.index("ToTensor") + 1] == ["RandAugment", "RandomJpeg", "ToTensor"]
    k = kinds(build_transforms(224, rotation_default=False, erasing_default=False, rotation_after_flip=True)[0])
    assert k[k.index("RandAugment") + 1:k.index("RandAugment") + 3] == ["RandomJpeg", "ToTensor"]
    # PIL head + GPU tail, with and without a policy: on the device, never in the workers
    for ops in ("2", None):
        monkeypatch.setenv("RAND_AUGMENT_OPS", ops) if ops else monkeypatch.delenv("RAND_AUGMENT_OPS")
        train, val, train_tail, val_tail = build_transforms(224, gpu_tail=True)
        assert "RandomJpeg" not in kinds(train) + kinds(val) and kinds(train)[-1] == "ToUint8HWC"
        assert train_tail.jpeg == (0.5, 60, 100) and val_tail.jpeg is None and train_tail.flip_p == (0.0 if ops else 0.5)
        # everything on the device
        train, val, train_tail, val_tail = build_transforms(224, gpu_tail=True, gpu_resize=True)
        assert kinds(train)[-1] == "PlanGeometry" and "RandomJpeg" not in kinds(train) + kinds(val)
        assert train_tail.jpeg == (0.5, 60, 100) and val_tail.jpeg is None and train_tail.policy == ("rand" if ops else None)
    # too large for the augment kernel's LDS: rotation and jitter go back to the workers, the compression stays on the device
    train, val, train_tail, val_tail = build_transforms(256, gpu_tail=True, gpu_resize=True)
    assert "RandomJpeg" not in kinds(train) and "ColorJitter" in kinds(train) and train_tail.jpeg == (0.5, 60, 100)
    # an explicit argument wins over the environment
    assert build_transforms(224, gpu_tail=True, gpu_resize=True, jpeg=None)[2].jpeg is None
    assert "RandomJpeg" not in kinds(build_transforms(224, jpeg=None)[0])
    assert build_transforms(224, gpu_tail=True, jpeg=(1.0, 5, 9))[2].jpeg == (1.0, 5, 9)


KW = dict(flip_p=0.5, erase_p=0.5, rotate_degrees=10, jitter=(0.2, 0.2, 0.2, 0.05))


def _same(a, b) -> bool:
    return (a is None and b is None) or (a is not None and b is not None and torch.equal(a, b))


@needs_libjpeg
def test_tail_with_a_policy_draws_in_the_pil_pipelines_order(monkeypatch):
    """Angle, flip, jitter, policy, then the compression's two draws, picture by picture: the same generator state and the same
    qualities as the EfficientNet PIL pipeline with RandomJpeg appended."""
    n, h, w = 6, 16, 16
    tail = D.GpuInputTail([0.0] * 3, [1.0] * 3, flip_p=0.5, rotate_degrees=10, jitter=(0.2, 0.2, 0.2, 0.05), rand_augment=(2, 9),
                          jpeg=(0.5, 60, 100))
    pil = D.Compose([D.RandomRotation(10), D.RandomHorizontalFlip(0.5), D.ColorJitter(0.2, 0.2, 0.2, 0.05), D.RandAugment(2, 9),
                     D.RandomJpeg(0.5, (60, 100))])
    drawn = []
    real = D._jpeg_draw
    monkeypatch.setattr(D, "_jpeg_draw", lambda *a: (drawn.append(real(*a)), drawn[-1])[1])
    img = Image.fromarray(np.random.default_rng(0).integers(0, 256, (h, w, 3), dtype=np.uint8))
    for seed in (1, 2, 3):
        _seed(seed)
        for _ in range(n):
            pil(img)
        after, want, drawn[:] = torch.get_rng_state(), list(drawn), []
        _seed(seed)
        aug, policy, flip, erase, jpeg = tail._draw(n, h, w)
        drawn[:] = []
        assert torch.equal(torch.get_rng_state(), after)
        assert aug is None and flip is None and erase is None and tuple(policy.shape) == (n, D.AA_JOB_WORDS)
        assert jpeg.dtype == torch.int32 and jpeg[:, 0].tolist() == want and jpeg[:, 1].tolist() == [0] * n
        _seed(seed)
        assert torch.equal(tail.sample_policy(n, h, w), policy)
        drawn[:] = []
    assert any(want) and not all(want)


def test_tail_without_a_policy_draws_after_the_flips_and_before_the_boxes():
    n, h, w = 16, 24, 24
    tail = D.GpuInputTail([0.0] * 3, [1.0] * 3, jpeg=(0.5, 60, 100), **KW)
    plain = D.GpuInputTail([0.0] * 3, [1.0] * 3, **KW)
    _seed(9)
    aug = plain.sample_augment(n, h, w)
    flips = [1 if D._rand() < 0.5 else 0 for _ in range(n)]
    qualities = [int(torch.randint(60, 101, (1,))) if D._rand() < 0.5 else 0 for _ in range(n)]
    erase = plain._sample_erase(n, h, w)
    after = torch.get_rng_state()
    _seed(9)
    got = tail._draw(n, h, w)
    assert torch.equal(torch.get_rng_state(), after)
    assert torch.equal(got[0], aug) and got[1] is None and got[2] is None and torch.equal(got[3], erase)
    assert got[4].tolist() == [[q, f] for q, f in zip(qualities, flips)]          # the flip flags travel with the qualities
    assert 0 < sum(flips) < n and 0 < sum(q > 0 for q in qualities) < n


@pytest.mark.parametrize("policy", [None, "rand", "trivial"])
def test_tail_without_the_compression_draws_what_it_drew_before(policy):
    n, h, w = 8, 24, 24
    kw = dict(KW, **({"rand_augment": (2, 9)} if policy == "rand" else {"trivial_augment": True} if policy else {}))
    tail = D.GpuInputTail([0.0] * 3, [1.0] * 3, **kw)
    assert tail.jpeg is None
    _seed(4)
    if policy:
        want = (None, tail.sample_policy(n, h, w), None, tail._sample_erase(n, h, w))
    else:
        want = (tail.sample_augment(n, h, w), None, *tail.sample(n, h, w))
    after = torch.get_rng_state()
    _seed(4)
    got = tail._draw(n, h, w)
    assert torch.equal(torch.get_rng_state(), after) and got[4] is None
    assert all(_same(a, b) for a, b in zip(got[:4], want))
    # and a tail with the compression at p = 0 selects nothing
    _seed(4)
    off = D.GpuInputTail([0.0] * 3, [1.0] * 3, jpeg=(0.0, 60, 100), **kw)._draw(n, h, w)
    assert off[4][:, 0].tolist() == [0] * n


def test_abi_142_entry_point_checks_its_arguments_without_a_gpu():
    from deepfakedetection_amd import _lib
    from deepfakedetection_amd.build import SOURCES

    lib = _lib.load()
    assert lib.dfd_version() >= 142 and "dfd_jpeg.hip" in SOURCES
    assert lib.dfd_jpeg_ws(1, 8, 8) == 64 + 2 * 16 and lib.dfd_jpeg_ws(3, 5, 7) == 3 * (35 + 2 * 3 * 4)
    assert lib.dfd_jpeg_ws(256, 224, 224) == 256 * 224 * 224 * 3 // 2
    assert lib.dfd_jpeg_ws(0, 8, 8) == 0 and lib.dfd_jpeg_ws(1, 0, 8) == 0
    jobs = (ctypes.c_int32 * 2)()
    buf, out, ws = (ctypes.c_uint8 * 768)(), (ctypes.c_uint8 * 768)(), (ctypes.c_uint8 * 768)()
    j, s, o, k = (ctypes.addressof(b) for b in (jobs, buf, out, ws))
    assert lib.dfd_jpeg_u8(s, j, k, o, 1, 16, 4, None) == -1                        # DFD_EINVAL: narrower than 5 pixels
    assert lib.dfd_jpeg_u8(s, j, k, o, 0, 16, 16, None) == -1 and lib.dfd_jpeg_u8(s, j, k, o, 1, 0, 16, None) == -1
    for args in ((None, j, k, o), (s, None, k, o), (s, j, None, o), (s, j, k, None)):
        assert lib.dfd_jpeg_u8(*args, 1, 16, 16, None) == -1                        # a null pointer
    assert lib.dfd_jpeg_u8(s, j, k, s, 1, 16, 16, None) == -1                       # src == out


def test_kernel_wrapper_checks_its_arguments_without_a_gpu():
    from deepfakedetection_amd import kernels as K

    src = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    jobs = torch.zeros((2, 2), dtype=torch.int32)
    for bad_src in (src.float(), src[0], src[..., :2], src.permute(0, 2, 1, 3)[:, :, ::2]):
        with pytest.raises(ValueError, match="contiguous uint8"):
            K.jpeg_u8(bad_src, jobs)
    with pytest.raises(ValueError, match="5 pixels"):
        K.jpeg_u8(torch.zeros((2, 8, 4, 3), dtype=torch.uint8), jobs)
    for bad_jobs in (jobs.long(), jobs[:1], torch.zeros((2, 3), dtype=torch.int32), torch.zeros((4, 2), dtype=torch.int32)[::2]):
        with pytest.raises(ValueError, match="host int32"):
            K.jpeg_u8(src, bad_jobs)
    for q, f in ((101, 0), (-1, 0), (50, 2), (50, -1)):
        with pytest.raises(ValueError, match="quality must"):
            K.jpeg_u8(src, torch.tensor([[50, 1], [q, f]], dtype=torch.int32))
    with pytest.raises(ValueError, match="ws must"):
        K.jpeg_u8(src, jobs, ws=torch.zeros(10, dtype=torch.uint8))
