"""Mixup / CutMix without a GPU: the box arithmetic, the job tables of the three modes, the YAML -> environment mapping
and the trainers' reading of it, and the argument checks of dfd_mix_batch / dfd_ce_loss_soft (no device touched)."""

from __future__ import annotations

import ctypes
from pathlib import Path

import numpy as np
import pytest
import torch

from deepfakedetection_amd import _lib
from deepfakedetection_amd._lib import MIX_CUTMIX, MIX_JOB_WORDS, MIX_KEEP, MIX_MIXUP
from deepfakedetection_amd.mix import BatchMixer, Decision, cutmix_box, job_row
from tests import _mix_ref as R

_MIX_VARS = ("MIXUP_ALPHA", "CUTMIX_ALPHA", "MIX_PROB", "MIX_SWITCH_PROB", "MIX_MODE")


def test_box_worked_case_and_limits():
    assert cutmix_box(0.75, 10, 200, 224, 224) == (0, 66, 144, 224, 1 - 5280 / 50176)
    y0, y1, x0, x1, lam = cutmix_box(1.0, 100, 100, 224, 224)          # lam = 1: empty box, nothing is replaced
    assert y1 == y0 and x1 == x0 and lam == 1.0
    for lam in (0.0, 1e-20):                                           # 1 - lam rounds to 1: the box is the whole picture
        assert cutmix_box(lam, 112, 112, 224, 224) == (0, 224, 0, 224, 0.0)
    assert cutmix_box(0.0, 18, 14, 37, 29) == (0, 36, 0, 28, 1 - 36 * 28 / (37 * 29))   # odd sides: cut // 2 twice is one short


@pytest.mark.parametrize("H,W", [(224, 224), (37, 29)])
def test_box_at_the_four_borders_and_against_the_restatement(H, W):
    lam = 0.75
    ch, cw = int(H * 0.5) // 2, int(W * 0.5) // 2
    assert cutmix_box(lam, 0, W // 2, H, W)[:2] == (0, ch)                   # top
    assert cutmix_box(lam, H - 1, W // 2, H, W)[:2] == (H - 1 - ch, H)       # bottom
    assert cutmix_box(lam, H // 2, 0, H, W)[2:4] == (0, cw)                  # left
    assert cutmix_box(lam, H // 2, W - 1, H, W)[2:4] == (W - 1 - cw, W)      # right
    rng = np.random.default_rng(3)
    for _ in range(200):
        lam, cy, cx = float(rng.beta(1.0, 1.0)), int(rng.integers(0, H)), int(rng.integers(0, W))
        got = cutmix_box(lam, cy, cx, H, W)
        assert got == R.ref_box(lam, cy, cx, H, W)
        y0, y1, x0, x1, fixed = got
        assert 0 <= y0 <= y1 <= H and 0 <= x0 <= x1 <= W and fixed == 1 - (y1 - y0) * (x1 - x0) / (H * W)


def test_job_row_carries_float32_weights_subtracted_in_float64():
    lam = 0.9
    row = job_row(Decision(MIX_MIXUP, lam))
    assert len(row) == MIX_JOB_WORDS and row == R.job(R.MIXUP, lam)
    w = np.array(row[1:3], dtype=np.int32).view(np.float32)
    assert w[0] == np.float32(lam) and w[1] == np.float32(1.0 - lam)
    assert w[1] != np.float32(1.0) - np.float32(lam)                   # the float32 subtraction rounds differently
    assert job_row(Decision()) == [MIX_KEEP, int(np.array(np.float32(1)).view(np.int32)), 0, 0, 0, 0, 0, 0]


def _rows(table: torch.Tensor) -> list[tuple]:
    return [tuple(r) for r in table.tolist()]


@pytest.mark.parametrize("N", [8, 7])
def test_modes_share_decisions_as_promised(N):
    H, W = 37, 29
    torch.manual_seed(5)
    t = BatchMixer(0.8, 1.0, mode="batch", num_classes=2).sample(N, H, W)
    assert t.dtype == torch.int32 and tuple(t.shape) == (N, MIX_JOB_WORDS)
    rows = _rows(t)
    mixed = [r for k, r in enumerate(rows) if 2 * k + 1 != N]
    assert len(set(mixed)) == 1 and mixed[0][0] != MIX_KEEP              # prob = 1 and a Beta draw is never exactly 1
    pair_rows, elem_rows = [], []
    for seed in range(20):
        torch.manual_seed(seed)
        rows = _rows(BatchMixer(0.8, 1.0, mode="pair", num_classes=2).sample(N, H, W))
        assert all(rows[i] == rows[N - 1 - i] for i in range(N // 2))
        pair_rows.append(rows)
        torch.manual_seed(seed)
        elem_rows.append(_rows(BatchMixer(0.8, 1.0, mode="elem", num_classes=2).sample(N, H, W)))
    assert any(len(set(rows[:N // 2])) > 1 for rows in pair_rows)        # pairs decide independently
    assert any(rows[0] != rows[N - 1] for rows in elem_rows)             # samples decide independently
    modes = {r[0] for rows in elem_rows for r in rows}
    assert modes >= {MIX_MIXUP, MIX_CUTMIX}                               # switch_prob = 0.5 draws both kinds
    for rows in pair_rows + elem_rows:
        if N % 2:
            assert rows[N // 2] == tuple(R.job(R.KEEP))                   # the middle sample is its own partner
        for r in rows:
            if r[0] == MIX_CUTMIX:
                y0, y1, x0, x1 = r[3:7]
                assert 0 <= y0 < y1 <= H and 0 <= x0 < x1 <= W
                assert r[1:3] == tuple(R.job(R.CUTMIX, 1 - (y1 - y0) * (x1 - x0) / (H * W))[1:3])   # the corrected lam
            else:
                assert r[3:7] == (0, 0, 0, 0)


def test_prob_zero_keeps_everything_and_seed_reproduces():
    for mode in ("batch", "pair", "elem"):
        t = BatchMixer(0.8, 1.0, prob=0.0, mode=mode, num_classes=2).sample(9, 32, 32)
        assert _rows(t) == [tuple(R.job(R.KEEP))] * 9
        mixer = BatchMixer(0.8, 1.0, mode=mode, num_classes=2)
        torch.manual_seed(11)
        a = [mixer.sample(8, 64, 64) for _ in range(3)]
        torch.manual_seed(11)
        b = [mixer.sample(8, 64, 64) for _ in range(3)]
        assert all(torch.equal(p, q) for p, q in zip(a, b))
        assert not torch.equal(a[0], a[1])
    only_cut = BatchMixer(0.0, 1.0, mode="elem", num_classes=2).sample(8, 64, 64)
    assert set(only_cut[:, 0].tolist()) <= {MIX_CUTMIX, MIX_KEEP} and MIX_CUTMIX in only_cut[:, 0].tolist()
    only_mix = BatchMixer(0.8, 0.0, mode="elem", num_classes=2).sample(8, 64, 64)
    assert set(only_mix[:, 0].tolist()) == {MIX_MIXUP}


def test_mixer_argument_checks_and_cpu_refusal():
    for bad in (dict(mixup_alpha=0.0, cutmix_alpha=0.0), dict(mixup_alpha=-1.0), dict(prob=1.5), dict(switch_prob=-0.1),
                dict(mode="half"), dict(num_classes=0)):
        with pytest.raises(ValueError):
            BatchMixer(**bad)
    mixer = BatchMixer(0.8, 1.0, num_classes=2)
    with pytest.raises(RuntimeError, match="HIP device"):
        mixer(torch.zeros(2, 3, 8, 8), torch.zeros(2, dtype=torch.int64))


def test_host_table_check():
    from deepfakedetection_amd.kernels import check_mix_jobs

    ok = R.table([R.job(R.CUTMIX, 0.5, (0, 8, 0, 8)), R.job(R.KEEP), R.job(R.MIXUP, 0.3)])
    check_mix_jobs(ok, 3, 8, 8)
    for bad in ([R.job(R.CUTMIX, 0.5, (0, 9, 0, 8))] * 2, [R.job(R.CUTMIX, 0.5, (0, 8, -1, 8))] * 2,
                [R.job(R.CUTMIX, 0.5, (5, 4, 0, 8))] * 2, [R.job(3)] * 2,
                [R.job(R.KEEP), R.job(R.MIXUP, 0.5), R.job(R.KEEP)]):                # the middle of an odd batch mixes
        with pytest.raises(ValueError):
            check_mix_jobs(R.table(bad), len(bad), 8, 8)
    with pytest.raises(ValueError):
        check_mix_jobs(ok.long(), 3, 8, 8)


def test_reference_mix_on_a_hand_worked_batch():
    """The restatement itself, on numbers small enough to check by eye."""
    x = torch.arange(4 * 3 * 2 * 2, dtype=torch.float32).reshape(4, 3, 2, 2)
    labels = torch.tensor([0, 1, 1, 1])
    jobs = R.table([R.job(R.MIXUP, 0.25), R.job(R.CUTMIX, 0.75, (0, 1, 1, 2)), R.job(R.KEEP), R.job(R.MIXUP, 0.5)])
    out, y = R.ref_mix(x, labels, jobs, 3)
    assert torch.equal(out[0], x[0] * 0.25 + x[3] * 0.75) and torch.equal(out[3], x[3] * 0.5 + x[0] * 0.5)
    want1 = x[1].clone()
    want1[:, 0, 1] = x[2][:, 0, 1]
    assert torch.equal(out[1], want1) and torch.equal(out[2], x[2])
    assert y.tolist() == [[0.25, 0.75, 0.0], [0.0, 1.0, 0.0], [0.0, 1.0, 0.0], [0.5, 0.5, 0.0]]


def _overrides(training: dict) -> dict:
    from deepfakedetection_amd.orchestration.orchestrator import RunPaths, build_env_overrides

    run = Path("/nonexistent/run")
    cfg = {"data": {"root": "."}, "models": {"efficientnet_b0": {"training": training}}}
    return build_env_overrides(config=cfg, model_cfg={"name": "efficientnet_b0", "training": training},
                               run_paths=RunPaths(run, run / "c", run / "l", run / "p"), training=True)


def test_yaml_keys_map_to_environment():
    env = _overrides({"epochs": 1, "mixup_alpha": 0.8, "cutmix_alpha": 1.0, "mix_prob": 0.9, "mix_switch_prob": 0.25,
                      "mix_mode": "pair"})
    assert [env[v] for v in _MIX_VARS] == ["0.8", "1.0", "0.9", "0.25", "pair"]
    assert not set(_MIX_VARS) & set(_overrides({"epochs": 1}))


def test_trainer_settings_from_environment(monkeypatch):
    from deepfakedetection_amd.trainers.efficientnet import make_mixer, mix_settings

    for var in _MIX_VARS:
        monkeypatch.delenv(var, raising=False)
    assert mix_settings() is None and make_mixer(mix_settings(), 2, "cpu") is None      # absent: off
    monkeypatch.setenv("MIXUP_ALPHA", "0")
    monkeypatch.setenv("CUTMIX_ALPHA", "0.0")
    assert mix_settings() is None                                                       # both 0: off
    monkeypatch.setenv("CUTMIX_ALPHA", "1.0")
    s = mix_settings()
    assert (s.mixup_alpha, s.cutmix_alpha, s.prob, s.switch_prob, s.mode) == (0.0, 1.0, 1.0, 0.5, "batch")
    monkeypatch.setenv("MIXUP_ALPHA", "0.8")
    monkeypatch.setenv("MIX_PROB", "0.5")
    monkeypatch.setenv("MIX_SWITCH_PROB", "0.25")
    monkeypatch.setenv("MIX_MODE", "elem")
    s = mix_settings()
    assert (s.mixup_alpha, s.prob, s.switch_prob, s.mode) == (0.8, 0.5, 0.25, "elem")
    mixer = make_mixer(s, 5, "cuda:0")              # builds the host-side object only
    assert isinstance(mixer, BatchMixer) and (mixer.mode, mixer.num_classes, mixer.switch_prob) == ("elem", 5, 0.25)
    with pytest.raises(RuntimeError, match="HIP device"):
        make_mixer(s, 2, "cpu")


def test_loss_module_refuses_cpu_and_misshapen_probability_targets():
    from deepfakedetection_amd.optim import HipCrossEntropyLoss

    with pytest.raises(RuntimeError, match="HIP device"):
        HipCrossEntropyLoss(0.1)(torch.zeros(4, 2), torch.zeros(4, 2))


def test_abi_138_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.load()
    assert lib.dfd_version() >= 138
    buf = (ctypes.c_float * 64)()
    lab = (ctypes.c_int64 * 4)()
    jobs = (ctypes.c_int32 * 32)()
    p, l, j = ctypes.addressof(buf), ctypes.addressof(lab), ctypes.addressof(jobs)
    EINVAL = -1
    assert lib.dfd_mix_batch(None, l, j, p, 4, 2, 2, 2, 0, None) == EINVAL
    assert lib.dfd_mix_batch(p, None, j, p, 4, 2, 2, 2, 0, None) == EINVAL
    assert lib.dfd_mix_batch(p, l, None, p, 4, 2, 2, 2, 0, None) == EINVAL
    assert lib.dfd_mix_batch(p, l, j, None, 4, 2, 2, 2, 0, None) == EINVAL
    assert lib.dfd_mix_batch(p, l, j, p, 0, 2, 2, 2, 0, None) == EINVAL          # N < 1
    assert lib.dfd_mix_batch(p, l, j, p, 4, 2, 2, 0, 0, None) == EINVAL          # J < 1
    assert lib.dfd_mix_batch(p, l, j, p, 4, 0, 2, 2, 0, None) == EINVAL          # H < 1
    assert lib.dfd_mix_batch(p, l, j, p, 4, 2, 2, 2, 2, None) == EINVAL          # layout out of range
    assert lib.dfd_mix_batch(p, l, j, p, 4, 2, 2, 2, -1, None) == EINVAL
    for args in ((None, p, 2, 2, 0.1, 1.0, p, p, p, None), (p, None, 2, 2, 0.1, 1.0, p, p, p, None),
                 (p, p, 2, 2, 0.1, 1.0, None, p, p, None), (p, p, 2, 2, 0.1, 1.0, p, None, p, None),
                 (p, p, 0, 2, 0.1, 1.0, p, p, p, None), (p, p, 2, 0, 0.1, 1.0, p, p, p, None)):
        assert lib.dfd_ce_loss_soft(*args) == EINVAL
