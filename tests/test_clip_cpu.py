"""Gradient clipping without a GPU: the numpy restatement pinned to torch.nn.utils, the YAML -> environment mapping and the
engine's reading of it, HipAdamW's argument checks, the argument checks of the three ABI 140 entry points (no device touched),
and the stub trainer on the CPU with and without `training.clip_grad`."""

from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import pytest
import torch

from deepfakedetection_amd import _lib
from deepfakedetection_amd._lib import ADAMW_HP_LEN, ADAMW_TABLE_COLS, CLIP_CFG_LEN, CLIP_COEF, CLIP_NORM, CLIP_SKIP, CLIP_STATE_LEN
from tests import _clip_ref as ref
from tests.test_plumbing_cpu import TinyNet, _make_dataset, _train_stub

_F32 = np.float32


def _grads(seed: int = 0) -> list[np.ndarray]:
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(n).astype(_F32) for n in (1, 7, 129, 1000)]


def _bits(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=_F32)).view(np.uint32)


def _torch_norm_clip(grads, limit):
    params = [torch.nn.Parameter(torch.zeros(g.shape)) for g in grads]
    for p, g in zip(params, grads):
        p.grad = torch.from_numpy(g.copy())
    norm = torch.nn.utils.clip_grad_norm_(params, float(limit), foreach=False)
    return norm, [p.grad.numpy() for p in params]


@pytest.mark.parametrize("case", ["above", "below", "at"])
def test_reference_coefficient_and_gradients_equal_torch(case):
    """torch's coefficient is max_norm / (norm + 1e-6) clamped to 1, in f32: the restatement gives the same bits from torch's
    own norm, and the same clipped gradients."""
    grads = _grads()
    norm0, _ = _torch_norm_clip(grads, 1e30)
    limit = {"above": 0.25 * float(norm0), "below": 4.0 * float(norm0), "at": float(norm0)}[case]
    norm, clipped = _torch_norm_clip(grads, limit)
    assert np.array_equal(_bits(norm.numpy()), _bits(norm0.numpy()))
    c_torch = torch.clamp(torch.tensor(limit, dtype=torch.float32) / (norm + 1e-6), max=1.0).numpy()
    c = ref.coef(norm.numpy(), limit)
    assert c.dtype == _F32 and np.array_equal(_bits(c), _bits(c_torch)), (c, c_torch)
    # (exactly at the limit the 1e-6 vanishes in the f32 sum when the norm is this large: the coefficient is then 1, as torch's is)
    assert c < 1.0 if case == "above" else c == 1.0 if case == "below" else c <= 1.0
    for got, want in zip(ref.scale(grads, c), clipped):
        assert np.array_equal(_bits(got), _bits(want))
    # the exactly rounded norm and torch's f32 one are the same number up to torch's f32 summation error
    assert abs(float(ref.total_norm(grads)) - float(norm)) <= 1e-5 * float(norm)


def test_reference_value_clamp_equals_torch():
    grads = _grads(1)
    params = [torch.nn.Parameter(torch.zeros(g.shape)) for g in grads]
    for p, g in zip(params, grads):
        p.grad = torch.from_numpy(g.copy())
    torch.nn.utils.clip_grad_value_(params, 0.3, foreach=False)
    for got, p in zip(ref.clamp(grads, 0.3), params):
        assert np.array_equal(_bits(got), _bits(p.grad.numpy()))
    assert any(np.abs(g).max() > 0.3 for g in grads)


def test_reference_helpers():
    assert ref.coef(_F32("nan"), 1.0) == 1.0 and ref.coef(_F32("inf"), 1.0) == 0.0
    assert ref.within_one_ulp(_F32(1.0), np.nextafter(_F32(1.0), _F32(2.0)))
    assert not ref.within_one_ulp(_F32(1.0), _F32(1.0) + 4 * np.spacing(_F32(1.0)))
    assert ref.total_norm([np.array([3.0], _F32), np.array([4.0], _F32)], 0.5) == 2.5


def _overrides(training: dict) -> dict:
    from deepfakedetection_amd.orchestration.orchestrator import RunPaths, build_env_overrides

    run = Path("/nonexistent/run")
    cfg = {"data": {"root": "."}, "models": {"efficientnet_b0": {"training": training}}}
    return build_env_overrides(config=cfg, model_cfg={"name": "efficientnet_b0", "training": training},
                               run_paths=RunPaths(run, run / "c", run / "l", run / "p"), training=True)


def test_yaml_keys_map_to_environment():
    env = _overrides({"epochs": 1, "clip_grad": 0.5, "clip_mode": "value"})
    assert (env["CLIP_GRAD"], env["CLIP_MODE"]) == ("0.5", "value")
    assert not {"CLIP_GRAD", "CLIP_MODE"} & set(_overrides({"epochs": 1}))


def test_engine_settings_from_environment(monkeypatch):
    from deepfakedetection_amd.trainers._engine import clip_settings

    for var in ("CLIP_GRAD", "CLIP_MODE"):
        monkeypatch.delenv(var, raising=False)
    assert clip_settings() is None                     # absent: off
    monkeypatch.setenv("CLIP_GRAD", "0")
    assert clip_settings() is None                     # 0: off
    monkeypatch.setenv("CLIP_GRAD", "0.5")
    s = clip_settings()
    assert (s.limit, s.mode) == (0.5, "norm")
    monkeypatch.setenv("CLIP_MODE", "Value")
    assert clip_settings().mode == "value"
    monkeypatch.setenv("CLIP_MODE", "agc")
    with pytest.raises(ValueError, match="clip_mode"):
        clip_settings()
    monkeypatch.setenv("CLIP_MODE", "norm")
    for bad in ("-1", "nan", "inf"):
        monkeypatch.setenv("CLIP_GRAD", bad)
        with pytest.raises(ValueError, match="clip_grad"):
            clip_settings()


def test_hip_adamw_checks_its_clip_arguments():
    from deepfakedetection_amd.optim import HipAdamW

    params = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(5))]
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            HipAdamW(params, max_grad_norm=bad)
    with pytest.raises(ValueError, match="clip_mode"):
        HipAdamW(params, max_grad_norm=1.0, clip_mode="agc")
    groups = [{"params": params[:1], "grad_scale": 1.0}, {"params": params[1:], "grad_scale": 0.5}]
    with pytest.raises(ValueError, match="grad_scale"):
        HipAdamW(groups, max_grad_norm=1.0)
    opt = HipAdamW(groups)                              # different scales are fine as long as nothing is clipped
    assert opt.clip_stats() is None and opt.clip_state is None
    with pytest.raises(ValueError, match="grad_scale"):
        opt.set_clip(1.0)
    opt = HipAdamW(params)
    with pytest.raises(ValueError, match="max_grad_norm"):
        opt.set_clip(-2.0)
    with pytest.raises(ValueError, match="clip_mode"):
        opt.set_clip(1.0, "both")


def test_abi_140_entry_points_check_their_arguments_without_a_gpu():
    import ctypes

    lib = _lib.load()
    assert lib.dfd_version() >= 140
    table = (ctypes.c_int64 * ADAMW_TABLE_COLS)()
    partials = (ctypes.c_double * 1)()
    hp = (ctypes.c_float * ADAMW_HP_LEN)()
    cfg = (ctypes.c_float * CLIP_CFG_LEN)()
    state = (ctypes.c_float * CLIP_STATE_LEN)()
    t, pa, h, c, s = (ctypes.addressof(b) for b in (table, partials, hp, cfg, state))
    einval = -1
    assert lib.dfd_grad_sumsq(None, 1, pa, None) == einval
    assert lib.dfd_grad_sumsq(t, 1, None, None) == einval
    assert lib.dfd_grad_sumsq(t, 0, pa, None) == einval
    for args in ((None, 1, h, c, s), (pa, 0, h, c, s), (pa, 1, None, c, s), (pa, 1, h, None, s), (pa, 1, h, c, None)):
        assert lib.dfd_grad_clip_finish(*args, None) == einval, args
    for args in ((None, 1, h, c, s), (t, 0, h, c, s), (t, 1, None, c, s), (t, 1, h, None, s), (t, 1, h, c, None)):
        assert lib.dfd_adamw_step_clip(*args, None) == einval, args
    assert CLIP_STATE_LEN == 8 and (CLIP_NORM, CLIP_COEF, CLIP_SKIP) == (0, 1, 2)


def _stub_run(root: Path, monkeypatch, tag: str, **training):
    """One seeded CPU training of the EfficientNet trainer's stub in its own workspace: (log, final weights, throughput rows)."""
    from deepfakedetection_amd.orchestration import model_registry as reg

    ws = root / tag
    ws.mkdir()
    monkeypatch.chdir(ws)
    _make_dataset(ws / "data")
    reg.register_model_spec(reg.ModelSpec("tinynet_stub", "deepfakedetection_amd.trainers.efficientnet", "tinynet_stub", 32,
                                          lambda _name, nc: TinyNet(nc)))
    log = _train_stub(ws, "efficientnet", epochs=1, **training)
    run = sorted((ws / "runs" / "stub_efficientnet").iterdir())[0]
    weights = torch.load(run / "checkpoints" / "latest.ckpt")["model"]
    rows = [json.loads(line) for line in (run / "logs" / "throughput.jsonl").read_text().splitlines()]
    return log, weights, rows


_FIELDS = ("grad_norm_mean", "grad_norm_max", "clipped_steps", "skipped_steps")


def test_stub_trainer_clips_on_cpu(tmp_path, monkeypatch):
    import re

    log, clipped, rows = _stub_run(tmp_path, monkeypatch, "clip", clip_grad=1e-3)
    tail = r" \| grad_norm=(\S+) \(clipped (\d+)/(\d+)\)"
    lines = re.findall(r"(warmup) \| val_acc=\S+ \| val_loss=\S+ \(\d+/18\)" + tail, log)
    lines += re.findall(r"(epoch 1) \| train_loss=\S+ \| val_loss=\S+ \| val_acc=\S+ \(\d+/18\) \| lr=\S+" + tail, log)
    assert [m[0] for m in lines] == ["warmup", "epoch 1"], log
    for _, mean, k, n in lines:
        assert float(mean) > 1e-3 and k == n and int(n) >= 1           # every step's norm is above 1e-3: all clipped
    assert [r["phase"] for r in rows] == ["warmup", "fine-tune"]
    for r in rows:
        assert all(f in r for f in _FIELDS), r
        assert r["skipped_steps"] == 0 and r["clipped_steps"] >= 1 and r["grad_norm_max"] >= r["grad_norm_mean"] > 1e-3
    assert rows[0]["clipped_steps"] == 3 and rows[1]["clipped_steps"] == 1     # 18 images: 3 steps of 6; one cycle of 32 x 4

    log_off, plain, rows_off = _stub_run(tmp_path, monkeypatch, "absent")
    log_zero, zero, rows_zero = _stub_run(tmp_path, monkeypatch, "zero", clip_grad=0)
    for text, rws in ((log_off, rows_off), (log_zero, rows_zero)):
        assert "grad_norm" not in text and "clipped" not in text
        assert not any(f in r for r in rws for f in _FIELDS)
    assert set(plain) == set(zero) == set(clipped)
    assert all(torch.equal(plain[k], zero[k]) for k in plain)
    assert any(not torch.equal(plain[k], clipped[k]) for k in plain if plain[k].is_floating_point())


def test_stub_trainer_value_mode_and_bad_settings(tmp_path, monkeypatch):
    log, _, rows = _stub_run(tmp_path, monkeypatch, "value", clip_grad=1e-3, clip_mode="value")
    assert "grad_norm=" in log and all(r["clipped_steps"] == 0 and r["grad_norm_mean"] > 0 for r in rows)
    with pytest.raises(ValueError, match="clip_mode"):
        _stub_run(tmp_path, monkeypatch, "badmode", clip_grad=1.0, clip_mode="agc")
    with pytest.raises(ValueError, match="clip_grad"):
        _stub_run(tmp_path, monkeypatch, "negative", clip_grad=-1.0)
