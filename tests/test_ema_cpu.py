"""Weight EMA without a GPU: the decay schedule, the YAML -> environment mapping of the three training keys, the trainers'
reading of that environment, and the argument checks of dfd_ema_update (no device touched)."""

from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest

from deepfakedetection_amd import _lib
from deepfakedetection_amd.ema import decay_at, weight_at


def test_decay_schedule_warmup_cap_and_off():
    assert decay_at(1, 0.9999) == 2 / 11
    assert [decay_at(k, 0.9999) for k in (2, 3, 10)] == [3 / 12, 4 / 13, 11 / 20]
    # (1 + k) / (10 + k) reaches 0.9 at k = 80: the cap takes over from there
    assert decay_at(80, 0.9) == 0.9 and decay_at(79, 0.9) == 80 / 89 and decay_at(10**6, 0.9) == 0.9
    assert decay_at(10**9, 0.9999) == 0.9999
    assert all(decay_at(k, 0.99, warmup=False) == 0.99 for k in (1, 2, 1000))
    # w_k = float32(1 - d_k) computed in float64
    assert weight_at(1, 0.9999) == float(np.float32(1.0 - 2 / 11))
    assert weight_at(5, 0.999, warmup=False) == float(np.float32(1.0 - 0.999))


def _overrides(training: dict) -> dict:
    from deepfakedetection_amd.orchestration.orchestrator import RunPaths, build_env_overrides

    run = Path("/nonexistent/run")
    cfg = {"data": {"root": "."}, "models": {"efficientnet_b0": {"training": training}}}
    return build_env_overrides(config=cfg, model_cfg={"name": "efficientnet_b0", "training": training},
                               run_paths=RunPaths(run, run / "c", run / "l", run / "p"), training=True)


def test_yaml_keys_map_to_environment():
    env = _overrides({"epochs": 1, "ema_decay": 0.999, "ema_warmup": False, "ema_eval": True})
    assert (env["EMA_DECAY"], env["EMA_WARMUP"], env["EMA_EVAL"]) == ("0.999", "False", "True")
    env = _overrides({"epochs": 1})
    assert not {"EMA_DECAY", "EMA_WARMUP", "EMA_EVAL"} & set(env)


def test_trainer_settings_from_environment(monkeypatch):
    from deepfakedetection_amd.trainers.efficientnet import ema_settings

    for var in ("EMA_DECAY", "EMA_WARMUP", "EMA_EVAL"):
        monkeypatch.delenv(var, raising=False)
    assert ema_settings() is None                      # absent: off
    monkeypatch.setenv("EMA_DECAY", "0")
    assert ema_settings() is None                      # 0: off
    monkeypatch.setenv("EMA_DECAY", "0.999")
    s = ema_settings()
    assert (s.decay, s.warmup, s.select) == (0.999, True, True)
    monkeypatch.setenv("EMA_WARMUP", "False")
    monkeypatch.setenv("EMA_EVAL", "false")
    s = ema_settings()
    assert (s.warmup, s.select) == (False, False)


def test_model_ema_refuses_cpu_modules():
    import torch

    from deepfakedetection_amd.ema import ModelEma

    a, b = torch.nn.Linear(4, 2), torch.nn.Linear(4, 2)
    with pytest.raises(RuntimeError, match="HIP device"):
        ModelEma(a, b, decay=0.99)
    with pytest.raises(ValueError):
        ModelEma(a, b, decay=1.0)


def test_ema_update_rejects_bad_arguments_without_a_gpu():
    import ctypes

    lib = _lib.load()
    assert lib.dfd_version() >= 137
    table = (ctypes.c_int64 * 4)()
    w = ctypes.c_float(0.5)
    assert lib.dfd_ema_update(None, 1, ctypes.addressof(w), None) == -1          # DFD_EINVAL
    assert lib.dfd_ema_update(ctypes.addressof(table), 0, ctypes.addressof(w), None) == -1
    assert lib.dfd_ema_update(ctypes.addressof(table), 1, None, None) == -1
