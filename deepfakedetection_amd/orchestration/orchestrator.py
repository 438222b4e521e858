"""Orchestration layer: YAML -> per-model run directory -> training or inference job.

Counterpart of the reference's orchestration/orchestrator.py with the same public
surface and behaviour on the hot-path rows of SURVEY.md section 8:

  load_config              :112-125   YAML -> validated plain dict
  ensure_run_dirs          :138-145   <output_dir>/<YYYYmmdd-HHMMSS>/{checkpoints,logs,plots}
  snapshot_config          :148-159   config_snapshot.yaml
  resolve_transform_mapping:162-180
  build_env_overrides      :183-283   the YAML -> environment-variable contract
  run_training_job         :294-307   in-process `main()` of the spec's trainer under patched env
  build_eval_transforms    :316-347
  load_model               :350-377   builder -> device -> eval -> load_state_dict(strict=False)
  run_inference_job        :418-658   threshold sweep (binary), test pass, metrics.jsonl, plots
  orchestrate / run_cli    :661-713

What differs: models come from this package's registry (HIP kernels underneath), the data
pipeline is deepfakedetection_amd.data (no torchvision), soft-max/arg-max of the inference
loops run in the dfd_softmax_argmax kernel, the 501-threshold balanced-accuracy sweep is
vectorised, and three extra variables are exported for the trainers (MODEL_NAME,
FT_BATCH_SIZE, PRETRAINED) on top of the reference's set.
"""

from __future__ import annotations

import argparse
import contextlib
import importlib
import io
import json
import math
import os
import re
import sys
from collections.abc import Iterator
from dataclasses import asdict, dataclass, replace
from datetime import datetime
from pathlib import Path
from time import perf_counter
from typing import Any

import numpy as np
import torch
import yaml
from rich.console import Console
from rich.progress import BarColumn, MofNCompleteColumn, Progress, TextColumn, TimeElapsedColumn, TimeRemainingColumn
from torch import nn
from torch.utils.data import DataLoader

from .. import data as D
from .. import metrics as M
from .._lib import BLUR_MAX_PIXELS, BOOT_MAX_MEMBERS, BOOT_MAX_REPLICATES, CALIB_MAX_BINS, FUSE_MAX_MODELS
from .config_schema import OrchestratorConfig
from .model_registry import get_model_spec
from .train_env import apply_seed, as_bool, require_num_classes

console = Console()

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
RELEASE_URL = "https://github.com/thourihan/DeepfakeDetection/releases/download/v0.3.0/"
RELEASE_FILES = {
    "efficientnet_b3": "efficientnet_b3_v0.3.0.pth",
    "efficientformerv2_s1": "efficientformerv2_s1_v0.3.0.pth",
    "faster_vit_2_224": "faster_vit_2_224_v0.3.0.pth",
}


@dataclass(frozen=True)
class RunPaths:
    run_dir: Path
    checkpoints: Path
    logs: Path
    plots: Path


@contextlib.contextmanager
def patched_environ(overrides: dict[str, str]) -> Iterator[None]:
    """Set environment variables for the duration of a trainer call, then restore."""
    saved = {key: os.environ.get(key) for key in overrides}
    os.environ.update(overrides)
    try:
        yield
    finally:
        for key, old in saved.items():
            if old is None:
                os.environ.pop(key, None)
            else:
                os.environ[key] = old


@contextlib.contextmanager
def tee_output(log_path: Path) -> Iterator[None]:
    """Mirror stdout and stderr into `log_path` (truncated) while the block runs."""
    log_path.parent.mkdir(parents=True, exist_ok=True)
    out, err = sys.stdout, sys.stderr
    with log_path.open("w", encoding="utf-8") as log:

        class _Both(io.TextIOBase):
            def write(self, text: str) -> int:
                out.write(text)
                log.write(text)
                return len(text)

            def flush(self) -> None:
                out.flush()
                log.flush()

            def isatty(self) -> bool:
                probe = getattr(out, "isatty", None)
                return bool(probe()) if callable(probe) else False

            @property
            def encoding(self) -> str:  # type: ignore[override]
                return getattr(out, "encoding", "utf-8")

        sys.stdout = sys.stderr = _Both()  # type: ignore[assignment]
        try:
            yield
        finally:
            sys.stdout, sys.stderr = out, err
            log.flush()


def load_config(path: Path) -> dict[str, Any]:
    with Path(path).open("r", encoding="utf-8") as handle:
        raw = yaml.safe_load(handle)
    return OrchestratorConfig(**raw).model_dump()


def ensure_run_dirs(base: Path, timestamp: str) -> RunPaths:
    run = Path(base) / timestamp
    paths = RunPaths(run, run / "checkpoints", run / "logs", run / "plots")
    for folder in (paths.run_dir, paths.checkpoints, paths.logs, paths.plots):
        folder.mkdir(parents=True, exist_ok=True)
    return paths


def snapshot_config(run_paths: RunPaths, *, config: dict[str, Any], model_cfg: dict[str, Any]) -> None:
    snap = {
        "timestamp": datetime.now().isoformat(),
        "global": {key: val for key, val in config.items() if key not in ("models", "selection")},
        "model": model_cfg,
    }
    with (run_paths.run_dir / "config_snapshot.yaml").open("w", encoding="utf-8") as handle:
        yaml.safe_dump(snap, handle)


def resolve_transform_mapping(model_cfg: dict[str, Any], *, phase: str) -> dict[str, Any] | None:
    """Toggles for `phase` ('train' | 'eval'): models.<m>.transforms.<phase>, else a flat
    models.<m>.transforms mapping of scalars, else <training|inference>.transforms."""
    block = model_cfg.get("transforms")
    if isinstance(block, dict):
        scoped = block.get(phase)
        if isinstance(scoped, dict):
            return scoped
        if all(isinstance(v, (bool, int, float, str)) for v in block.values()):
            return block
    section = model_cfg.get("training" if phase == "train" else "inference") or {}   # None when the YAML lacks the block
    nested = section.get("transforms")
    return nested if isinstance(nested, dict) else None


_DATA_ENV = (("train_split", "TRAIN_SPLIT"), ("val_split", "VAL_SPLIT"), ("test_split", "TEST_SPLIT"),
             ("img_size", "IMG_SIZE"), ("num_classes", "NUM_CLASSES"))
_TRAIN_ENV = (("batch_size", "BATCH_SIZE"), ("epochs", "EPOCHS"), ("num_workers", "NUM_WORKERS"), ("lr", "LR"),
              ("weight_decay", "WEIGHT_DECAY"), ("accum_steps", "ACCUM_STEPS"), ("warmup_epochs", "WARMUP_EPOCHS"),
              ("early_stop_patience", "EARLY_STOP_PATIENCE"))
_EXTRA_TRAIN_ENV = (("ft_batch_size", "FT_BATCH_SIZE"), ("pretrained", "PRETRAINED"), ("gpu_input_tail", "GPU_INPUT_TAIL"),
                    ("graph_step", "GRAPH_STEP"), ("fp8_weights", "FP8_WEIGHTS"), ("gpu_resize", "GPU_RESIZE"),
                    ("ema_decay", "EMA_DECAY"), ("ema_warmup", "EMA_WARMUP"), ("ema_eval", "EMA_EVAL"),
                    ("mixup_alpha", "MIXUP_ALPHA"), ("cutmix_alpha", "CUTMIX_ALPHA"), ("mix_prob", "MIX_PROB"),
                    ("mix_switch_prob", "MIX_SWITCH_PROB"), ("mix_mode", "MIX_MODE"),
                    ("rand_augment_ops", "RAND_AUGMENT_OPS"), ("rand_augment_magnitude", "RAND_AUGMENT_MAGNITUDE"),
                    ("trivial_augment", "TRIVIAL_AUGMENT"), ("clip_grad", "CLIP_GRAD"), ("clip_mode", "CLIP_MODE"),
                    ("jpeg_p", "JPEG_P"), ("jpeg_quality_min", "JPEG_QUALITY_MIN"), ("jpeg_quality_max", "JPEG_QUALITY_MAX"),
                    ("blur_p", "BLUR_P"), ("blur_sigma_min", "BLUR_SIGMA_MIN"), ("blur_sigma_max", "BLUR_SIGMA_MAX"),
                    ("val_auc", "VAL_AUC"), ("select_metric", "SELECT_METRIC"),
                    ("class_weights", "CLASS_WEIGHTS"), ("focal_gamma", "FOCAL_GAMMA"), ("balanced_sampling", "BALANCED_SAMPLING"))


def _first_set(*values: Any) -> Any:
    for value in values:
        if value is not None:
            return value
    return None


def build_env_overrides(*, config: dict[str, Any], model_cfg: dict[str, Any], run_paths: RunPaths,
                        training: bool) -> dict[str, str]:
    data_cfg = config.get("data") or {}
    train_cfg = model_cfg.get("training") or {}
    infer_cfg = model_cfg.get("inference") or {}
    env: dict[str, str] = {"OUTPUT_DIR": str(run_paths.run_dir), "MODEL_NAME": str(model_cfg["name"])}
    if config.get("seed") is not None:
        env["SEED"] = str(config["seed"])
    if config.get("device"):
        env["DEVICE"] = str(config["device"])
    if data_cfg.get("root"):
        env["DATA_ROOT"] = str(Path(data_cfg["root"]).expanduser().resolve())
    for key, var in _DATA_ENV:
        if data_cfg.get(key) is not None:
            env[var] = str(data_cfg[key])
    classes = infer_cfg.get("num_classes", model_cfg.get("num_classes", data_cfg.get("num_classes")))
    if classes is not None:
        env["NUM_CLASSES"] = str(classes)

    if training:
        for key, var in _TRAIN_ENV + _EXTRA_TRAIN_ENV:
            if train_cfg.get(key) is not None:
                env[var] = str(train_cfg[key])
        if train_cfg.get("img_size") is not None:
            env["IMG_SIZE"] = str(train_cfg["img_size"])
        env["RESUME_AUTO"] = "1" if str(train_cfg.get("resume", "")).lower() in ("1", "true", "auto") else "0"
    else:
        spec = get_model_spec(model_cfg["name"])
        if infer_cfg.get("split"):
            env["TEST_SPLIT"] = str(infer_cfg["split"])
        env["BATCH_SIZE"] = str(_first_set(infer_cfg.get("batch_size"), train_cfg.get("batch_size"), 64))
        env["NUM_WORKERS"] = str(_first_set(infer_cfg.get("num_workers"), train_cfg.get("num_workers"),
                                            data_cfg.get("num_workers", 0)))
        env["IMG_SIZE"] = str(_first_set(infer_cfg.get("img_size"), train_cfg.get("img_size"),
                                         data_cfg.get("img_size", spec.default_image_size)))

    toggles = resolve_transform_mapping(model_cfg, phase="train" if training else "eval")
    if toggles:
        env["TRANSFORMS"] = json.dumps(toggles)
    return env


def import_trainer(module_name: str) -> Any:
    module = importlib.import_module(module_name)
    if not hasattr(module, "main"):
        raise AttributeError(f"Trainer module '{module_name}' must expose a main() function.")
    return module.main


def run_training_job(config: dict[str, Any], model_cfg: dict[str, Any], run_paths: RunPaths) -> None:
    spec = get_model_spec(model_cfg["name"])
    env = build_env_overrides(config=config, model_cfg=model_cfg, run_paths=run_paths, training=True)
    log_path = run_paths.logs / "train.log"
    log_path.unlink(missing_ok=True)
    env["LOG_PATH"] = str(log_path)
    console.print(f"[bold]→ training {model_cfg['name']}[/]")
    with patched_environ(env):
        import_trainer(spec.train_module)()


def _to_rgb(image):
    return image if image.mode == "RGB" else image.convert("RGB")


def build_eval_transforms(image_size: int, *, toggles: dict[str, Any] | None = None) -> D.Compose:
    on = {"ensure_rgb": True, "val_resize": True, "val_center_crop": True, "val_to_tensor": True, "val_normalize": True}
    on.update({key: as_bool(val) for key, val in (toggles or {}).items()})
    ops: list[Any] = []
    if on.get("ensure_rgb", True):
        ops.append(D.Lambda(_to_rgb))
    if on.get("val_resize", True):
        ops.append(D.Resize(image_size))
    if on.get("val_center_crop", True):
        ops.append(D.CenterCrop(image_size))
    if on.get("val_to_tensor", True):
        ops.append(D.ToTensor())
    if on.get("val_normalize", True):
        ops.append(D.Normalize(IMAGENET_MEAN, IMAGENET_STD))
    return D.Compose(ops)


def load_model(model_name: str, num_classes: int, weights_path: Path | None, device: torch.device,
               img_size: int | None = None) -> nn.Module:
    """Reference orchestrator.py:350-377.  One addition: a builder that takes `img_size` (EfficientFormerV2: its
    attention-bias tables depend on the resolution; the reference's registry builder omits it, model_registry.py:40,
    and so only works at the default 224) receives the job's image size."""
    import inspect

    builder = get_model_spec(model_name).builder
    if img_size is not None and "img_size" in inspect.signature(builder).parameters:
        model = builder(model_name, num_classes, img_size)
    else:
        model = builder(model_name, num_classes)
    model.to(device)
    model.eval()
    if weights_path is not None:
        if not weights_path.exists():
            console.print(f"[bold red]Weights not found:[/] {weights_path}")
            raise SystemExit(1)
        console.print(f"[bold green]Loading weights[/]: {weights_path} ({weights_path.stat().st_size / 2**20:.2f} MiB)")
        state = torch.load(weights_path, map_location=device)
        if isinstance(state, dict) and "state_dict" in state:
            state = state["state_dict"]
        elif isinstance(state, dict) and "model" in state:
            state = state["model"]
        model.load_state_dict(state, strict=False)
    return model


_GPU_EVAL_TAIL = D.GpuInputTail(IMAGENET_MEAN, IMAGENET_STD)


def build_inference_loader(*, dataset, batch_size: int, num_workers: int) -> DataLoader:
    extra = {"prefetch_factor": 2} if num_workers > 0 else {}
    tf = getattr(dataset, "transform", None)
    if tf is not None and any(isinstance(op, D.PlanGeometry) for op in getattr(tf, "ops", ())):
        extra["collate_fn"] = D.collate_raw         # device-side resize: decoded images + plans (data.PlanGeometry)
    return DataLoader(dataset, batch_size=batch_size, shuffle=False, num_workers=num_workers, pin_memory=True,
                      persistent_workers=num_workers > 0, **extra)


def class_probabilities(model: nn.Module, images: torch.Tensor, device: torch.device, amp: bool = False, tail=None,
                        return_logits: bool = False):
    """logits -> (softmax probabilities, arg-max) for one batch (orchestrator.py:589-592).  amp: run the forward in a
    bf16 autocast region (opt-in `inference.amp: bf16`; the reference's inference is f32, which stays the default).
    tail: the D.GpuInputTail a data.collate_raw batch goes through (default: _GPU_EVAL_TAIL; the robustness pass hands in
    one that perturbs the cropped bytes first).  return_logits: hand back (probabilities, arg-max, f32 logits) instead
    (`inference.calibration` keeps them)."""
    with torch.inference_mode(), torch.autocast(device_type=device.type, dtype=torch.bfloat16, enabled=amp and device.type == "cuda"):
        if isinstance(images, (tuple, list)):          # data.collate_raw batch: resize / crop / normalise on the device
            images = (tail if tail is not None else _GPU_EVAL_TAIL)(images, device)
        logits = model(images.to(device, non_blocking=True))
        if logits.is_cuda:
            from .. import kernels  # HIP softmax/argmax epilogue

            logits = logits.float().contiguous()
            probs, preds = kernels.softmax_argmax(logits, True)
        else:
            probs = torch.softmax(logits, dim=1)
            preds = torch.argmax(probs, dim=1)
    if return_logits:
        return probs, preds, logits.float()
    return probs, preds


def calibration_settings(infer_cfg: dict[str, Any]) -> tuple[int, str | float] | None:
    """Extra key `inference.calibration: {bins: 15, temperature: fit}`: (bins, "fit" or the temperature to apply) or None without
    the key.  temperature: `fit` (the default: fitted on the validation split), `off` (1.0) or a number > 0.  ValueError for
    anything else or for bins outside 1..64."""
    raw = infer_cfg.get("calibration")
    if raw is None or raw is False:
        return None
    if raw is True:
        raw = {}
    if not isinstance(raw, dict):
        raise ValueError(f"inference.calibration must be a mapping like {{bins: 15, temperature: fit}}, got {raw!r}")
    bins = int(raw.get("bins", 15))
    if not 1 <= bins <= CALIB_MAX_BINS:
        raise ValueError(f"inference.calibration.bins must be 1..{CALIB_MAX_BINS}, got {bins}")
    temperature = raw.get("temperature", "fit")
    if temperature is False or temperature is None or str(temperature).strip().lower() in ("off", "none", "false", "no"):
        return bins, 1.0                        # YAML reads a bare `off` as false
    if temperature is True or str(temperature).strip().lower() in ("fit", "true", "on", "yes"):
        return bins, "fit"
    value = float(temperature)
    if not (math.isfinite(value) and value > 0.0):
        raise ValueError(f"inference.calibration.temperature must be fit, off or a number > 0, got {temperature!r}")
    return bins, value


def bootstrap_settings(raw: Any, where: str = "inference.bootstrap") -> tuple[int, float, int] | None:
    """Extra key `inference.bootstrap: {replicates: 2000, level: 0.95, seed: 0}` (and `ensemble.bootstrap`): (replicates, level,
    seed) of the percentile intervals metrics.bootstrap adds to every judged pass, or None without the key.  ValueError for another
    key, replicates outside 1..65536, a level outside (0, 1) or a seed that is no unsigned 64-bit integer."""
    if raw is None or raw is False:
        return None
    if raw is True:
        raw = {}
    if not isinstance(raw, dict):
        raise ValueError(f"{where} must be a mapping like {{replicates: 2000, level: 0.95, seed: 0}}, got {raw!r}")
    unknown = sorted(set(map(str, raw)) - {"replicates", "level", "seed"})
    if unknown:
        raise ValueError(f"{where} takes replicates, level and seed; not {', '.join(unknown)}")
    try:
        replicates, level, seed = int(raw.get("replicates", 2000)), float(raw.get("level", 0.95)), int(raw.get("seed", 0))
    except (TypeError, ValueError):
        raise ValueError(f"{where} takes numbers, got {raw!r}") from None
    if not 1 <= replicates <= BOOT_MAX_REPLICATES:
        raise ValueError(f"{where}.replicates must be 1..{BOOT_MAX_REPLICATES}, got {raw.get('replicates')!r}")
    if not 0.0 < level < 1.0:
        raise ValueError(f"{where}.level must lie inside (0, 1), got {raw.get('level')!r}")
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"{where}.seed must be an unsigned 64-bit integer, got {raw.get('seed')!r}")
    return replicates, level, seed


GROUP_KEYS, GROUP_POOLS = ("parent", "regex"), ("mean", "vote", "max")


def group_settings(raw: Any, where: str = "inference.group_by") -> tuple[str, str | None, str] | None:
    """Extra key `inference.group_by: {key: parent, pool: mean}` or `{key: regex, pattern: '^(.+)_\\d+$', pool: vote}`: (key,
    pattern, pool) by which the frames of a split are grouped into videos (metrics.group_ids) and a video's frames pooled into one
    score (metrics.group_pool), or None without the key.  pool: mean (the default), vote or max.  ValueError for another key, an
    unknown value, `regex` without a pattern that compiles and has a capture group, or a pattern without `regex`."""
    if raw is None or raw is False:
        return None
    if not isinstance(raw, dict):
        raise ValueError(f"{where} must be a mapping like {{key: parent, pool: mean}}, got {raw!r}")
    unknown = sorted(set(map(str, raw)) - {"key", "pattern", "pool"})
    if unknown:
        raise ValueError(f"{where} takes key, pattern and pool; not {', '.join(unknown)}")
    key, pool, pattern = str(raw.get("key", "parent")).strip().lower(), str(raw.get("pool", "mean")).strip().lower(), raw.get("pattern")
    if key not in GROUP_KEYS:
        raise ValueError(f"{where}.key must be one of {', '.join(GROUP_KEYS)}, got {raw.get('key')!r}")
    if pool not in GROUP_POOLS:
        raise ValueError(f"{where}.pool must be one of {', '.join(GROUP_POOLS)}, got {raw.get('pool')!r}")
    if key == "regex":
        try:
            groups = re.compile(str(pattern)).groups if isinstance(pattern, str) and pattern else 0
        except re.error as exc:
            raise ValueError(f"{where}.pattern does not compile: {exc}") from None
        if groups < 1:
            raise ValueError(f"{where}.pattern must be a regular expression with a capture group, got {pattern!r}")
    elif pattern is not None:
        raise ValueError(f"{where}.pattern needs key: regex")
    return key, (str(pattern) if key == "regex" else None), pool


@dataclass(frozen=True)
class EnsembleSettings:
    """The top-level `ensemble:` key, every default applied (ensemble_settings)."""
    members: tuple[str, ...]                        # keys of `models`, in the order they are fused
    mode: str                                       # "logit" (log-linear pool) | "prob" (linear pool)
    weights: str | tuple[float, ...]                # "equal" | "fit" | one weight per member
    l2: float
    output_dir: Path
    bootstrap: tuple[int, float, int] | None = None     # bootstrap_settings of `ensemble.bootstrap`


def ensemble_settings(config: dict[str, Any], out: Console) -> EnsembleSettings | None:
    """Extra top-level key `ensemble: {members: [...], mode: logit, weights: fit, l2: 0.0, output_dir: runs/ensemble}`, or None
    without the key.  members: default the selection; each must be a key of `models` that the selection runs.  mode: `logit`
    (softmax of the weighted sum of logits) or `prob` (weighted sum of probabilities).  weights: `equal`, `fit` (fitted on the
    validation split; logit mode only) or a list with one finite number per member (prob mode: none negative, summing to 1).
    ValueError for anything else.  A single member warns on `out`: it is fused, but there is nothing to combine."""
    raw = config.get("ensemble")
    if raw is None or raw is False:
        return None
    if raw is True:
        raw = {}
    if not isinstance(raw, dict):
        raise ValueError(f"ensemble must be a mapping like {{members: [a, b], mode: logit, weights: fit}}, got {raw!r}")
    models_cfg = config.get("models") or {}
    selection = [str(n) for n in (config.get("selection") if config.get("selection") is not None else list(models_cfg))]
    members = raw.get("members")
    members = tuple(selection if members is None else [str(m) for m in members]) if members is None or isinstance(members, (list, tuple)) else None
    if not members or not 1 <= len(members) <= FUSE_MAX_MODELS or len(set(members)) != len(members):
        raise ValueError(f"ensemble.members must list 1..{FUSE_MAX_MODELS} distinct models, got {raw.get('members')!r}")
    missing = [m for m in members if m not in models_cfg or m not in selection]
    if missing:
        raise ValueError(f"ensemble.members must be models that the selection runs; not among them: {', '.join(missing)}")
    mode = str(raw.get("mode", "logit")).strip().lower()
    if mode not in ("logit", "prob"):
        raise ValueError(f"ensemble.mode must be logit or prob, got {raw.get('mode')!r}")
    weights = raw.get("weights", "fit" if mode == "logit" else "equal")
    if isinstance(weights, (list, tuple)):
        try:
            weights = tuple(float(w) for w in weights)
        except (TypeError, ValueError):
            weights = ()
        if len(weights) != len(members) or not all(math.isfinite(w) for w in weights):
            raise ValueError(f"ensemble.weights must hold one finite number per member ({len(members)}), got {raw.get('weights')!r}")
        if mode == "prob" and (min(weights) < 0.0 or abs(math.fsum(weights) - 1.0) > 1e-12):
            raise ValueError(f"ensemble.weights in prob mode must be >= 0 and sum to 1, got {list(weights)}")
    else:
        weights = str(weights).strip().lower()
        if weights not in ("equal", "fit"):
            raise ValueError(f"ensemble.weights must be equal, fit or a list with one number per member, got {raw.get('weights')!r}")
        if weights == "fit" and mode == "prob":
            raise ValueError("ensemble.weights: fit needs ensemble.mode: logit (the fit is that of the log-linear pool)")
    l2 = float(raw.get("l2", 0.0))
    if not (math.isfinite(l2) and l2 >= 0.0):
        raise ValueError(f"ensemble.l2 must be a number >= 0, got {raw.get('l2')!r}")
    if len(members) == 1:
        out.print("[bold yellow]ensemble[/]: one member only; its scores are fused with nothing")
    return EnsembleSettings(members, mode, weights, l2, Path(str(raw.get("output_dir") or "runs/ensemble")),
                            bootstrap_settings(raw.get("bootstrap"), "ensemble.bootstrap"))


def robustness_levels(infer_cfg: dict[str, Any]) -> list[tuple[str, float | int]]:
    """Extra key `inference.robustness: {blur_sigma: [1, 2, 3], jpeg_quality: [90, 70, 50]}`: the perturbation levels the test
    split is evaluated at once more after the metrics pass, as ("blur_sigma", sigma) / ("jpeg_quality", quality) in the order
    written, blur first.  Either list may be absent; no key, no levels.  ValueError for a sigma outside 0..16 or a quality
    outside 1..100."""
    raw = infer_cfg.get("robustness")
    if not isinstance(raw, dict):
        return []
    levels: list[tuple[str, float | int]] = []
    for sigma in raw.get("blur_sigma") or []:
        levels.append(("blur_sigma", D.check_blur(1.0, float(sigma), float(sigma))[1]))
    for quality in raw.get("jpeg_quality") or []:
        levels.append(("jpeg_quality", D.check_jpeg(1.0, quality, quality)[1]))
    return levels


def robustness_tail(kind: str, level: float | int) -> D.GpuInputTail:
    """The eval tail that applies one perturbation level to every picture of the cropped uint8 batch: RandomBlur or RandomJpeg at
    probability 1 over a range of one value, so the same kernels as in training and nothing random in the result."""
    if kind == "blur_sigma":
        return D.GpuInputTail(IMAGENET_MEAN, IMAGENET_STD, blur=(1.0, level, level))
    return D.GpuInputTail(IMAGENET_MEAN, IMAGENET_STD, jpeg=(1.0, level, level))


def cam_limit(infer_cfg: dict[str, Any]) -> int | None:
    """Extra key `inference.cam`: Grad-CAM overlays of the first `limit` images of the split after the metrics pass.
    `{limit: 64}` / `{limit: all}` / `true` (all) / an integer; absent, `false`, `{enabled: false}` or a limit of 0: off (None)."""
    raw = infer_cfg.get("cam")
    if isinstance(raw, dict):
        if not as_bool(raw.get("enabled", True)):
            return None
        raw = raw.get("limit", "all")
    if raw is None or raw is False:
        return None
    if raw is True or str(raw).strip().lower() in ("all", "true", "yes", "on"):
        return sys.maxsize
    if str(raw).strip().lower() in ("", "false", "no", "off"):
        return None
    limit = int(raw)
    return limit if limit > 0 else None


def write_cam_overlays(model: nn.Module, dataset, probs: torch.Tensor, preds: torch.Tensor, limit: int, cam_dir: Path, *,
                       batch_size: int, num_workers: int) -> int:
    """Grad-CAM overlays (deepfakedetection_amd.cam) of the first `limit` images of `dataset`, each explaining the class the
    metrics pass predicted: <cam_dir>/<true_class>/<stem>__pred-<class>_<prob>.png plus one line per image in
    <cam_dir>/index.jsonl.  Returns the number of images written."""
    from PIL import Image

    from ..cam import GradCam

    n = min(limit, len(dataset))
    subset = torch.utils.data.Subset(dataset, range(n))
    subset.transform = getattr(dataset, "transform", None)           # build_inference_loader picks the collate function by it
    cam_dir.mkdir(parents=True, exist_ok=True)
    device = next(model.parameters()).device
    done = 0
    with (cam_dir / "index.jsonl").open("w", encoding="utf-8") as index, GradCam(model, batch_size=batch_size) as cam:
        for images, targets in build_inference_loader(dataset=subset, batch_size=batch_size, num_workers=num_workers):
            count = int(targets.shape[0])
            chosen = preds[done:done + count]
            if isinstance(images, torch.Tensor):
                images = images.to(device, non_blocking=True)
            overlays = cam(images, targets=chosen.to(device), overlay=True).overlay.cpu().numpy()
            for k in range(count):
                i = done + k
                path, truth = dataset.samples[i]
                pred = int(chosen[k])
                prob = float(probs[i, pred])
                dest = cam_dir / dataset.classes[truth] / f"{Path(path).stem}__pred-{dataset.classes[pred]}_{prob:.3f}.png"
                dest.parent.mkdir(parents=True, exist_ok=True)
                Image.fromarray(overlays[k]).save(dest, format="PNG")
                index.write(json.dumps({"path": str(path), "truth": dataset.classes[truth], "prediction": dataset.classes[pred],
                                        "probability": prob, "png": str(dest.relative_to(cam_dir.parent))}) + "\n")
            done += count
    return done


def best_balanced_accuracy_threshold(scores: np.ndarray, truth: np.ndarray, steps: int = 501) -> float:
    """First threshold on linspace(0,1,steps) that maximises balanced accuracy of
    (scores >= thr); same result as the reference's per-threshold sklearn loop (:533-544)."""
    thresholds = np.linspace(0.0, 1.0, steps, dtype=np.float64)
    pred = scores[None, :] >= thresholds[:, None]                  # [steps, n]
    pos, neg = truth == 1, truth == 0
    recall_pos = (pred & pos[None, :]).sum(1) / max(int(pos.sum()), 1)
    recall_neg = (~pred & neg[None, :]).sum(1) / max(int(neg.sum()), 1)
    return float(thresholds[int(np.argmax((recall_pos + recall_neg) / 2.0))])


def confusion_counts(truth: np.ndarray, pred: np.ndarray) -> np.ndarray:
    labels = np.unique(np.concatenate([truth, pred]))
    index = {int(label): i for i, label in enumerate(labels)}
    cm = np.zeros((len(labels), len(labels)), dtype=np.int64)
    for t, p in zip(truth.tolist(), pred.tolist()):
        cm[index[int(t)], index[int(p)]] += 1
    return cm


def _save_plots(cm: np.ndarray, labels: list[str], truth: np.ndarray, scores: np.ndarray | None, plots: Path, roc=None,
                reliability=None) -> None:
    """confusion_matrix.png / roc_curve.png; skipped quietly when matplotlib/sklearn are absent.  roc: a metrics.RocResult
    (inference.device_metrics) whose integer curve is drawn instead of sklearn's.  reliability: (temperature, the
    metrics.CalibrationResult at T = 1, the one at `temperature`) of inference.calibration, drawn as reliability.png: the
    accuracy per confidence bin against the diagonal, before and after."""
    try:
        import matplotlib

        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except Exception:  # noqa: BLE001
        return
    fig, ax = plt.subplots(figsize=(6, 5))
    ax.imshow(cm, cmap="Blues")
    ticks = range(cm.shape[0])
    ax.set_xticks(list(ticks), labels=[labels[i] if i < len(labels) else str(i) for i in ticks])
    ax.set_yticks(list(ticks), labels=[labels[i] if i < len(labels) else str(i) for i in ticks])
    for i in ticks:
        for j in ticks:
            ax.text(j, i, int(cm[i, j]), ha="center", va="center")
    ax.set_xlabel("Predicted label")
    ax.set_ylabel("True label")
    fig.tight_layout()
    fig.savefig(plots / "confusion_matrix.png")
    plt.close(fig)
    if reliability is not None:
        temperature, before, after = reliability
        fig, axes = plt.subplots(1, 2, figsize=(10, 5), sharey=True)
        for ax, res, title in ((axes[0], before, "T = 1"), (axes[1], after, f"T = {temperature:.4g}")):
            M_bins = len(res.count)
            centres = (np.arange(M_bins) + 0.5) / M_bins
            ax.bar(centres, np.nan_to_num(res.accuracy), width=1.0 / M_bins, edgecolor="black", alpha=0.7)
            ax.plot([0, 1], [0, 1], linestyle="--", color="gray")
            ece = "n/a" if res.ece is None else f"{res.ece:.4f}"
            ax.set_title(f"{title}  (ECE {ece})")
            ax.set_xlabel("Confidence")
            ax.set_xlim(0, 1)
            ax.set_ylim(0, 1)
        axes[0].set_ylabel("Accuracy")
        fig.tight_layout()
        fig.savefig(plots / "reliability.png")
        plt.close(fig)
    points = None
    if roc is not None:
        if roc.n_pos and roc.n_neg and not roc.nonfinite:
            fps, tps, _ = roc.curve()
            points = np.concatenate([[0.0], fps / roc.n_neg]), np.concatenate([[0.0], tps / roc.n_pos])
    elif scores is not None:
        try:
            from sklearn.metrics import roc_curve

            points = roc_curve(truth, scores)[:2]
        except Exception:  # noqa: BLE001
            return
    if points is not None:
        fig, ax = plt.subplots(figsize=(6, 5))
        ax.plot(*points)
        ax.set_title("ROC Curve")
        ax.set_xlabel("False Positive Rate")
        ax.set_ylabel("True Positive Rate")
        fig.tight_layout()
        fig.savefig(plots / "roc_curve.png")
        plt.close(fig)


def run_inference_job(*, config_path: Path, config: dict[str, Any], model_cfg: dict[str, Any], run_paths: RunPaths,
                      capture: bool = False) -> MemberScores | None:
    """capture (the job is a member of the `ensemble:` key): hand back what the ensemble fuses (MemberScores), else None."""
    console.print(f"[bold]→ inference {model_cfg['name']}[/]")
    log_path = run_paths.logs / "inference.log"
    log_path.unlink(missing_ok=True)
    with tee_output(log_path):
        return _run_inference_job(config_path=config_path, config=config, model_cfg=model_cfg, run_paths=run_paths, capture=capture)


def _resolve_weights(infer_cfg: dict[str, Any], model_name: str, out: Console) -> Path | None:
    value = infer_cfg.get("weights")
    if not value:
        return None
    path = Path(value).expanduser()
    if not path.is_absolute():
        path = (Path.cwd() / path).resolve()
    if not path.exists() and sys.stdin is not None and sys.stdin.isatty():
        answer = input(f"Missing weights at '{path}'. Download from GitHub Releases? [Y/N]: ").strip().lower()
        if answer == "y":
            if model_name in RELEASE_FILES:
                import urllib.request

                path.parent.mkdir(parents=True, exist_ok=True)
                urllib.request.urlretrieve(RELEASE_URL + RELEASE_FILES[model_name], str(path))
            else:
                out.print("[bold yellow]No download URL mapped for this model.[/]")
    return path


def _split_metrics(name: str, split: str, probs_t: torch.Tensor, preds_t: torch.Tensor, targets_t: torch.Tensor, num_classes: int,
                   threshold: float) -> tuple[dict[str, Any], torch.Tensor, np.ndarray]:
    """(one metrics.jsonl record, the predictions it judges, their confusion matrix) of one pass over a split; a binary problem
    predicts by `threshold` on the second class's probability."""
    if num_classes == 2:
        preds_t = (probs_t[:, 1] >= threshold).long()
    accuracy = (preds_t == targets_t).float().mean().item()
    metrics: dict[str, Any] = {"model": name, "split": split, "accuracy": accuracy, "timestamp": datetime.now().isoformat()}
    truth_np, pred_np = targets_t.numpy(), preds_t.numpy()
    if torch.unique(targets_t).numel() > 1:
        try:
            from sklearn.metrics import roc_auc_score

            if num_classes == 2:
                metrics["roc_auc"] = float(roc_auc_score(truth_np, probs_t[:, 1].numpy()))
            else:
                metrics["roc_auc"] = float(roc_auc_score(truth_np, probs_t.numpy(), multi_class="ovr"))
        except (ImportError, ValueError):
            pass
    if num_classes == 2:
        metrics["threshold"] = float(threshold)
    cm = confusion_counts(truth_np, pred_np)
    metrics["confusion_matrix"] = cm.tolist()
    return metrics, preds_t, cm


SWEEP_STEPS = 501           # best_balanced_accuracy_threshold's grid


def _device_threshold(book) -> float | None:
    """best_balanced_accuracy_threshold of a validation pass kept in a metrics.ScoreBook, from the device sweep; None when
    the pass saw one class only (or scores that are not finite): the caller keeps its default."""
    res = M.binary_roc(book.probs[:, 1], book.targets, cuts=np.linspace(0.0, 1.0, SWEEP_STEPS, dtype=np.float64), strict=False)
    if not res.n_pos or not res.n_neg or res.nonfinite:
        return None
    return res.best_balanced_accuracy_threshold()


def _split_metrics_device(name: str, split: str, book, num_classes: int, threshold: float):
    """_split_metrics of a pass kept in a metrics.ScoreBook (inference.device_metrics): the same record with the same keys, the
    AUC, the equal error rate and the confusion matrix from the device kernels (exact, no sklearn), plus `eer` and
    `balanced_accuracy` (mean recall over the classes that occur, at the record's predictions).  Returns (record, host
    probabilities, host predictions, host targets, confusion matrix, the binary RocResult or None): one transfer of the book."""
    probs_d, preds_d, targets_d = book.probs, book.preds, book.targets
    roc = None
    if num_classes == 2:
        preds_d = (probs_d[:, 1] >= threshold).long()
        roc = M.binary_roc(probs_d[:, 1], targets_d, strict=False)
        auc, eer = roc.auc, roc.eer
    else:
        per_class = [M.binary_roc(probs_d[:, j], targets_d, positive=j, strict=False) for j in range(num_classes)]
        present = all(r.n_pos and r.n_neg for r in per_class)
        auc = float(sum(r.auc for r in per_class) / num_classes) if present else None
        eer = float(sum(r.eer for r in per_class) / num_classes) if present else None
    full = M.confusion(targets_d, preds_d, num_classes).cpu().numpy()
    probs_t, preds_t, targets_t = probs_d.cpu(), preds_d.cpu(), targets_d.cpu()
    accuracy = (preds_t == targets_t).float().mean().item()
    record: dict[str, Any] = {"model": name, "split": split, "accuracy": accuracy, "timestamp": datetime.now().isoformat()}
    if auc is not None:
        record["roc_auc"] = auc
    if num_classes == 2:
        record["threshold"] = float(threshold)
    occurs = (full.sum(0) + full.sum(1)) > 0                    # the labels in truth or prediction, as confusion_counts keeps them
    cm = full[occurs][:, occurs]
    record["confusion_matrix"] = cm.tolist()
    rows = full.sum(1)
    record["eer"] = eer
    record["balanced_accuracy"] = float(np.mean(np.diag(full)[rows > 0] / rows[rows > 0])) if rows.any() else None
    return record, probs_t, preds_t, targets_t, cm, roc


def _validation_threshold(book) -> float | None:
    """The balanced-accuracy threshold of a binary validation pass, swept where the book lives; None: keep the default."""
    if book.probs.is_cuda:
        return _device_threshold(book)
    scores, truth = book.probs[:, 1].numpy(), book.targets.numpy()
    return best_balanced_accuracy_threshold(scores, truth) if scores.size and np.unique(truth).size > 1 else None


def _score_pass(model: nn.Module, dataset, s: InferenceSettings, book=None, tail=None, progress: Progress | None = None,
                keep_logits: bool = False):
    """One pass over `dataset` into `book`, which is returned: a metrics.ScoreBook, emptied first; None: a new one, on the device
    under inference.device_metrics (its rows arrive without a host round trip), with the logits under inference.calibration or
    `keep_logits` (a member of the ensemble)."""
    keep_logits = keep_logits or s.calibration is not None
    if book is None:
        book = M.ScoreBook(len(dataset), s.num_classes, s.device if s.device_metrics else "cpu", keep_logits=keep_logits)
    book.reset()
    loader = build_inference_loader(dataset=dataset, batch_size=s.batch_size, num_workers=s.num_workers)
    start = perf_counter()
    with progress if progress is not None else contextlib.nullcontext():
        task = progress.add_task("inference", total=len(loader), speed="") if progress is not None else None
        for images, targets in loader:
            probs, preds, logits = class_probabilities(model, images, s.device, s.amp, tail=tail, return_logits=True)
            book.append(probs, preds, targets.to(book.targets.device, non_blocking=True),
                        logits=logits if keep_logits else None)
            if progress is not None:
                progress.update(task, advance=1, speed=f"{book.count / max(perf_counter() - start, 1e-6):.1f} img/s")
    return book


@dataclass
class PassResult:
    """One judged pass: its metrics.jsonl record, what it was judged on (host tensors of its own) and what the plots take."""
    record: dict[str, Any]
    probs: torch.Tensor
    preds: torch.Tensor
    targets: torch.Tensor
    cm: np.ndarray
    roc: Any                        # the binary metrics.RocResult of a device book, else None
    reliability: Any                # (temperature, CalibrationResult at T = 1, at T) of a clean pass under calibration, else None
    group_record: dict[str, Any] | None = None      # the second record of the pass under inference.group_by, else None


@dataclass
class _Groups:
    """inference.group_by of one split: every sample's group id beside the book's rows (int32 on the book's device), the groups,
    those of one sample, the pooling mode and the threshold the pooled scores are judged at (the balanced-accuracy threshold of
    the pooled validation pass, else the frame path's default), held fixed for every level."""
    ids: torch.Tensor
    count: int
    singletons: int
    pool: str
    threshold: float = 0.5


def _split_groups(s: "InferenceSettings", paths: list[str], split: str, device) -> _Groups:
    key, pattern, pool = s.group_by
    ids, count, _ = M.group_ids(paths, s.root / split, key, pattern)
    sizes = np.bincount(ids, minlength=count)
    return _Groups(torch.from_numpy(ids).to(device), count, int((sizes == 1).sum()), pool)


def _pooled_book(book, groups: _Groups) -> M.ScoreBook:
    """The book of the groups' pooled scores.  group_ids keeps the class directory in every key, so no group mixes targets; a row
    that cannot be pooled (a probability that is NaN or outside [0, 1]) is an error here."""
    pooled = M.group_pool(book.probs, groups.ids, book.targets, groups.pool, positive=1 if book.num_classes > 1 else 0, num_groups=groups.count)
    if any(pooled.info):
        raise ValueError(f"inference.group_by: {pooled.info[0]} rows are not probabilities, {pooled.info[1]} ids are out of range and "
                         f"{pooled.info[3]} of {groups.count} groups are empty")
    out = M.ScoreBook(groups.count, book.num_classes, book.probs.device)
    out.append(pooled.probs, pooled.preds, pooled.targets)
    return out


def _group_record(s: "InferenceSettings", book, groups: _Groups) -> dict[str, Any]:
    """The pass judged per group: the pooled scores through the frame path's own record function, at the groups' threshold; under
    inference.bootstrap the ordinary bootstrap over the G pooled scores."""
    pooled = _pooled_book(book, groups)
    record, _, _, _, _, roc = _split_metrics_device(s.name, s.split, pooled, s.num_classes, groups.threshold)
    record.update(unit="group", pool=groups.pool, groups=groups.count, singletons=groups.singletons)
    if s.bootstrap is not None and roc is not None:
        record.update(_bootstrap_keys(pooled, groups.threshold, s.bootstrap, roc))
    return record


def _judge(s: InferenceSettings, book, threshold: float, calib: _Calibration | None, clean: bool = False,
           groups: _Groups | None = None) -> PassResult:
    """A filled book -> the pass's result: rescaled first under inference.calibration, then judged where the book lives.  groups
    (inference.group_by): the pass is judged per group too, and the frame record's intervals come from the cluster bootstrap."""
    figures, reliability = calib.apply(book, clean) if calib is not None else ({}, None)
    if book.probs.is_cuda:
        record, probs, preds, targets, cm, roc = _split_metrics_device(s.name, s.split, book, s.num_classes, threshold)
    else:
        probs, targets, roc = book.probs.clone(), book.targets.clone(), None        # the book is filled again by the next level
        record, preds, cm = _split_metrics(s.name, s.split, probs, book.preds.clone(), targets, s.num_classes, threshold)
    record.update(figures)
    if s.bootstrap is not None and roc is not None:
        record.update(_bootstrap_keys(book, threshold, s.bootstrap, roc, groups))
    group_record = _group_record(s, book, groups) if groups is not None else None
    return PassResult(record, probs, preds, targets, cm, roc, reliability, group_record)


BOOT_RECORD_METRICS = (("roc_auc", "auc"), ("eer", "eer"), ("accuracy", "accuracy"), ("balanced_accuracy", "balanced_accuracy"))


def _bootstrap_keys(book, threshold: float, settings: tuple[int, float, int], roc, groups: _Groups | None = None) -> dict[str, Any]:
    """The `ci` and `bootstrap` keys of a binary pass kept on the device: percentile intervals at the threshold in force, which is
    held fixed (its own uncertainty is not resampled).  Scores that are not finite leave ci None.  groups: the resamples draw
    whole groups (the cluster bootstrap), and `bootstrap` says so."""
    replicates, level, seed = settings
    about: dict[str, Any] = {"replicates": replicates, "seed": seed, "level": level, "degenerate": None}
    if groups is not None:
        about.update(cluster=True, groups=groups.count)
    if roc.nonfinite:
        return {"ci": None, "bootstrap": about}
    res = M.bootstrap(book.probs[:, 1], book.targets, cut=threshold, replicates=replicates, seed=seed, level=level,
                      groups=groups.ids if groups is not None else None)
    about["degenerate"] = res.degenerate()
    ci = {}
    for key, metric in BOOT_RECORD_METRICS:
        interval = res.interval(metric)
        ci[key] = list(interval) if interval is not None else None
    return {"ci": ci, "bootstrap": about}


def _emit(record: dict[str, Any], run_paths: RunPaths, out: Console, head: str) -> None:
    """One line more in logs/metrics.jsonl, and the console row: `head`, the accuracy, then the record's other float fields."""
    with (run_paths.logs / "metrics.jsonl").open("a", encoding="utf-8") as handle:
        handle.write(json.dumps(record) + "\n")
    extras = " ".join(f"{k}={v:.4f}" for k, v in record.items() if isinstance(v, float) and k != "accuracy")
    out.print(f"{head} {record['accuracy']:.4f} {extras}")


class _Calibration:
    """inference.calibration of one job: the bins, the mode ("fit" or the temperature given), the temperature in force and the
    calibration.json document.  The passes it judges are kept with their logits (ScoreBook(keep_logits=True))."""

    def __init__(self, bins: int, mode: str | float) -> None:
        self.bins, self.mode, self.temperature = bins, mode, 1.0 if mode == "fit" else float(mode)
        self.doc = dict(temperature=self.temperature, bins=bins, fitted_on=None, n=0, nll_before=None, nll_after=None)

    def fit(self, book, fitted_on: str, out: Console) -> None:
        """Settle the temperature on the validation pass (None: there was none) and leave that pass rescaled for the threshold sweep."""
        if self.mode == "fit" and book is None:
            out.print("[bold yellow]inference.calibration[/]: no validation split to fit the temperature on; T = 1 is used")
            self.doc["temperature_fit"] = "unavailable"
        elif self.mode == "fit":
            fit = M.fit_temperature(book.logits, book.targets)
            self.doc.update(fitted_on=fitted_on, n=book.count, nll_before=fit.nll_before, nll_after=fit.nll_after)
            if fit.at_bound:
                out.print(f"[bold yellow]inference.calibration[/]: the fitted temperature sits at its bound "
                          f"{fit.temperature:g}; T = 1 is used")
                self.doc["temperature_fit"] = "at_bound"
            else:
                self.temperature = self.doc["temperature"] = float(fit.temperature)
        if book is not None:
            self._rescale(book)

    def _rescale(self, book) -> None:
        probs, preds = M.apply_temperature(book.logits, self.temperature)       # softmax / arg max of logits / T
        book.probs.copy_(probs)
        book.preds.copy_(preds)

    def _figures(self, book, temperature: float):
        res = M.calibration(book.probs, book.targets, self.bins)
        return {"ece": res.ece, "mce": res.mce, "brier": res.brier, "nll": M.mean_nll(book.logits, book.targets, temperature)}, res

    def apply(self, book, clean: bool = False):
        """Rescale a pass -> (its record's calibration keys, None).  clean: plus the figures at T = 1 and _save_plots' reliability."""
        before = self._figures(book, 1.0) if clean else None
        self._rescale(book)
        after = self._figures(book, self.temperature)
        keys = {"temperature": float(self.temperature), **after[0]}
        if clean:
            keys.update(uncalibrated=before[0], **{k: v for k, v in self.doc.items() if k == "temperature_fit"})
        return keys, (self.temperature, before[1], after[1]) if clean else None

    def write(self, run_dir: Path) -> None:
        (run_dir / "calibration.json").write_text(json.dumps(self.doc, indent=2) + "\n", encoding="utf-8")


@dataclass(frozen=True)
class InferenceSettings:
    """What the inference job reads from the YAML, every fallback applied (inference_settings)."""
    name: str
    root: Path
    split: str
    val_split: str
    num_classes: int
    image_size: int
    batch_size: int
    num_workers: int
    amp: bool                                       # extra key `amp: bf16`; default: f32 as the reference
    device: torch.device
    fp8_weights: bool                               # extra key (FasterViT, with `amp: bf16`): Linear weights as MX fp8 (fp8 MFMA)
    transform: D.Compose                            # extra key `gpu_resize`: the workers only decode, the device does the rest
    device_metrics: bool                            # extra key: the passes stay on the device, judged by the exact counting kernels
    calibration: tuple[int, str | float] | None     # extra key (calibration_settings): the passes keep their logits, T rescales them
    robustness: tuple[tuple[str, float | int], ...]         # the robustness_levels that can run (the device pipeline's batch is perturbed)
    cam_limit: int | None                           # None also where Grad-CAM cannot run
    bootstrap: tuple[int, float, int] | None = None     # extra key (bootstrap_settings): every judged pass gains `ci` and `bootstrap`
    group_by: tuple[str, str | None, str] | None = None     # extra key (group_settings): every judged pass gains a record per group


def inference_settings(config: dict[str, Any], model_cfg: dict[str, Any], out: Console) -> InferenceSettings:
    """The job's settings from the configuration alone (no model, no data): an extra key that cannot take effect warns on `out`."""
    on = ("1", "true", "yes", "on")
    name = model_cfg["name"]
    data_cfg = config.get("data") or {}
    infer_cfg = model_cfg.get("inference") or {}        # reference uses .get("inference", {}) and breaks on None
    split = infer_cfg.get("split") or data_cfg.get("test_split", "test")
    batch_size = int(infer_cfg.get("batch_size", 64))
    out.print(f"[bold]Model[/]: {name} | split={split} | batch={batch_size}")
    image_size = int(_first_set(infer_cfg.get("img_size"), data_cfg.get("img_size"), get_model_spec(name).default_image_size))
    device = torch.device(config.get("device") or "cuda")
    if device.type == "cuda" and not torch.cuda.is_available():
        out.print("[bold yellow]⚠️  CUDA requested but unavailable[/]: using CPU")
        device = torch.device("cpu")
    eval_toggles = resolve_transform_mapping(model_cfg, phase="eval")
    transform, gpu_resize = build_eval_transforms(image_size, toggles=eval_toggles), False
    if str(infer_cfg.get("gpu_resize", "")).lower() in on and device.type == "cuda":
        # The device pipeline (bit-exact with PIL, tests/test_ops_gpu.py::test_resize_crop_matches_pillow_bit_for_bit) IS the default
        # eval pipeline: with an eval toggle off its results would silently differ, so it engages only under the default toggles.
        switched_off = sorted(k for k in ("ensure_rgb", "val_resize", "val_center_crop", "val_to_tensor", "val_normalize")
                              if not as_bool((eval_toggles or {}).get(k, True)))
        if switched_off:
            out.print(f"[bold yellow]inference.gpu_resize ignored[/]: eval toggles {switched_off} are off; the PIL pipeline honours them")
        else:
            transform = D.Compose([D.Lambda(_to_rgb), D.PlanGeometry("center", image_size, image_size)])
            gpu_resize = True
    root = Path(data_cfg.get("root")).expanduser()
    device_metrics = as_bool(infer_cfg.get("device_metrics", False))
    if device_metrics and device.type != "cuda":
        out.print("[bold yellow]inference.device_metrics ignored[/]: needs a CUDA device; the host metrics run")
        device_metrics = False
    calibration = calibration_settings(infer_cfg)
    if calibration is not None and not device_metrics:
        out.print("[bold yellow]inference.calibration ignored[/]: needs inference.device_metrics on a CUDA device")
        calibration = None
    num_classes = int(model_cfg.get("num_classes", data_cfg.get("num_classes", 2)))
    bootstrap = bootstrap_settings(infer_cfg.get("bootstrap"))
    if bootstrap is not None and not (device_metrics and num_classes == 2):
        out.print("[bold yellow]inference.bootstrap ignored[/]: needs inference.device_metrics on a CUDA device and a binary problem")
        bootstrap = None
    group_by = group_settings(infer_cfg.get("group_by"))
    if group_by is not None and not device_metrics:
        out.print("[bold yellow]inference.group_by ignored[/]: needs inference.device_metrics on a CUDA device")
        group_by = None
    levels = robustness_levels(infer_cfg)
    if levels and not gpu_resize:           # the perturbation is applied to the cropped uint8 batch of the device pipeline
        out.print("[bold yellow]inference.robustness skipped[/]: needs inference.gpu_resize on a CUDA device")
        levels = []
    elif image_size * image_size > BLUR_MAX_PIXELS and any(kind == "blur_sigma" for kind, _ in levels):
        out.print(f"[bold yellow]inference.robustness blur_sigma skipped[/]: dfd_blur_u8 takes at most {BLUR_MAX_PIXELS} pixels")
        levels = [(kind, level) for kind, level in levels if kind != "blur_sigma"]
    limit = cam_limit(infer_cfg)
    if limit is not None and device.type != "cuda":
        out.print("[bold yellow]inference.cam skipped[/]: Grad-CAM runs on the HIP device only")
        limit = None
    return InferenceSettings(
        name=name, root=root if root.is_absolute() else (Path.cwd() / root).resolve(), split=split,
        val_split=str(data_cfg.get("val_split", "val")), num_classes=num_classes,
        image_size=image_size, batch_size=batch_size, num_workers=int(infer_cfg.get("num_workers", 4)),
        amp=str(infer_cfg.get("amp", "")).lower() in ("bf16", "bfloat16", "true", "1"), device=device,
        fp8_weights=str(infer_cfg.get("fp8_weights", "")).lower() in on, transform=transform,
        device_metrics=device_metrics, calibration=calibration, bootstrap=bootstrap, group_by=group_by, robustness=tuple(levels), cam_limit=limit)


@dataclass
class MemberScores:
    """What one inference job leaves for the ensemble (run_ensemble_job): device tensors of its own, the logits as the network
    gave them (a fitted temperature is kept beside them, not applied)."""
    settings: InferenceSettings
    classes: list[str]
    paths: list[str]                                # the split's sample paths, in the order of the rows
    val: tuple[torch.Tensor, torch.Tensor] | None   # (logits, targets) of the validation split; None: there was none
    val_paths: list[str]
    clean: tuple[torch.Tensor, torch.Tensor]        # (logits, targets) of the clean pass
    preds: torch.Tensor                             # the predictions the clean record judges (host)
    levels: dict[tuple[str, float | int], torch.Tensor]     # the logits of every robustness level
    temperature: float | None                       # inference.calibration's temperature, if any
    record: dict[str, Any]                          # the clean pass's metrics.jsonl record


def _run_inference_job(*, config_path: Path, config: dict[str, Any], model_cfg: dict[str, Any], run_paths: RunPaths,
                       capture: bool = False) -> MemberScores | None:
    tty = getattr(sys.stdout, "isatty", None)
    out = Console(file=sys.stdout, force_terminal=bool(tty()) if callable(tty) else False)
    s = inference_settings(config, model_cfg, out)
    model = load_model(s.name, s.num_classes, _resolve_weights(model_cfg.get("inference") or {}, s.name, out), s.device, s.image_size)
    if s.fp8_weights and hasattr(model, "fp8_weights"):
        model.fp8_weights = True
    calib = _Calibration(*s.calibration) if s.calibration is not None else None
    capture = capture and s.device_metrics          # the ensemble fuses logits kept on the device
    threshold = group_threshold = 0.5
    val_scores, val_paths = None, []
    if s.num_classes == 2 or (calib is not None and calib.mode == "fit") or capture:
        val_dir = s.root / s.val_split
        val_set = D.ImageFolder(val_dir, transform=s.transform) if val_dir.exists() else ()
        val_book = _score_pass(model, val_set, s, keep_logits=capture) if len(val_set) > 0 else None
        if capture and val_book is not None:
            val_scores, val_paths = (val_book.logits.clone(), val_book.targets.clone()), [str(path) for path, _ in val_set.samples]
        if calib is not None:
            calib.fit(val_book, s.val_split, out)
        if val_book is not None and s.num_classes == 2:
            threshold = _first_set(_validation_threshold(val_book), threshold)
            if s.group_by is not None:
                val_groups = _split_groups(s, [str(path) for path, _ in val_set.samples], s.val_split, s.device)
                group_threshold = _first_set(_validation_threshold(_pooled_book(val_book, val_groups)), group_threshold)
        del val_book                                    # its device buffers go before the split's own book is made

    split_dir = s.root / s.split
    if not split_dir.exists():
        out.print(f"[bold red]Split not found:[/] {split_dir}")
        raise SystemExit(1)
    dataset = D.ImageFolder(split_dir, transform=s.transform)
    require_num_classes(dataset, s.num_classes, split=s.split, dataset_root=split_dir)
    if len(dataset) == 0:
        out.print(f"[bold yellow]No images found in[/] {split_dir}")
        return None
    progress = Progress(TextColumn("[bold blue]{task.description}"), BarColumn(bar_width=None), MofNCompleteColumn(),
                        TimeElapsedColumn(), TimeRemainingColumn(), TextColumn("{task.fields[speed]}"), console=out)
    book = _score_pass(model, dataset, s, progress=progress, keep_logits=capture)   # one book for this pass and every level below
    clean_scores = (book.logits.clone(), book.targets.clone()) if capture else None
    groups = None
    if s.group_by is not None:
        groups = replace(_split_groups(s, [str(path) for path, _ in dataset.samples], s.split, s.device), threshold=group_threshold)
    clean = _judge(s, book, threshold, calib, clean=True, groups=groups)
    if calib is not None:
        calib.write(run_paths.run_dir)
    scores = clean.probs[:, 1].numpy() if s.num_classes == 2 and torch.unique(clean.targets).numel() > 1 else None
    _save_plots(clean.cm, list(dataset.classes), clean.targets.numpy(), scores, run_paths.plots, roc=clean.roc,
                reliability=clean.reliability)
    _emit(clean.record, run_paths, out, "[bold]Accuracy[/]:")
    if clean.group_record is not None:
        _emit(clean.group_record, run_paths, out, f"[bold]Accuracy per group[/] ({groups.count} groups, {groups.pool}):")
    levels = {}
    for kind, level in s.robustness:
        _score_pass(model, dataset, s, book, tail=robustness_tail(kind, level), keep_logits=capture)
        if capture:
            levels[(kind, level)] = book.logits.clone()
        judged = _judge(s, book, threshold, calib, groups=groups)   # at the clean pass's thresholds and temperature
        for perturbed, unit in ((judged.record, ""), (judged.group_record, " per group")):
            if perturbed is not None:
                perturbed["perturbation"] = {kind: level}
                _emit(perturbed, run_paths, out, f"[bold]Robustness[/] {kind}={level:g}: accuracy{unit}")
    if s.cam_limit is not None:
        count = write_cam_overlays(model, dataset, clean.probs, clean.preds, s.cam_limit, run_paths.run_dir / "cam",
                                   batch_size=s.batch_size, num_workers=s.num_workers)
        out.print(f"[bold]Grad-CAM[/]: {count} overlays in {run_paths.run_dir / 'cam'}")
    if not capture:
        return None
    return MemberScores(settings=s, classes=list(dataset.classes), paths=[str(path) for path, _ in dataset.samples], val=val_scores,
                        val_paths=val_paths, clean=clean_scores, preds=clean.preds, levels=levels,
                        temperature=float(calib.temperature) if calib is not None else None, record=clean.record)


def _fused_book(members: list[MemberScores], logits: list[torch.Tensor], targets: torch.Tensor, ens: EnsembleSettings, weights) -> M.ScoreBook:
    """The members' logits of one pass, fused into a device book that keeps the fused logits."""
    probs, preds, fused = M.fuse(logits, weights, ens.mode, [m.temperature for m in members])
    book = M.ScoreBook(targets.shape[0], members[0].settings.num_classes, targets.device, keep_logits=True)
    book.append(probs, preds, targets, logits=fused)
    return book


def _ensemble_figures(book) -> dict[str, Any]:
    res = M.calibration(book.probs, book.targets)
    return {"ece": res.ece, "mce": res.mce, "brier": res.brier, "nll": M.mean_nll(book.logits, book.targets)}


def _ensemble_vs_members(book, threshold: float, names: list[str], members: list[MemberScores], settings: tuple[int, float, int]) -> dict[str, Any]:
    """ensemble.json's `vs_members`: per member the paired bootstrap of ensemble minus member on the clean pass, in AUC and in
    accuracy, each side at its own record's threshold and temperature.  One metrics.bootstrap call scores the ensemble beside up to
    BOOT_MAX_MEMBERS - 1 members; a larger ensemble takes a second call, which draws the same resamples from the same seed."""
    replicates, level, seed = settings
    targets = book.targets
    out: dict[str, Any] = {}
    for start in range(0, len(members), BOOT_MAX_MEMBERS - 1):
        part = list(zip(names, members))[start:start + BOOT_MAX_MEMBERS - 1]
        scores = [book.probs[:, 1]] + [M.apply_temperature(m.clean[0], m.temperature if m.temperature is not None else 1.0)[0][:, 1]
                                       for _, m in part]
        cuts = [float(threshold)] + [float(m.record.get("threshold", 0.5)) for _, m in part]
        res = M.bootstrap(scores, targets, cut=cuts, replicates=replicates, seed=seed, level=level)
        for k, (name, _) in enumerate(part, start=1):
            out[name] = {"auc": asdict(res.delta("auc", 0, k)), "accuracy": asdict(res.delta("accuracy", 0, k))}
    return out


def run_ensemble_job(ens: EnsembleSettings, names: list[str], members: list[MemberScores], run_paths: RunPaths) -> None:
    """Fuse the members' kept logits (metrics.fuse), judge the fused passes as a member's are judged and write ensemble.json."""
    console.print(f"[bold]→ ensemble of {', '.join(names)}[/]")
    log_path = run_paths.logs / "ensemble.log"
    log_path.unlink(missing_ok=True)
    with tee_output(log_path):
        _run_ensemble_job(ens, names, members, run_paths)


def _run_ensemble_job(ens: EnsembleSettings, names: list[str], members: list[MemberScores], run_paths: RunPaths) -> None:
    tty = getattr(sys.stdout, "isatty", None)
    out = Console(file=sys.stdout, force_terminal=bool(tty()) if callable(tty) else False)
    first, count = members[0], len(members)
    for name, m in zip(names[1:], members[1:]):
        if m.paths != first.paths or not torch.equal(m.clean[1], first.clean[1]):
            raise ValueError(f"ensemble: {name} scored other samples or targets of split {first.settings.split!r} than {names[0]}")
        if (m.val is None) != (first.val is None) or m.val_paths != first.val_paths or \
                (m.val is not None and not torch.equal(m.val[1], first.val[1])):
            raise ValueError(f"ensemble: {name} scored other samples or targets of split {first.settings.val_split!r} than {names[0]}")
    boot = ens.bootstrap
    if boot is not None and first.settings.num_classes != 2:
        out.print("[bold yellow]ensemble.bootstrap ignored[/]: needs a binary problem")
        boot = None
    s = replace(first.settings, name="ensemble", calibration=None, bootstrap=boot)
    temperatures = [m.temperature for m in members]
    doc: dict[str, Any] = {"members": list(names), "mode": ens.mode, "weights": ens.weights if isinstance(ens.weights, str) else "given",
                           "temperatures": temperatures, "fit": None}
    weights = [1.0 / count] * count if isinstance(ens.weights, str) else list(ens.weights)
    if ens.weights == "fit":
        start = [w / (t if t is not None else 1.0) for w, t in zip(weights, temperatures)]         # 1 / (K T_k)
        if first.val is None:
            out.print("[bold yellow]ensemble[/]: no validation split to fit the weights on; the start 1 / (K T_k) is used")
            doc["fit"] = "unavailable"
        else:
            fit = M.fit_fusion([m.val[0] for m in members], first.val[1], start=start, l2=ens.l2)
            doc["fit"] = asdict(fit)
            if fit.at_bound:
                out.print("[bold yellow]ensemble[/]: the fitted weights left their bound (the validation split is separable); "
                          "the start 1 / (K T_k) is used")
            else:
                temperatures = [None] * count                           # the fitted coefficients multiply the logits as they are
                weights = list(fit.coef)
    fold = ens.mode == "logit"
    doc["coefficients"] = [w / (t if fold and t is not None else 1.0) for w, t in zip(weights, temperatures)]
    pooled = [replace(m, temperature=t) for m, t in zip(members, temperatures)]

    threshold = group_threshold = 0.5
    if first.val is not None and s.num_classes == 2:
        val_book = _fused_book(pooled, [m.val[0] for m in members], first.val[1], ens, weights)
        threshold = _first_set(_validation_threshold(val_book), threshold)
        if s.group_by is not None:
            val_groups = _split_groups(s, first.val_paths, s.val_split, first.val[1].device)
            group_threshold = _first_set(_validation_threshold(_pooled_book(val_book, val_groups)), group_threshold)
        del val_book
    groups = None
    if s.group_by is not None:                                          # the members share their paths: one grouping for all
        groups = replace(_split_groups(s, first.paths, s.split, first.clean[1].device), threshold=group_threshold)
    book = book_clean = _fused_book(pooled, [m.clean[0] for m in members], first.clean[1], ens, weights)
    clean = _judge(s, book, threshold, None, clean=True, groups=groups)
    clean.record.update(_ensemble_figures(book))
    scores = clean.probs[:, 1].numpy() if s.num_classes == 2 and torch.unique(clean.targets).numel() > 1 else None
    _save_plots(clean.cm, first.classes, clean.targets.numpy(), scores, run_paths.plots, roc=clean.roc)
    _emit(clean.record, run_paths, out, "[bold]Ensemble accuracy[/]:")
    if clean.group_record is not None:
        _emit(clean.group_record, run_paths, out, f"[bold]Ensemble accuracy per group[/] ({groups.count} groups, {groups.pool}):")
    for kind, level in first.settings.robustness:
        if not all((kind, level) in m.levels for m in members):
            continue
        book = _fused_book(pooled, [m.levels[(kind, level)] for m in members], first.clean[1], ens, weights)
        judged = _judge(s, book, threshold, None, groups=groups)        # at the clean pass's thresholds and coefficients
        judged.record.update(_ensemble_figures(book))
        for perturbed, unit in ((judged.record, ""), (judged.group_record, " per group")):
            if perturbed is not None:
                perturbed["perturbation"] = {kind: level}
                _emit(perturbed, run_paths, out, f"[bold]Ensemble robustness[/] {kind}={level:g}: accuracy{unit}")

    device = first.clean[1].device
    div = M.diversity([m.preds.to(device) for m in members], first.clean[1], s.num_classes)    # of the predictions the records judge
    doc["diversity"] = asdict(div)
    doc["clean"] = {name: {"accuracy": rec.get("accuracy"), "roc_auc": rec.get("roc_auc")}
                    for name, rec in [*zip(names, (m.record for m in members)), ("ensemble", clean.record)]}
    doc["threshold"] = float(threshold)
    if boot is not None and not clean.roc.nonfinite:
        doc["vs_members"] = _ensemble_vs_members(book_clean, threshold, names, members, boot)
    (run_paths.run_dir / "ensemble.json").write_text(json.dumps(doc, indent=2) + "\n", encoding="utf-8")
    out.print(f"[bold]Ensemble[/]: coefficients {doc['coefficients']} | oracle accuracy {div.oracle_accuracy} | {run_paths.run_dir / 'ensemble.json'}")


def ensemble_obstacle(ens: EnsembleSettings, captured: dict[str, MemberScores | None]) -> str | None:
    """Why the ensemble cannot run on what the member jobs left (None: it can): every member must have kept its scores on the
    device, and all must share the split, the validation split and the classes."""
    absent = [name for name in ens.members if captured.get(name) is None]
    if absent:
        return f"{', '.join(absent)} kept no scores: every member needs inference.device_metrics on a CUDA device (and a split with images)"
    settings = [captured[name].settings for name in ens.members]
    for key in ("split", "val_split", "num_classes"):
        values = {getattr(s, key) for s in settings}
        if len(values) > 1:
            return f"the members differ in {key}: {sorted(map(str, values))}"
    return None


def orchestrate(config_path: Path, *, mode: str) -> None:
    config = load_config(config_path)
    apply_seed(config.get("seed"))
    models_cfg = config.get("models", {})
    if not isinstance(models_cfg, dict):
        raise TypeError("models section must be a mapping of name -> config")
    selection = config.get("selection")
    names = list(models_cfg) if selection is None else [str(n) for n in selection]
    ens = ensemble_settings(config, console) if mode == "inference" else None
    captured: dict[str, MemberScores | None] = {}
    for name in names:
        base = models_cfg.get(name)
        if base is None:
            console.print(f"[bold yellow]Skipping unknown model[/]: {name}")
            continue
        model_cfg = {"name": name, **base}
        run_paths = ensure_run_dirs(Path(model_cfg.get("output_dir") or f"runs/{name}"), datetime.now().strftime("%Y%m%d-%H%M%S"))
        snapshot_config(run_paths, config=config, model_cfg=model_cfg)
        if mode == "training":
            run_training_job(config, model_cfg, run_paths)
        elif mode == "inference":
            member = ens is not None and name in ens.members
            scores = run_inference_job(config_path=config_path, config=config, model_cfg=model_cfg, run_paths=run_paths, capture=member)
            if member:
                captured[name] = scores
        else:
            raise ValueError(f"Unknown mode '{mode}'")
    if ens is not None:
        obstacle = ensemble_obstacle(ens, captured)
        if obstacle is not None:
            console.print(f"[bold yellow]ensemble skipped[/]: {obstacle}")
            return
        run_paths = ensure_run_dirs(ens.output_dir, datetime.now().strftime("%Y%m%d-%H%M%S"))
        run_ensemble_job(ens, list(ens.members), [captured[name] for name in ens.members], run_paths)


def run_cli() -> None:
    parser = argparse.ArgumentParser(description="DeepfakeDetection orchestrator (MI355X engine)")
    parser.add_argument("--mode", choices=["training", "inference"], default="training")
    parser.add_argument("--config", type=Path)
    args = parser.parse_args()
    path = args.config or Path("config/train.yaml" if args.mode == "training" else "config/inference.yaml")
    orchestrate(path.resolve(), mode=args.mode)


if __name__ == "__main__":
    run_cli()
