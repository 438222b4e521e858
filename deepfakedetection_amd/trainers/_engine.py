"""The one training engine of the EfficientNet, EfficientFormerV2 and FasterViT trainers on the MI355X.

The reference keeps three near-identical scripts (trainers/efficientnet.py, efficientformer_v2.py, fastervit.py).  Here the
epoch loop, the evaluation loop, the throughput log and the phase driver exist once; a trainer module is its constants, a
`TrainerSpec` and `main()`.  The spec carries what differs — this table is the one list of it:

  behaviour (spec field)                  efficientnet.py                     efficientformer_v2.py               fastervit.py
  warm-up trainable set (warmup_keys)     "_fc" or "classifier" (:433-437)    "classifier" or "head" (:351-352)   "head" (:400-402)
  fine-tune trainable set (unfreeze_keys) all (:479-480)                      UNFREEZE_KEYS (:66-74, :389-393)    all (:434-435)
  fine-tune batch x accum (ft_*)          $FT_BATCH_SIZE 32 x $ACCUM_STEPS 4  BATCH_SIZE, none (:419-430)         32 x 4 hard-coded (:437-453)
  zero_grad (zero_grad_first)             epoch start + after the step        before the forward (:242)           after the step (:278-283)
  warm-up zero_grad (warmup_zero_grad_first)  epoch start + after the step    before the forward (:362-382)       before the forward (:408-428)
  losses (report_loss)                    evaluate: accuracy + mean CE;       accuracy only (:206-219)            accuracy only (:224-240)
                                          epoch: mean loss over ranks
  early stop (early_stop)                 EARLY_STOP_PATIENCE                 no                                  EARLY_STOP_PATIENCE (:322, :526)
  transforms (transform_kwargs)           build_transforms defaults           rotation / erasing off, jitter 0.1, rotation after flip (both)
  model (pass_img_size)                   builder(name, classes)              builder(name, classes, img_size)    builder(name, classes)
  console lines (warmup_line, epoch_line, with val_loss / train_loss, counts  bare val_acc; EMA with counts       val_acc, counts, lr; EMA with counts
                 ema_line)                and lr
  warm-up progress (warmup_task,          "warmup (head only)",               "warmup", rate in the extra column (both)
                    warmup_label)         train | loss | img/s

Everything else — env contract, phases, checkpoints, file names, SystemExit paths — is the reference's.  Deliberate
differences, all keeping the reference's defaults: the model is `get_model_spec($MODEL_NAME).builder`,
pretrained weights come from $PRETRAINED / weights/<name>.pth if present (no network), else random init with a warning;
bf16 autocast and a disabled GradScaler kept for API parity; HIP loss / AdamW on a cuda device; one host sync per LOG_EVERY
steps instead of a `loss.item()` per iteration; `prefetch_factor` only with workers; WORLD_SIZE > 1 (torchrun) shards the
minibatches over ranks, all-reduces gradients over RCCL, rank 0 logs and writes checkpoints; `logs/throughput.jsonl`.
"""

from __future__ import annotations

import json
import math
from dataclasses import dataclass, field
from pathlib import Path
from time import perf_counter, time

import torch
from rich.progress import BarColumn, MofNCompleteColumn, Progress, TaskID, TextColumn, TimeElapsedColumn, TimeRemainingColumn
from torch import nn, optim
from torch.utils.data import DataLoader

from ..dp import GradAllReducer, all_reduce_counts, broadcast_module_state, init_distributed
from ..orchestration.model_registry import get_model_spec
from ..orchestration.train_env import (
    apply_seed, as_bool, create_console, env_float, env_int, env_path, env_str, maybe_load_checkpoint, prepare_training_environment,
    save_best_checkpoint, save_latest_checkpoint,
)
from ._inputs import balanced_sampling, blur_settings, device_batches, get_loaders, jpeg_settings, make_loader, policy_settings

DATA_ROOT = Path.home() / "code" / "DeepfakeDetection" / "data" / "Dataset"
LOG_EVERY = 10
ACC = "val_acc={res.acc:.4f}"                           # pieces of the console lines below: str.format templates
ACC_COUNTS = ACC + " ({res.correct}/{res.total})"

console = create_console()      # re-bound by every run(): LOG_PATH differs per orchestrated run


@dataclass(frozen=True)
class TrainerSpec:
    model_name: str
    best_weights_name: str
    default_epochs: int
    default_batch_size: int
    warmup_keys: tuple[str, ...]
    unfreeze_keys: tuple[str, ...] | None           # None: fine-tune everything
    ft_batch_size: int | None = None                # None: BATCH_SIZE batches, no `Fine-tune:` line
    ft_accum_steps: int = 1
    ft_from_env: bool = False                       # the two above are the defaults of $FT_BATCH_SIZE / $ACCUM_STEPS
    zero_grad_first: bool = False
    warmup_zero_grad_first: bool = True
    report_loss: bool = False                       # evaluate() adds the mean CE loss, an epoch its mean training loss
    early_stop: bool = False
    default_patience: int = 4
    default_img_size: int = 224
    default_num_workers: int = 8
    head_lr: float = 3e-4
    head_wd: float = 5e-2
    ft_lr: float = 1e-4
    ft_wd: float = 5e-2
    pass_img_size: bool = False                      # builder takes img_size (EfficientFormerV2 bias tables)
    transform_kwargs: dict | None = field(default_factory=lambda: dict(      # None: build_transforms' own defaults
        rotation_default=False, erasing_default=False, jitter=(0.1, 0.1, 0.1, 0.05), rotation_after_flip=True))
    warmup_task: str = "warmup"
    warmup_label: str | None = "warmup"             # progress text `<label> | loss` + rate in the extra column; None: as training
    warmup_line: str = ACC                          # formatted with res=EvalResult
    epoch_line: str = ACC                           # res, train_loss (None without report_loss), lr
    ema_line: str = ACC_COUNTS                      # res (of the EMA model)


@dataclass(frozen=True)
class EvalResult:
    acc: float
    total: int
    correct: int
    loss: float | None = None                       # mean CE loss when evaluate() got a criterion
    auc: float | None = None                        # ROC-AUC over all ranks' validation scores (val_auc; macro one-vs-rest above two classes)
    eer: float | None = None                        # equal error rate (val_auc, two classes)


@dataclass(frozen=True)
class EpochResult:
    stats: dict                                     # throughput figures for logs/throughput.jsonl
    loss: float | None = None                       # mean training loss over all ranks (with_loss)
    clip: dict | None = None                        # the epoch's gradient-clipping record (clip_settings() on)


@dataclass(frozen=True)
class MetricSettings:
    val_auc: bool           # evaluate() also reports the exact ROC-AUC (metrics.binary_roc on the device)
    select: str             # "acc" or "auc": what the best epoch, early stopping and the best-weights file follow


def metric_settings() -> MetricSettings:
    """$VAL_AUC (YAML training.val_auc, default off) and $SELECT_METRIC (training.select_metric: acc | auc, default acc —
    today's behaviour); selecting by AUC switches val_auc on."""
    select = env_str("SELECT_METRIC", "acc").strip().lower() or "acc"
    if select not in ("acc", "auc"):
        raise ValueError(f"SELECT_METRIC must be acc or auc, got {select!r}")
    return MetricSettings(val_auc=as_bool(env_str("VAL_AUC", "0")) or select == "auc", select=select)


def selection_value(res: "EvalResult", metric: str) -> float | None:
    """The figure of an evaluation that the best epoch follows; None (no AUC: a class is absent, or a diverged epoch's scores
    are not finite) never counts as an improvement."""
    if metric == "auc":
        return None if res.auc is None or math.isnan(res.auc) else res.auc
    return res.acc


def improves(value: float | None, best: float) -> bool:
    return value is not None and value > best + 1e-4


def auc_suffix(res: "EvalResult") -> str:
    return "" if res.auc is None else f" | auc={res.auc:.4f}"


def eval_forward(model: nn.Module, device: str):
    """The callable evaluate() runs per batch: the model itself, or — on a HIP device, unless GRAPH_STEP is off — a
    graph_step.GraphedForward kept on the model, which replays the eval-mode forward per batch shape (bit-identical to
    the eager forward; at the reference's validation batch sizes the eager forward is host-bound)."""
    if not str(device).startswith("cuda") or env_str("GRAPH_STEP", "1").lower() in {"0", "false", "no", "off"}:
        return model
    fwd = model.__dict__.get("_graphed_eval")
    if fwd is None:
        from ..graph_step import GraphedForward

        fwd = model.__dict__["_graphed_eval"] = GraphedForward(model)
    return fwd


def make_stepper(model: nn.Module, criterion: nn.Module, opt, *, accum_steps: int, use_cuda: bool, world: int, reducer=None,
                 ema=None):
    """hipGraph replay of the loop body ($GRAPH_STEP, YAML training.graph_step; default on) on a HIP device with the
    HIP optimizer; with `world` > 1 the object also drives the gradient exchange (`reducer`): graph(zero_grad + forward +
    backward) -> all-reduce of the flat gradient arena (RCCL, outside of capture) -> graph(AdamW [+ EMA update]).  Otherwise
    None: the loop runs eagerly as the reference's does."""
    if not use_cuda or getattr(opt, "arena", None) is None or (world > 1 and reducer is None):
        return None
    if env_str("GRAPH_STEP", "1").lower() in {"0", "false", "no", "off"}:
        return None
    from ..graph_step import GraphedTrainStep

    return GraphedTrainStep(model, criterion, opt, accum_steps=accum_steps, use_amp=True, reducer=reducer, ema=ema)


@dataclass(frozen=True)
class EmaSettings:
    decay: float
    warmup: bool
    select: bool            # best epoch / early stopping / best weights follow the EMA model


def ema_settings() -> EmaSettings | None:
    """$EMA_DECAY (YAML training.ema_decay; absent or 0: off), $EMA_WARMUP (default on), $EMA_EVAL (default on)."""
    decay = env_float("EMA_DECAY", 0.0)
    if not decay:
        return None
    on = lambda name: env_str(name, "1").lower() not in {"0", "false", "no", "off"}     # noqa: E731
    return EmaSettings(decay=decay, warmup=on("EMA_WARMUP"), select=on("EMA_EVAL"))


def make_model_ema(model: nn.Module, build, device: str, settings: EmaSettings):
    """ema.ModelEma of `model` with a shadow from `build()` (the model's own registry builder) placed like the model."""
    from ..ema import ModelEma

    if not str(device).startswith("cuda"):
        raise RuntimeError("the weight EMA (training.ema_decay) runs on a HIP device only (no CPU fallback)")
    shadow = build()
    shadow.to(memory_format=torch.channels_last)
    shadow = shadow.to(device)
    return ModelEma(model, shadow, decay=settings.decay, warmup=settings.warmup)


def restore_model_ema(ema, state: dict | None) -> None:
    """On resume: the checkpoint's `model_ema` (+ `model_ema_updates`); without one EMA starts over as a copy of the model."""
    if ema is None or state is None:
        return
    if state.get("model_ema") is None:
        console.print("[bold yellow]⚠️  The checkpoint holds no model_ema[/]; the EMA starts over as a copy of the model")
        ema.reset()
        return
    ema.load_state_dict({"module": state["model_ema"], "updates": int(state.get("model_ema_updates", 0))})


def ema_checkpoint_extra(ema) -> dict:
    return {} if ema is None else {"model_ema": ema.module.state_dict(), "model_ema_updates": ema.updates}


@dataclass(frozen=True)
class ClipSettings:
    limit: float
    mode: str               # norm | value


def clip_settings() -> ClipSettings | None:
    """$CLIP_GRAD (YAML training.clip_grad, timm's --clip-grad; absent or 0: off) and $CLIP_MODE (training.clip_mode:
    norm | value, default norm).  A negative or non-finite limit and an unknown mode are a ValueError."""
    limit, mode = env_float("CLIP_GRAD", 0.0), env_str("CLIP_MODE", "norm").lower()
    if mode not in {"norm", "value"}:
        raise ValueError(f"training.clip_mode must be norm or value, got {mode!r}")
    if not math.isfinite(limit) or limit < 0.0:
        raise ValueError(f"training.clip_grad must be a finite number >= 0 (0: off), got {limit!r}")
    return ClipSettings(limit=limit, mode=mode) if limit else None


class TorchClipper:
    """Gradient clipping in front of torch's AdamW (device: cpu): torch.nn.utils.clip_grad_norm_ / clip_grad_value_ over the
    optimizer's parameters, with the record HipAdamW.clip_stats() keeps on the device.  Like HipAdamW it lets a step with a
    non-finite gradient norm pass without an update."""

    def __init__(self, opt: optim.Optimizer, settings: ClipSettings) -> None:
        self.params = [p for g in opt.param_groups for p in g["params"]]
        self.settings = settings
        self.norms: list[float] = []
        self.clipped = self.skipped = 0

    def clip(self) -> bool:
        """Clip the gradients in place; False when the step must be skipped."""
        if self.settings.mode == "norm":
            norm = float(torch.nn.utils.clip_grad_norm_(self.params, self.settings.limit))
        else:
            norm = float(torch.nn.utils.get_total_norm([p.grad for p in self.params if p.grad is not None]))
            torch.nn.utils.clip_grad_value_(self.params, self.settings.limit)
        if not math.isfinite(norm):
            self.skipped += 1
            return False
        self.norms.append(norm)
        self.clipped += self.settings.mode == "norm" and self.settings.limit / (norm + 1e-6) < 1.0
        return True

    def clip_stats(self, reset: bool = True) -> dict:
        n = len(self.norms)
        rec = {"grad_norm_last": self.norms[-1] if n else 0.0, "grad_norm_mean": sum(self.norms) / max(1, n),
               "grad_norm_max": max(self.norms, default=0.0), "steps": n + self.skipped, "clipped_steps": int(self.clipped),
               "skipped_steps": self.skipped}
        if reset:
            self.norms, self.clipped, self.skipped = [], 0, 0
        return rec


def clip_suffix(clip: dict | None) -> str:
    """` | grad_norm=<mean> (clipped k/n[, skipped s])` of an epoch's console line; empty without clipping."""
    if clip is None:
        return ""
    skipped = f", skipped {clip['skipped_steps']}" if clip["skipped_steps"] else ""
    return f" | grad_norm={clip['grad_norm_mean']:.4g} (clipped {clip['clipped_steps']}/{clip['steps']}{skipped})"


@dataclass(frozen=True)
class MixSettings:
    mixup_alpha: float
    cutmix_alpha: float
    prob: float
    switch_prob: float
    mode: str


def mix_settings() -> MixSettings | None:
    """$MIXUP_ALPHA, $CUTMIX_ALPHA (YAML training.mixup_alpha / cutmix_alpha; both absent or 0: off), $MIX_PROB (default 1),
    $MIX_SWITCH_PROB (default 0.5), $MIX_MODE (batch | pair | elem, default batch)."""
    mixup, cutmix = env_float("MIXUP_ALPHA", 0.0), env_float("CUTMIX_ALPHA", 0.0)
    if not mixup and not cutmix:
        return None
    return MixSettings(mixup_alpha=mixup, cutmix_alpha=cutmix, prob=env_float("MIX_PROB", 1.0),
                       switch_prob=env_float("MIX_SWITCH_PROB", 0.5), mode=env_str("MIX_MODE", "batch").lower())


def make_mixer(settings: MixSettings | None, num_classes: int, device: str):
    """mix.BatchMixer for the training batches of every phase (None when mixing is off); evaluation never mixes."""
    if settings is None:
        return None
    if not str(device).startswith("cuda"):
        raise RuntimeError("Mixup / CutMix (training.mixup_alpha, cutmix_alpha) run on a HIP device only (no CPU fallback)")
    from ..mix import BatchMixer

    return BatchMixer(mixup_alpha=settings.mixup_alpha, cutmix_alpha=settings.cutmix_alpha, prob=settings.prob,
                      switch_prob=settings.switch_prob, mode=settings.mode, num_classes=num_classes)


@dataclass(frozen=True)
class LossSettings:
    class_weights: tuple[float, ...] | str | None      # the weights, "balanced" until resolve_loss_settings() has the counts, or None
    focal_gamma: float

    def describe(self) -> str:
        w = "none" if self.class_weights is None else self.class_weights if isinstance(self.class_weights, str) \
            else "[" + ", ".join(f"{v:.4g}" for v in self.class_weights) + "]"
        return f"class_weights={w} | focal_gamma={self.focal_gamma:g}"


def loss_settings(num_classes: int) -> LossSettings | None:
    """$CLASS_WEIGHTS (YAML training.class_weights: `balanced`, or one weight per class — a YAML list, comma-separated in the
    environment) and $FOCAL_GAMMA (training.focal_gamma, a float >= 0; absent or 0: off).  Both absent: None, and the criterion is
    the plain one.  ValueError for a list that has not `num_classes` finite entries >= 0 and for a negative or non-finite gamma."""
    from ..optim import check_class_weight, check_focal_gamma

    raw = env_str("CLASS_WEIGHTS", "").strip()
    gamma = check_focal_gamma(env_float("FOCAL_GAMMA", 0.0))
    weights: tuple[float, ...] | str | None = None
    if raw.lower() == "balanced":
        weights = "balanced"
    elif raw and raw.lower() not in {"none", "0", "false", "off", "no"}:
        fields = [f.strip() for f in raw.strip("[]() ").split(",") if f.strip()]
        try:
            values = [float(f) for f in fields]
        except ValueError as exc:
            raise ValueError(f"training.class_weights must be `balanced` or a list of numbers, got {raw!r}") from exc
        if len(values) != num_classes:
            raise ValueError(f"training.class_weights has {len(values)} entries for {num_classes} classes: {raw!r}")
        weights = tuple(check_class_weight(values).double().tolist())
    return None if weights is None and not gamma else LossSettings(class_weights=weights, focal_gamma=gamma)


def balanced_class_weights(counts, names=None) -> tuple[float, ...]:
    """w_j = n / (J * n_j) from the pictures per class of the whole training split (scikit-learn's `balanced`); a class without
    a picture is a ValueError that names it."""
    counts = [int(c) for c in counts]
    empty = [str(names[j]) if names is not None and j < len(names) else str(j) for j, c in enumerate(counts) if c < 1]
    if empty or not counts:
        raise ValueError(f"training.class_weights: balanced needs a training picture of every class, none of: {', '.join(empty) or 'any class'}")
    n, J = sum(counts), len(counts)
    return tuple(n / (J * c) for c in counts)


def resolve_loss_settings(settings: LossSettings | None, targets, num_classes: int, names=None) -> LossSettings | None:
    """`balanced` made into numbers from the training dataset's `targets` — the whole split, not a rank's shard, so that every
    rank gets the same weights."""
    if settings is None or settings.class_weights != "balanced":
        return settings
    counts = torch.bincount(torch.as_tensor(list(targets), dtype=torch.int64), minlength=num_classes).tolist()
    return LossSettings(class_weights=balanced_class_weights(counts, names), focal_gamma=settings.focal_gamma)


def _load_pretrained(model: nn.Module, name: str) -> None:
    hint = env_str("PRETRAINED", "")
    if hint.lower() in ("0", "false", "no", "none"):
        return
    candidates = [Path(hint)] if hint else [Path("weights") / f"{name}.pth", Path("weights") / f"{name}_v0.3.0.pth"]
    for path in candidates:
        if path.is_file():
            state = torch.load(path, map_location="cpu")
            if isinstance(state, dict) and "state_dict" in state:
                state = state["state_dict"]
            elif isinstance(state, dict) and "model" in state:
                state = state["model"]
            own = model.state_dict()
            usable = {k: v for k, v in state.items() if k in own and v.shape == own[k].shape}   # head may differ in classes
            model.load_state_dict(usable, strict=False)
            console.print(f"[bold green]Loaded pretrained weights[/] {path} ({len(usable)}/{len(own)} tensors)")
            return
    console.print("[bold yellow]⚠️  No local pretrained weights[/] (set training.pretrained); starting from random init")


def _make_criterion_and_optimizer(use_cuda: bool, loss_cfg: LossSettings | None = None):
    """The TRAINING criterion (label smoothing 0.1; `loss_cfg`: resolved class weights and focal gamma) and the optimizer class."""
    weights = None if loss_cfg is None else loss_cfg.class_weights
    gamma = 0.0 if loss_cfg is None else loss_cfg.focal_gamma
    if isinstance(weights, str):
        raise ValueError("class_weights: balanced must be resolved from the training targets first (resolve_loss_settings)")
    if use_cuda:
        from ..optim import HipAdamW, HipCrossEntropyLoss

        if weights is None and not gamma:
            return HipCrossEntropyLoss(label_smoothing=0.1), HipAdamW
        return HipCrossEntropyLoss(label_smoothing=0.1, weight=weights, focal_gamma=gamma), HipAdamW
    # device: cpu — the reference's own torch path; only non-HIP (plug-in) modules can run there
    if gamma:
        raise RuntimeError("the focal loss (training.focal_gamma) runs on a HIP device only (no CPU fallback)")
    weight = None if weights is None else torch.tensor(weights, dtype=torch.float32)
    return nn.CrossEntropyLoss(weight=weight, label_smoothing=0.1), optim.AdamW


def _make_eval_criterion(use_cuda: bool) -> nn.Module:
    """What evaluate() reports as val_loss: always the plain label-smoothed cross entropy, whatever the training criterion is
    weighted by, so that validation losses compare between runs and with earlier checkpoints."""
    return _make_criterion_and_optimizer(use_cuda)[0]


def evaluate(model: nn.Module, dl: DataLoader, device: str, tail=None, criterion: nn.Module | None = None,
             val_auc: bool = False) -> EvalResult:
    """Top-1 accuracy and, with a `criterion`, the mean loss; f32, no autocast (efficientnet.py:237-262,
    efficientformer_v2.py:206-219, fastervit.py:224-240).  The counters stay on the device and are read once at the end
    (and summed over ranks in one collective).  val_auc: the softmax scores stay on the device as well, are gathered over the
    ranks (disjoint validation shards) and give the exact ROC-AUC and equal error rate; non-finite scores give nan, not an error."""
    model.eval()
    kept_probs, kept_targets = [], []
    correct = torch.zeros((), dtype=torch.float64, device=device)
    loss_sum = torch.zeros((), dtype=torch.float64, device=device) if criterion is not None else None
    total = 0
    with torch.inference_mode():
        # (large validation batches: the forward is GPU-bound and the in-stream copy would add ~40 % to it)
        fwd = eval_forward(model, device)
        for inputs, targets in device_batches(dl, device, tail, prefetch=(getattr(dl, "batch_size", 0) or 0) >= 128):
            logits = fwd(inputs)
            if criterion is not None:
                loss_sum += criterion(logits, targets).double() * targets.size(0)
            correct += (logits.argmax(1) == targets).sum()
            total += targets.numel()
            if val_auc:
                kept_probs.append(torch.softmax(logits.float(), dim=1))        # a new tensor: a graphed forward reuses `logits`
                kept_targets.append(targets.to(torch.int64))
    sums = [float(correct), float(total)] + ([float(loss_sum)] if criterion is not None else [])
    n_correct, n_total, *s_loss = all_reduce_counts(*sums, device=device)
    auc = eer = None
    if val_auc and kept_probs:
        from ..metrics import binary_roc, gather_scores, ovr_auc

        probs, truth = gather_scores(torch.cat(kept_probs), torch.cat(kept_targets))
        if probs.shape[1] == 2:
            roc = binary_roc(probs[:, 1], truth, strict=False)
            auc, eer = roc.auc, roc.eer
        else:
            auc = ovr_auc(probs, truth, probs.shape[1], strict=False)
    return EvalResult(acc=n_correct / max(1, n_total), total=int(n_total), correct=int(n_correct),
                      loss=s_loss[0] / max(1, n_total) if s_loss else None, auc=auc, eer=eer)


def train_one_epoch(model: nn.Module, dl: DataLoader, opt: optim.Optimizer, scaler, criterion: nn.Module, device: str, *,
                    use_cuda_amp: bool, progress: Progress, task: TaskID, accum_steps: int = 1, zero_grad_first: bool = False,
                    reducer: GradAllReducer | None = None, tail=None, label: str | None = None, stepper=None, ema=None,
                    mixer=None, with_loss: bool = False, clipper: TorchClipper | None = None) -> EpochResult:
    """One epoch (efficientnet.py:265-333; efficientformer_v2.py:222-257; fastervit.py:243-300).  `stepper`
    (graph_step.GraphedTrainStep) replays the captured loop body instead of dispatching it and updates its own `ema`;
    an eager optimizer step updates `ema` (ema.ModelEma) itself.  `mixer` (mix.BatchMixer) mixes every batch in place and
    turns its labels into probability rows before the step sees them.  `with_loss` sums the loss on the device (one more
    launch per micro-batch) for the mean training loss over all ranks.  `label`: progress text `<label> | loss` with the
    rate in the extra column instead of `train | loss | img/s`.  Gradient clipping is part of HipAdamW's step (so of the
    stepper's graph too); `clipper` clips for torch's AdamW right before its step.  Either way the epoch's norms and counts
    are read once, after the loop."""
    model.train()
    start = perf_counter()
    if not zero_grad_first:
        opt.zero_grad(set_to_none=True)
    loss_sum = torch.zeros((), dtype=torch.float64, device=device) if with_loss else None
    seen_total = pending = 0
    shown = float("nan")
    for i, (inputs, targets) in enumerate(device_batches(dl, device, tail, prefetch=stepper is not None), 1):
        if mixer is not None:
            inputs, targets = mixer(inputs, targets)        # outside of the captured step: one launch on this stream
        if stepper is not None:
            # zero_grad is part of the "first" body; `last` lets an eager micro-batch overlap the DP exchange with its backward
            loss = stepper.micro_batch(inputs, targets, first=pending == 0, last=pending + 1 == accum_steps)
            pending += 1
            if pending == accum_steps:
                stepper.optimizer_step()
                pending = 0
        else:
            if zero_grad_first:
                opt.zero_grad(set_to_none=True)
            with torch.autocast(device_type="cuda", dtype=torch.bfloat16, enabled=use_cuda_amp):
                loss = criterion(model(inputs), targets)
                if accum_steps > 1:
                    loss = loss / accum_steps
            if reducer is not None and pending + 1 == accum_steps:
                reducer.arm()                   # this backward completes the step: buckets leave as they fill
            scaler.scale(loss).backward()
            pending += 1
            if pending == accum_steps:
                if reducer is not None:
                    reducer.finish()
                if clipper is None or clipper.clip():
                    scaler.step(opt)
                scaler.update()
                if ema is not None:
                    ema.step()
                if not zero_grad_first:
                    opt.zero_grad(set_to_none=True)
                pending = 0
        bsz = targets.size(0)
        seen_total += bsz
        if with_loss:
            loss_sum += loss.detach().double() * (bsz * max(1, accum_steps))
        if i % LOG_EVERY == 0 or i == len(dl):
            shown = float(loss.detach()) * max(1, accum_steps)          # the only host sync of the loop
        seen = min(i * (dl.batch_size or bsz), len(dl.sampler) if dl.sampler is not None else len(dl.dataset))
        ips = seen / max(1e-6, perf_counter() - start)
        if label is not None:
            progress.update(task, advance=1, description=f"{label} | loss={shown:.4f}", extra=f"{ips:.0f} img/s")
        else:
            progress.update(task, advance=1, description=f"train | loss={shown:.4f} | {ips:.0f} img/s")
    if pending > 0:
        if stepper is not None:
            stepper.optimizer_step()
        else:
            if reducer is not None:
                reducer.finish()
            if clipper is None or clipper.clip():
                scaler.step(opt)
            scaler.update()
            if ema is not None:
                ema.step()
        opt.zero_grad(set_to_none=True)
    if str(device).startswith("cuda"):
        torch.cuda.synchronize()
    seconds = perf_counter() - start
    stats = {"images": seen_total, "seconds": seconds, "images_per_sec": seen_total / max(1e-9, seconds),
             "launch": "hipgraph" if (stepper is not None and stepper.replays > 0 and not stepper.failed) else "eager"}
    # gradient clipping: the record of this epoch's optimizer steps, one host read (every rank holds the same one)
    clip = clipper.clip_stats() if clipper is not None else opt.clip_stats() if hasattr(opt, "clip_stats") else None
    if clip is not None:
        stats.update({k: clip[k] for k in ("grad_norm_mean", "grad_norm_max", "clipped_steps", "skipped_steps")})
    if not with_loss:
        return EpochResult(stats, clip=clip)
    (total_loss,) = all_reduce_counts(float(loss_sum), device=device)
    (total_seen,) = all_reduce_counts(float(seen_total), device=device)
    return EpochResult(stats, total_loss / max(1.0, total_seen), clip=clip)


def log_throughput(env, chief: bool, world: int, **record) -> None:
    """One JSON line per phase in OUTPUT_DIR/logs/throughput.jsonl: the machine-readable twin of the progress bar's
    `img/s`."""
    if not chief:
        return
    path = Path(env.logs_dir) / "throughput.jsonl"
    path.parent.mkdir(parents=True, exist_ok=True)
    record = {"timestamp": time(), "n_gpus": world, **record}
    if "images_per_sec" in record:
        record["images_per_sec_all_ranks"] = record["images_per_sec"] * world
    with path.open("a", encoding="utf-8") as fh:
        fh.write(json.dumps(record) + "\n")


def run(spec: TrainerSpec) -> None:  # noqa: PLR0915
    global console
    console = create_console()
    env = prepare_training_environment(weights_name=spec.best_weights_name, best_checkpoint_name="best.ckpt",
                                       latest_checkpoint_name="latest.ckpt")
    apply_seed(env.seed)
    data_root = env_path("DATA_ROOT", DATA_ROOT)
    train_split, val_split = env_str("TRAIN_SPLIT", "Train"), env_str("VAL_SPLIT", "Validation")
    batch_size, epochs = env_int("BATCH_SIZE", spec.default_batch_size), env_int("EPOCHS", spec.default_epochs)
    img_size, num_workers = env_int("IMG_SIZE", spec.default_img_size), env_int("NUM_WORKERS", spec.default_num_workers)
    num_classes = env_int("NUM_CLASSES", 2)
    ft_lr, ft_wd = env_float("LR", spec.ft_lr), env_float("WEIGHT_DECAY", spec.ft_wd)
    patience = env_int("EARLY_STOP_PATIENCE", spec.default_patience)
    ft_batch, accum = spec.ft_batch_size, spec.ft_accum_steps if spec.ft_batch_size is not None else 1
    if spec.ft_from_env:
        ft_batch, accum = env_int("FT_BATCH_SIZE", ft_batch), env_int("ACCUM_STEPS", accum)
    # the reference's trainers ignore the YAML's model name; this one honours MODEL_NAME when the
    # orchestrator exports it, so the registry's prefix entries (faster_vit_0_224, efficientformerv2_s0, ...) train too
    model_name = env_str("MODEL_NAME", spec.model_name)

    use_cuda = torch.cuda.is_available()
    device = "cuda" if use_cuda else "cpu"
    if env.device_override:
        if env.device_override.startswith("cuda") and not torch.cuda.is_available():
            console.print("[bold yellow]⚠️  Requested CUDA device not available[/]; falling back to CPU")
            device, use_cuda = "cpu", False
        else:
            device, use_cuda = env.device_override, env.device_override.startswith("cuda")
    rank, local_rank, world = init_distributed() if use_cuda else (0, 0, 1)
    if use_cuda and world > 1:
        device = f"cuda:{local_rank}"
    chief = rank == 0
    torch.backends.cudnn.benchmark = use_cuda and env.seed is None

    if not (data_root / train_split).exists() or not (data_root / val_split).exists():
        console.print(f"[bold red]Dataset not found under[/] {data_root}")
        console.print(f"Expected: {data_root}/{train_split}/<class> and {data_root}/{val_split}/<class>")
        raise SystemExit(1)
    jpeg_settings()         # likewise a bad training.jpeg_p / jpeg_quality_min / jpeg_quality_max
    blur_settings()         # and a bad training.blur_p / blur_sigma_min / blur_sigma_max
    policy_settings()       # a bad training.rand_augment_* / trivial_augment is a ValueError here, not a class-count message below
    clip_cfg = clip_settings()      # and so is a bad training.clip_grad / clip_mode
    metric_cfg = metric_settings()  # and a bad training.select_metric
    loss_cfg = loss_settings(num_classes)   # and a bad training.class_weights / focal_gamma
    if metric_cfg.val_auc and not use_cuda:
        console.print("[bold yellow]training.val_auc / select_metric: auc ignored[/]: the AUC kernels need a CUDA device; accuracy is followed")
        metric_cfg = MetricSettings(val_auc=False, select="acc")
    val_auc, metric = metric_cfg.val_auc, metric_cfg.select
    try:
        # $GPU_INPUT_TAIL (YAML training.gpu_input_tail): loaders ship uint8 batches, the device does
        # flip / to-float / normalise / erasing
        gpu_tail = use_cuda and (env_str("GPU_INPUT_TAIL", "0").lower() in {"1", "true", "yes"}
                                 or env_str("GPU_RESIZE", "0").lower() in {"1", "true", "yes"})     # device resize implies the device tail
        train_dl, val_dl, *tails = get_loaders(data_root, train_split, val_split, img_size, batch_size, num_workers,
                                               expected_classes=num_classes, rank=rank, world=world, seed=env.seed or 0,
                                               gpu_tail=gpu_tail, transform_kwargs=spec.transform_kwargs)
        train_tail, val_tail = tails if tails else (None, None)
    except ValueError as exc:
        console.print("[bold red]Class configuration mismatch[/]", f"→ {exc}")
        console.print("Update `data.num_classes` in your YAML to match the dataset. For MNIST, set it to 10.")
        raise SystemExit(1) from exc
    console.print(f"[bold]Data[/]: train={len(train_dl.dataset)} | val={len(val_dl.dataset)} | bs={batch_size} | "
                  f"steps/epoch={len(train_dl)}" + (f" | ranks={world}" if world > 1 else ""))

    builder = get_model_spec(model_name).builder
    build = lambda: builder(model_name, num_classes, img_size) if spec.pass_img_size else builder(model_name, num_classes)  # noqa: E731
    model = build()
    _load_pretrained(model, model_name)
    model.to(memory_format=torch.channels_last)
    model = model.to(device)
    broadcast_module_state(model)
    # class weights / focal loss ($CLASS_WEIGHTS, $FOCAL_GAMMA) shape the training criterion only: val_loss stays the plain loss
    loss_cfg = resolve_loss_settings(loss_cfg, getattr(train_dl.dataset, "targets", ()), num_classes,
                                     getattr(train_dl.dataset, "classes", None))
    if loss_cfg is None:
        criterion, make_opt = _make_criterion_and_optimizer(use_cuda)
        eval_criterion = criterion if spec.report_loss else None
    else:
        criterion, make_opt = _make_criterion_and_optimizer(use_cuda, loss_cfg)
        criterion = criterion.to(device)
        eval_criterion = _make_eval_criterion(use_cuda) if spec.report_loss else None
        console.print(f"[bold]Loss[/]: {loss_cfg.describe()} (training only; val_loss is the unweighted loss)")
    if balanced_sampling():
        console.print("[bold]Sampling[/]: class-balanced epochs (training.balanced_sampling), drawn with replacement")
    mixer = make_mixer(mix_settings(), num_classes, device)      # Mixup / CutMix ($MIXUP_ALPHA, $CUTMIX_ALPHA)
    scaler = torch.amp.GradScaler(enabled=False)        # bf16 needs no loss scaling; calls kept for parity
    opt_extra = {"grad_scale": 1.0 / world} if use_cuda else {}
    if use_cuda and clip_cfg is not None:       # HipAdamW clips inside its step; torch's AdamW (device: cpu) gets a TorchClipper
        opt_extra.update(max_grad_norm=clip_cfg.limit, clip_mode=clip_cfg.mode)
    make_clipper = lambda o: TorchClipper(o, clip_cfg) if clip_cfg is not None and not use_cuda else None    # noqa: E731

    progress = Progress(TextColumn("[bold blue]{task.description}"), BarColumn(bar_width=None), MofNCompleteColumn(),
                        TimeElapsedColumn(), TimeRemainingColumn(), TextColumn("{task.fields[extra]}"), console=console,
                        transient=False, disable=not chief)
    best_val_acc, best_epoch, epochs_no_improve = -1.0, -1, 0
    warmup_done = env.resume_checkpoint is not None

    with progress:
        if not warmup_done:
            for name, p in model.named_parameters():
                p.requires_grad = any(key in name for key in spec.warmup_keys)
            head = [p for p in model.parameters() if p.requires_grad]
            warm_opt = make_opt(head, lr=spec.head_lr, weight_decay=spec.head_wd, **opt_extra)
            reducer = GradAllReducer(head, arena=getattr(warm_opt, "arena", None)) if world > 1 else None
            if reducer is not None:
                reducer.attach()
            task = progress.add_task(spec.warmup_task, total=len(train_dl), extra="")
            console.print("[bold]Warmup (head only)[/]")
            # the reference's inline warm-up loops (efficientformer_v2.py:362-382 / fastervit.py:408-428) are
            # train_one_epoch with zero_grad first, no accumulation and the rate in the `extra` column
            done = train_one_epoch(model, train_dl, warm_opt, scaler, criterion, device, use_cuda_amp=use_cuda, progress=progress,
                                   task=task, accum_steps=1, zero_grad_first=spec.warmup_zero_grad_first, reducer=reducer,
                                   tail=train_tail, label=spec.warmup_label, mixer=mixer, with_loss=spec.report_loss,
                                   clipper=make_clipper(warm_opt),
                                   stepper=make_stepper(model, criterion, warm_opt, accum_steps=1, use_cuda=use_cuda, world=world,
                                                        reducer=reducer))
            log_throughput(env, chief, world, phase="warmup", epoch=0, model=model_name, batch_size=batch_size, **done.stats)
            if reducer is not None:
                reducer.detach()
            res = evaluate(model, val_dl, device, val_tail, eval_criterion, val_auc=val_auc)
            value = selection_value(res, metric)
            best_val_acc, best_epoch, warmup_done = best_val_acc if value is None else value, 0, True
            console.print("[bold cyan]warmup[/] | " + spec.warmup_line.format(res=res) + clip_suffix(done.clip) + auc_suffix(res))
            if getattr(warm_opt, "arena", None) is not None:
                warm_opt.zero_grad()
                warm_opt.arena.release()

        for name, p in model.named_parameters():
            p.requires_grad = spec.unfreeze_keys is None or any(key in name for key in spec.unfreeze_keys)
        ft_dl = train_dl
        if ft_batch is not None:
            console.print(f"[bold]Fine-tune[/]: bs={ft_batch}, accum_steps={accum} (effective ≈ {ft_batch * accum * world})")
            ft_dl = make_loader(train_dl.dataset, ft_batch, num_workers, shuffle=True, rank=rank, world=world, seed=env.seed or 0)
        trainable = [p for p in model.parameters() if p.requires_grad]
        opt = make_opt(trainable, lr=ft_lr, weight_decay=ft_wd, **opt_extra)
        reducer = GradAllReducer(trainable, arena=getattr(opt, "arena", None)) if world > 1 else None
        if reducer is not None:
            reducer.attach()
        scheduler = optim.lr_scheduler.CosineAnnealingLR(opt, T_max=max(1, epochs - 1))
        # weight EMA ($EMA_DECAY): starts here as a copy of the warmed-up model, or from the checkpoint's model_ema
        ema_cfg = ema_settings()
        ema = None if ema_cfg is None else make_model_ema(model, build, device, ema_cfg)
        stepper = make_stepper(model, criterion, opt, accum_steps=accum, use_cuda=use_cuda, world=world, reducer=reducer, ema=ema)
        clipper = make_clipper(opt)
        start_epoch = 0
        resume_state = maybe_load_checkpoint(env, model=model, optimizer=opt, scheduler=scheduler)
        restore_model_ema(ema, resume_state)
        if resume_state is not None:
            start_epoch = int(resume_state.get("epoch", 0))
            best_val_acc = float(resume_state.get("best_val_acc", best_val_acc))
            best_epoch = int(resume_state.get("best_epoch", best_epoch))
            warmup_done = bool(resume_state.get("warmup_done", warmup_done))
            epochs_no_improve = max(0, start_epoch - best_epoch)
            saved_metric = str(resume_state.get("select_metric", "acc"))
            if saved_metric != metric:
                console.print(f"[bold yellow]Resume[/]: the checkpoint's best value follows {saved_metric}, this run follows {metric}; "
                              "the best value starts over")
                best_val_acc, epochs_no_improve = -1.0, 0
            console.print(f"[bold green]Resumed[/] from epoch {start_epoch} using {env.resume_checkpoint}")

        for epoch in range(start_epoch + 1, epochs + 1):
            if hasattr(ft_dl.sampler, "set_epoch"):
                ft_dl.sampler.set_epoch(epoch)
            task = progress.add_task(f"epoch {epoch}", total=len(ft_dl), extra="")
            done = train_one_epoch(model, ft_dl, opt, scaler, criterion, device, use_cuda_amp=use_cuda, progress=progress, task=task,
                                   accum_steps=accum, zero_grad_first=spec.zero_grad_first, reducer=reducer, tail=train_tail,
                                   stepper=stepper, ema=ema, mixer=mixer, with_loss=spec.report_loss, clipper=clipper)
            log_throughput(env, chief, world, phase="fine-tune", epoch=epoch, model=model_name,
                           batch_size=ft_dl.batch_size, accum_steps=accum, **done.stats)
            scheduler.step()
            res = evaluate(model, val_dl, device, val_tail, eval_criterion, val_auc=val_auc)
            console.print(f"[bold cyan]epoch {epoch}[/] | "
                          + spec.epoch_line.format(res=res, train_loss=done.loss, lr=scheduler.get_last_lr()[0])
                          + clip_suffix(done.clip) + auc_suffix(res))
            acc = selection_value(res, metric)
            if ema is not None:
                res_ema = evaluate(ema.module, val_dl, device, val_tail, eval_criterion, val_auc=val_auc)
                console.print(f"[bold cyan]epoch {epoch} EMA[/] | " + spec.ema_line.format(res=res_ema) + f" | updates={ema.updates}"
                              + auc_suffix(res_ema))
                if ema_cfg.select:
                    acc = selection_value(res_ema, metric)
            improved = improves(acc, best_val_acc)
            if improved:
                best_val_acc, best_epoch, epochs_no_improve = acc, epoch, 0
            else:
                epochs_no_improve += 1
            if chief:
                state = save_latest_checkpoint(env, model=model, optimizer=opt, scheduler=scheduler, epoch=epoch,
                                               best_val_acc=best_val_acc, best_epoch=best_epoch,
                                               extra={"warmup_done": warmup_done, **ema_checkpoint_extra(ema),
                                                      **({"select_metric": metric} if metric != "acc" else {})})
                if improved:
                    save_best_checkpoint(env, state, weights_key="model_ema" if ema is not None and ema_cfg.select else "model")
                    console.print(f"[bold green]new best[/] val_{metric}={best_val_acc:.4f} (epoch {best_epoch}) → saved "
                                  f"{env.best_weights_path.name}")
            if spec.early_stop and not improved and epochs_no_improve >= patience:
                console.print(f"[bold yellow]Early stopping[/]: no improvement for {patience} epoch(s). "
                              f"Best at epoch {best_epoch} with val_{metric}={best_val_acc:.4f}.")
                break

    console.print(f"[bold green]Best weights saved →[/] {env.best_weights_path.resolve()}")
    console.print(f"[bold green]Best checkpoint saved →[/] {env.best_checkpoint_path.resolve()}")
