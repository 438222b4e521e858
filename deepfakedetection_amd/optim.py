"""Loss and optimizer objects of the hot loop, backed by libdfd_hip.so.

`HipCrossEntropyLoss` replaces `nn.CrossEntropyLoss(label_smoothing=0.1)`
(trainers/efficientnet.py:412); `HipAdamW` replaces `optim.AdamW(params, lr, weight_decay)`
(trainers/efficientnet.py:440,487-491) with ONE fused multi-tensor kernel per step and
keeps torch.optim.AdamW's state layout (`step`, `exp_avg`, `exp_avg_sq`) so the
checkpoints written by train_env.save_latest_checkpoint stay interchangeable.
"""

from __future__ import annotations

import math

import torch
from torch import nn

from . import kernels as K
from ._lib import (
    ADAMW_HP_LEN, CLIP_CFG_LEN, CLIP_CLIPPED, CLIP_MODE_NORM, CLIP_MODE_VALUE, CLIP_NORM, CLIP_NORM_MAX, CLIP_NORM_SUM, CLIP_SKIPPED,
    CLIP_STATE_LEN, CLIP_STEPS,
)
from .arena import GradArena
from .functions import CrossEntropyFunction, WeightedCrossEntropyFunction

_CHUNK = 4096          # elements per workgroup of the fused kernel (~1000 workgroups for EfficientNet-B0)
_CLIP_MODES = {"norm": CLIP_MODE_NORM, "value": CLIP_MODE_VALUE}


def check_clip(limit, mode: str) -> tuple[float | None, str]:
    """(limit or None, mode) of a gradient-clipping request; ValueError for a limit <= 0, a non-finite limit or an unknown mode."""
    if mode not in _CLIP_MODES:
        raise ValueError(f"clip_mode must be one of {sorted(_CLIP_MODES)}, got {mode!r}")
    if limit is None:
        return None, mode
    limit = float(limit)
    if not math.isfinite(limit) or limit <= 0.0:
        raise ValueError(f"max_grad_norm must be a finite number > 0 (or None for no clipping), got {limit!r}")
    return limit, mode


def check_class_weight(weight) -> torch.Tensor | None:
    """f32 [J] on the CPU from a sequence or tensor of class weights (None stays None); ValueError unless it is a non-empty vector
    of finite numbers >= 0."""
    if weight is None:
        return None
    try:
        w = torch.as_tensor(weight, dtype=torch.float64).detach().cpu()
    except (TypeError, ValueError, RuntimeError) as exc:
        raise ValueError(f"class weights must be a sequence of numbers, got {weight!r}") from exc
    if w.dim() != 1 or w.numel() < 1:
        raise ValueError(f"class weights must be a vector with one entry per class, got shape {tuple(w.shape)}")
    if not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
        raise ValueError(f"class weights must be finite and >= 0, got {w.tolist()}")
    return w.float()


def check_focal_gamma(gamma) -> float:
    gamma = float(gamma)
    if not math.isfinite(gamma) or gamma < 0.0:
        raise ValueError(f"focal_gamma must be a finite number >= 0 (0: off), got {gamma!r}")
    return gamma


class HipCrossEntropyLoss(nn.Module):
    """nn.CrossEntropyLoss(label_smoothing=, weight=) on the device, plus the focal factor (1 - p)^focal_gamma of Lin et al. 2017
    on every term.  `weight` is kept as an f32 buffer (it follows .to(device), and a captured step reads it at a fixed address:
    `criterion.weight.copy_(new)` reaches the next replay).  Without weights and with focal_gamma 0 the module launches exactly
    dfd_ce_loss / dfd_ce_loss_soft; otherwise dfd_ce_loss_w.  The mean is torch's: over sum_n weight[t_n] for class indices, over
    N for probability targets."""

    def __init__(self, label_smoothing: float = 0.0, weight=None, focal_gamma: float = 0.0) -> None:
        super().__init__()
        self.label_smoothing = float(label_smoothing)
        self.focal_gamma = check_focal_gamma(focal_gamma)
        self.register_buffer("weight", check_class_weight(weight))

    def extra_repr(self) -> str:
        w = None if self.weight is None else [round(v, 4) for v in self.weight.tolist()]
        return f"label_smoothing={self.label_smoothing}, weight={w}, focal_gamma={self.focal_gamma}"

    def forward(self, logits: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
        if not logits.is_cuda:
            raise RuntimeError("HipCrossEntropyLoss needs logits on a HIP device (no CPU fallback)")
        # like nn.CrossEntropyLoss: integer targets are class indices [N], floating targets are class probabilities [N, J]
        if targets.is_floating_point() and targets.shape != logits.shape:
            raise ValueError(f"probability targets must have the logits' shape {tuple(logits.shape)}, got {tuple(targets.shape)}")
        if self.weight is None and self.focal_gamma == 0.0:
            return CrossEntropyFunction.apply(logits.float(), targets, self.label_smoothing)
        weight = self.weight
        if weight is not None:
            if weight.numel() != logits.shape[-1]:
                raise ValueError(f"{weight.numel()} class weights for logits of {logits.shape[-1]} classes")
            if weight.device != logits.device:          # a criterion nobody moved: once, at its first use (never inside a capture,
                self.weight = weight = weight.to(logits.device)     # whose first sight of a batch shape runs eagerly)
        if not targets.is_floating_point() and targets.dtype != torch.int64:
            targets = targets.long()
        return WeightedCrossEntropyFunction.apply(logits.float(), targets, self.label_smoothing, self.focal_gamma, weight)


class HipAdamW(torch.optim.Optimizer):
    """AdamW (decoupled weight decay, bias correction) as one kernel launch per group.

    `max_grad_norm` turns gradient clipping on (None: off, and then the launches are exactly the ones above).  With
    `clip_mode="norm"` the gradients of ALL groups are scaled by min(1, limit / (norm + 1e-6)), norm being their global L2 norm
    after `grad_scale`: torch.nn.utils.clip_grad_norm_'s formula, in f32, from an f64 sum of squares.  With "value" every
    gradient element is clamped to [-limit, limit] (clip_grad_value_).  A step then is dfd_grad_sumsq per group, one
    dfd_grad_clip_finish and dfd_adamw_step_clip per group, all capturable; the limit and the mode live in device memory and
    are uploaded by prepare_step(), so set_clip() takes effect at the next replay of a captured step.

    Unlike torch, a step whose norm is not finite (an inf or NaN gradient, in either mode) is SKIPPED: parameters and moments
    stay as they are, which is what a GradScaler does for an overflowed step (clip_grad_norm_ would multiply by 0 or NaN).  The
    host-side step counter still advances on a skipped step, so the bias corrections are one step ahead afterwards.
    clip_stats() reports the norms and how many steps were clipped and skipped."""

    def __init__(self, params, lr: float = 1e-3, betas: tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, grad_scale: float = 1.0, use_arena: bool = True,
                 max_grad_norm: float | None = None, clip_mode: str = "norm") -> None:
        limit, clip_mode = check_clip(max_grad_norm, clip_mode)
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, grad_scale=grad_scale)
        super().__init__(params, defaults)
        self._clip_limit, self._clip_mode = limit, clip_mode
        self._clip_buffers: tuple[torch.Tensor, torch.Tensor, torch.Tensor] | None = None
        if limit is not None:
            self._check_clip_groups()
            self._alloc_clip()
        self._tables: dict[int, K.AddressTable] = {}
        self._hp: dict[int, torch.Tensor] = {}
        self._shared_step: dict[int, torch.Tensor] = {}
        # gradients of the trainable parameters live at fixed addresses (see arena.py): the
        # pointer table below is then built once and the backward kernels write in place
        self.arena: GradArena | None = None
        trainable = [p for g in self.param_groups for p in g["params"] if p.requires_grad and p.is_cuda]
        if use_arena and trainable:
            self.arena = GradArena(trainable)

    def _check_clip_groups(self) -> None:
        scales = {float(g["grad_scale"]) for g in self.param_groups}
        if len(scales) > 1:
            raise ValueError(f"gradient clipping needs one grad_scale for all param groups (one global norm), got {sorted(scales)}")

    def _alloc_clip(self) -> None:
        """partials (one f64 per chunk of every parameter), cfg and the state record: allocated here, never under capture."""
        if self._clip_buffers is not None:
            return
        params = [p for g in self.param_groups for p in g["params"]]
        device = next((p.device for p in params if p.is_cuda), None)
        if device is None:
            return                              # nothing to step on a HIP device: step() raises like without clipping
        nchunks = sum((p.numel() + _CHUNK - 1) // _CHUNK for p in params)
        self._clip_buffers = (torch.zeros(max(1, nchunks), dtype=torch.float64, device=device),
                              torch.zeros(CLIP_CFG_LEN, dtype=torch.float32, device=device),
                              torch.zeros(CLIP_STATE_LEN, dtype=torch.float32, device=device))

    def set_clip(self, limit: float | None, mode: str | None = None) -> None:
        """Change the clipping limit (None: off) and, if given, the mode.  A captured step keeps its launches: switching
        clipping on or off needs a new capture, a new limit or mode reaches the replay through prepare_step()."""
        limit, mode = check_clip(limit, self._clip_mode if mode is None else mode)
        if limit is not None:
            self._check_clip_groups()
        self._clip_limit, self._clip_mode = limit, mode
        if limit is not None:
            self._alloc_clip()

    @property
    def clip_state(self) -> torch.Tensor | None:
        """The device record dfd_grad_clip_finish keeps (f32, CLIP_STATE_LEN; see include/dfd_hip.h), None without clipping."""
        return None if self._clip_buffers is None else self._clip_buffers[2]

    def clip_stats(self, reset: bool = True) -> dict | None:
        """Norms and counts since the last reset, read with ONE host sync: {grad_norm_last, grad_norm_mean, grad_norm_max,
        steps, clipped_steps, skipped_steps}; mean and max are over the steps with a finite norm.  None without clipping."""
        if self._clip_limit is None or self._clip_buffers is None:
            return None
        state = self._clip_buffers[2]
        rec = state.tolist()
        if reset:
            state.zero_()
        steps, skipped = int(rec[CLIP_STEPS]), int(rec[CLIP_SKIPPED])
        return {"grad_norm_last": rec[CLIP_NORM], "grad_norm_mean": rec[CLIP_NORM_SUM] / max(1, steps - skipped),
                "grad_norm_max": rec[CLIP_NORM_MAX], "steps": steps, "clipped_steps": int(rec[CLIP_CLIPPED]),
                "skipped_steps": skipped}

    def state_dict(self):
        """torch.optim.AdamW's format: every parameter gets its OWN `step` tensor.  Internally all parameters of a
        group share one counter object (see prepare_step); pickling that aliasing would make torch.optim.AdamW advance
        the shared counter once per parameter after loading the checkpoint (train_env.save_latest_checkpoint stores this
        dict as is, reference train_env.py:254-278)."""
        sd = super().state_dict()
        sd["state"] = {k: {n: (v.clone() if n == "step" and isinstance(v, torch.Tensor) else v) for n, v in st.items()}
                       for k, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict) -> None:
        super().load_state_dict(state_dict)
        self._shared_step.clear()                  # the loaded per-parameter counters are re-shared at the next step

    def zero_grad(self, set_to_none: bool = True) -> None:
        """Drop the gradients (always set-to-none: an arena slot must not be both the
        destination of a backward kernel and the accumulator autograd adds into)."""
        super().zero_grad(set_to_none=True)
        if self.arena is not None:
            self.arena.reset()

    def _table(self, gi: int, entries: list[tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]]) -> K.AddressTable:
        flat = [t for e in entries for t in e]
        cached = self._tables.get(gi)
        if cached is not None and cached.valid_for(flat):
            return cached
        rows = []
        for p, g, m, v in entries:
            base = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr())
            for off in range(0, p.numel(), _CHUNK):
                rows.append([b + 4 * off for b in base] + [min(_CHUNK, p.numel() - off)])
        table = self._tables[gi] = K.AddressTable(flat)
        table.upload(rows, entries[0][0].device, cached)
        return table

    def _ensure_state(self, p: torch.Tensor) -> dict:
        st = self.state[p]
        if not st:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    @torch.no_grad()
    def prepare_step(self) -> None:
        """Advance the step counters and upload this step's hyper-parameters
        {lr, betas, eps, wd, bias corrections, grad_scale} to device memory.

        `step()` does this itself in eager mode.  When the whole training step is a
        captured hipGraph, call prepare_step() before every replay: the kernel reads the
        values from memory, so the replayed launch sees the new learning rate / step."""
        for gi, group in enumerate(self.param_groups):
            # one step counter per group: every trainable parameter's state["step"] is the SAME CPU tensor, advanced by
            # one in-place add per optimizer step (per-parameter counters were 2 x len(params) host-side tensor ops per
            # step).  After load_state_dict the entries are separate tensors again: they are re-shared here.
            shared, device = self._shared_step.get(gi), None
            for p in group["params"]:
                if not p.requires_grad:
                    continue
                st = self._ensure_state(p)
                if shared is None:
                    shared = self._shared_step[gi] = st["step"] if isinstance(st["step"], torch.Tensor) else torch.tensor(float(st["step"]))
                if st["step"] is not shared:
                    st["step"] = shared
                device = p.device
            if device is None:
                continue
            shared += 1
            step_no = float(shared)
            b1, b2 = group["betas"]
            hp_vals = [group["lr"], b1, b2, group["eps"], group["weight_decay"], 1.0 - b1 ** step_no,
                       1.0 - b2 ** step_no, group["grad_scale"]]
            assert len(hp_vals) == ADAMW_HP_LEN
            dev = self._hp.get(gi)
            if dev is None:
                dev = torch.empty(ADAMW_HP_LEN, dtype=torch.float32, device=device)
                self._hp[gi] = dev
            dev.copy_(torch.tensor(hp_vals, dtype=torch.float32))   # pageable source: host-synchronous staging
        if self._clip_limit is not None and self._clip_buffers is not None:
            self._clip_buffers[1].copy_(torch.tensor([self._clip_limit, float(_CLIP_MODES[self._clip_mode])], dtype=torch.float32))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        capturing = torch.cuda.is_current_stream_capturing()
        if not capturing:
            self.prepare_step()
        work = []
        for gi, group in enumerate(self.param_groups):
            entries = []
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.dtype != torch.float32 or not p.is_cuda or not p.is_contiguous():
                    raise RuntimeError("HipAdamW needs contiguous f32 parameters on a HIP device (no CPU fallback)")
                st = self._ensure_state(p)
                g = p.grad
                if g.dtype != torch.float32 or not g.is_contiguous():
                    g = g.float().contiguous()
                entries.append((p, g, st["exp_avg"], st["exp_avg_sq"]))
            if not entries:
                continue
            if gi not in self._hp:
                raise RuntimeError("HipAdamW.step() under stream capture needs prepare_step() before the capture")
            if self._clip_limit is None:
                K.adamw_step(self._table(gi, entries), self._hp[gi])
            else:
                work.append((self._table(gi, entries), self._hp[gi]))
        if work:
            # one global norm over all groups: sum of squares per group into its slice of the partials, one finish, then the steps
            if self._clip_buffers is None:
                raise RuntimeError("HipAdamW clipping buffers are missing: the parameters were not on a HIP device at set_clip()")
            partials, cfg, state = self._clip_buffers
            off = 0
            for table, _ in work:
                K.grad_sumsq(table, partials[off:off + table.dev.shape[0]])
                off += table.dev.shape[0]
            K.grad_clip_finish(partials[:off], work[0][1], cfg, state)
            for table, hp in work:
                K.adamw_step_clip(table, hp, cfg, state)
        return loss


__all__ = ["HipAdamW", "HipCrossEntropyLoss"]
