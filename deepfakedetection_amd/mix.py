"""Mixup and CutMix of a training batch on the device: one dfd_mix_batch launch per batch (timm data/mixup.py, `Mixup`).

`BatchMixer(mixup_alpha, cutmix_alpha, prob, switch_prob, mode, num_classes)` takes timm's parameters.  There is no
`label_smoothing` argument: smoothing stays in the criterion (HipCrossEntropyLoss), which gives the same targets because
both steps are linear.  `cutmix_minmax` is not provided.

The partner of sample i is always N - 1 - i (timm's `x.flip(0)`).  One DECISION is drawn per batch, per pair (i, N - 1 - i)
or per sample, by `mode`:

    mix with probability `prob`; if both alphas are positive choose cutmix with probability `switch_prob`;
    lam ~ Beta(alpha, alpha) of the chosen kind; otherwise lam = 1 (keep)
    cutmix: a box from lam and a uniform centre (cutmix_box), then lam is corrected to the box's true share

Every draw comes from the host torch generator, so `apply_seed` reproduces a run.  The decisions become a job table, int32
[N, 8] rows {mode, w0, w1, y0, y1, x0, x1, 0} with w0 = float32(lam) and w1 = float32(1 - lam) (subtracted in float64) as
bit patterns; the kernel mixes the pictures in place and writes the targets f32 [N, num_classes]:
zeros, y[i][labels[i]] = w0, then y[i][labels[N-1-i]] += w1.  The middle sample of an odd batch is its own partner and is kept.

`mixer(x, labels)` always returns dense targets, also for a batch that drew `keep`, so that the key of a captured training
step (graph_step.GraphedTrainStep: x shape, dtype, y shape) does not flip between batches.  It runs OUTSIDE the captured
graph, before `stepper.micro_batch`.
"""

from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

from . import kernels as K
from ._lib import MIX_CUTMIX, MIX_JOB_WORDS, MIX_KEEP, MIX_MIXUP

MODES = ("batch", "pair", "elem")


def cutmix_box(lam: float, cy: int, cx: int, H: int, W: int) -> tuple[int, int, int, int, float]:
    """timm's rand_bbox + the lam correction: rows [y0, y1), columns [x0, x1) of the box around the centre (cy, cx) whose
    sides are sqrt(1 - lam) of the picture's, cut at the borders, and the share of the picture that stays."""
    r = math.sqrt(1.0 - lam)
    cut_h, cut_w = int(H * r), int(W * r)
    clip = lambda v, hi: max(0, min(hi, v))     # noqa: E731
    y0, y1 = clip(cy - cut_h // 2, H), clip(cy + cut_h // 2, H)
    x0, x1 = clip(cx - cut_w // 2, W), clip(cx + cut_w // 2, W)
    return y0, y1, x0, x1, 1.0 - (y1 - y0) * (x1 - x0) / float(H * W)


@dataclass(frozen=True)
class Decision:
    mode: int = MIX_KEEP
    lam: float = 1.0
    box: tuple[int, int, int, int] = (0, 0, 0, 0)        # y0, y1, x0, x1


KEEP = Decision()


def _rand() -> float:
    return float(torch.rand(1).item())


def _beta(alpha: float) -> float:
    """Beta(alpha, alpha) from two Gamma(alpha, 1) draws of the host generator."""
    g = torch._standard_gamma(torch.full((2,), float(alpha), dtype=torch.float64))
    total = float(g.sum())
    return float(g[0]) / total if total > 0.0 else 0.5


def job_row(d: Decision) -> list[int]:
    """One row of the table: {mode, bits of float32(lam), bits of float32(1 - lam), y0, y1, x0, x1, 0}."""
    w = np.array([d.lam, 1.0 - d.lam], dtype=np.float64).astype(np.float32).view(np.int32)
    return [d.mode, int(w[0]), int(w[1]), *d.box, 0]


def job_table(decisions: list[Decision]) -> torch.Tensor:
    """Host int32 [N, MIX_JOB_WORDS] table of one decision per sample."""
    table = torch.tensor([job_row(d) for d in decisions], dtype=torch.int32).reshape(len(decisions), MIX_JOB_WORDS)
    return table


class BatchMixer:
    """Mixup / CutMix with timm's `Mixup` parameters; see the module docstring."""

    def __init__(self, mixup_alpha: float = 1.0, cutmix_alpha: float = 0.0, prob: float = 1.0, switch_prob: float = 0.5,
                 mode: str = "batch", num_classes: int = 2) -> None:
        if mixup_alpha < 0.0 or cutmix_alpha < 0.0 or not (mixup_alpha > 0.0 or cutmix_alpha > 0.0):
            raise ValueError(f"BatchMixer needs a positive mixup_alpha or cutmix_alpha, got {mixup_alpha} and {cutmix_alpha}")
        if not 0.0 <= prob <= 1.0 or not 0.0 <= switch_prob <= 1.0:
            raise ValueError(f"prob and switch_prob must lie in [0, 1], got {prob} and {switch_prob}")
        if mode not in MODES:
            raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
        if num_classes < 1:
            raise ValueError(f"num_classes must be positive, got {num_classes}")
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.prob, self.switch_prob = float(prob), float(switch_prob)
        self.mode, self.num_classes = mode, int(num_classes)

    def decide(self, H: int, W: int) -> Decision:
        """One decision from the host generator."""
        if not _rand() < self.prob:
            return KEEP
        if self.mixup_alpha > 0.0 and self.cutmix_alpha > 0.0:
            cut = _rand() < self.switch_prob
        else:
            cut = self.cutmix_alpha > 0.0
        lam = _beta(self.cutmix_alpha if cut else self.mixup_alpha)
        if lam == 1.0:
            return KEEP
        if not cut:
            return Decision(MIX_MIXUP, lam)
        cy = int(torch.randint(0, H, (1,)).item())
        cx = int(torch.randint(0, W, (1,)).item())
        y0, y1, x0, x1, lam = cutmix_box(lam, cy, cx, H, W)
        if lam == 1.0:                          # empty box
            return KEEP
        return Decision(MIX_CUTMIX, lam, (y0, y1, x0, x1))

    def sample(self, N: int, H: int, W: int) -> torch.Tensor:
        """The job table of one batch of N pictures H x W: host int32 [N, MIX_JOB_WORDS]."""
        jobs = [KEEP] * N
        if self.mode == "batch":
            d = self.decide(H, W)
            jobs = [d] * N
        elif self.mode == "pair":
            for i in range(N // 2):
                jobs[i] = jobs[N - 1 - i] = self.decide(H, W)
        else:
            jobs = [self.decide(H, W) if 2 * i + 1 != N else KEEP for i in range(N)]
        if N % 2 == 1:
            jobs[N // 2] = KEEP                 # its own partner
        return job_table(jobs)

    @torch.no_grad()
    def __call__(self, x: torch.Tensor, labels: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        """Mixes the f32 batch `x` [N, 3, H, W] in place on the current stream; returns (x, soft targets f32 [N, num_classes])."""
        if not x.is_cuda:
            raise RuntimeError("BatchMixer needs the batch on a HIP device (no CPU fallback)")
        N, _, H, W = x.shape
        jobs = self.sample(N, H, W).pin_memory()
        return x, K.mix_batch(x, labels, jobs, self.num_classes)


__all__ = ["BatchMixer", "Decision", "KEEP", "MODES", "cutmix_box", "job_row", "job_table"]
