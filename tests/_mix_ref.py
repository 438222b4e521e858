"""CPU restatement of Mixup / CutMix in plain numpy / torch: what dfd_mix_batch and mix.BatchMixer must compute.

The pictures: the partner of sample i is N - 1 - i; every job reads the batch as it was BEFORE the call.
    keep    picture untouched, y[i] = onehot(labels[i])
    mixup   x[i] = fl(fl(x_i * w0) + fl(x_j * w1)) in float32 (numpy never fuses a multiply into an add)
    cutmix  x[i][:, y0:y1, x0:x1] = x_j[:, y0:y1, x0:x1]
    targets of both mixing modes: zeros, y[i][labels[i]] = w0, then y[i][labels[j]] += w1
with w0 = float32(lam), w1 = float32(1 - lam), the subtraction done in float64.

The box (timm's rand_bbox and its lam correction) is restated with numpy's own operations, independently of mix.cutmix_box.
"""

from __future__ import annotations

import numpy as np
import torch

KEEP, MIXUP, CUTMIX = 0, 1, 2
_F32 = np.float32


def weights(lam: float) -> tuple[np.float32, np.float32]:
    return _F32(np.float64(lam)), _F32(np.float64(1.0) - np.float64(lam))


def ref_box(lam: float, cy: int, cx: int, H: int, W: int):
    """(y0, y1, x0, x1, corrected lam)."""
    ratio = np.sqrt(1 - lam)
    cut_h, cut_w = int(H * ratio), int(W * ratio)
    yl, yh = np.clip(cy - cut_h // 2, 0, H), np.clip(cy + cut_h // 2, 0, H)
    xl, xh = np.clip(cx - cut_w // 2, 0, W), np.clip(cx + cut_w // 2, 0, W)
    area = (yh - yl) * (xh - xl)
    return int(yl), int(yh), int(xl), int(xh), float(1.0 - area / float(H * W))


def job(mode: int, lam: float = 1.0, box=(0, 0, 0, 0)) -> list[int]:
    """One row of the int32 job table: {mode, bits(w0), bits(w1), y0, y1, x0, x1, 0}."""
    w0, w1 = weights(lam)
    return [mode, int(np.array(w0).view(np.int32)), int(np.array(w1).view(np.int32)), *[int(v) for v in box], 0]


def table(jobs: list[list[int]]) -> torch.Tensor:
    return torch.tensor(jobs, dtype=torch.int32).reshape(len(jobs), 8)


def ref_mix(x: torch.Tensor, labels: torch.Tensor, jobs: torch.Tensor, num_classes: int):
    """x: f32 [N, 3, H, W] (any memory format; read logically), labels int64 [N], jobs int32 [N, 8] -> (mixed x as a
    contiguous NCHW tensor, targets f32 [N, num_classes])."""
    src = x.detach().cpu().contiguous().numpy().astype(_F32, copy=True)
    out = src.copy()
    lab = labels.detach().cpu().numpy()
    tab = jobs.detach().cpu().numpy().astype(np.int32)
    N = src.shape[0]
    y = np.zeros((N, num_classes), dtype=_F32)
    for i in range(N):
        j = N - 1 - i
        mode = int(tab[i, 0])
        w0, w1 = tab[i, 1:3].copy().view(_F32)
        y0, y1, x0, x1 = (int(v) for v in tab[i, 3:7])
        if mode == KEEP or i == j:
            y[i, lab[i]] = _F32(1.0)
            continue
        if mode == MIXUP:
            a = (src[i] * w0).astype(_F32)
            b = (src[j] * w1).astype(_F32)
            out[i] = (a + b).astype(_F32)
        else:
            out[i, :, y0:y1, x0:x1] = src[j, :, y0:y1, x0:x1]
        y[i, lab[i]] = w0
        y[i, lab[j]] = _F32(y[i, lab[j]] + w1)
    return torch.from_numpy(out), torch.from_numpy(y)
