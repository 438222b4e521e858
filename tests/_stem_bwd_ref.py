"""float64 reference of the stem's backward, factored as a one-pass kernel would (the map applied to the pixel sums):

    dW[co][k] = gamma[co] rstd[co] (A[co][k] - m1[co] S[k] - m2[co] B[co][k])
    A = sum dz patch    B = sum yh patch    S = sum patch    m1 = sum dz / M    m2 = sum dz yh / M    yh = (y - mean) rstd

Shared by tests/test_stem_bwd_algebra_cpu.py (against autograd) and tests/test_stem_bwd_fused_gpu.py (against the kernels)."""

from __future__ import annotations

import torch
import torch.nn.functional as F


def patches(x_nhwc: torch.Tensor, Ho: int, Wo: int, pad_top: int, pad_left: int, k: int = 3, stride: int = 2) -> torch.Tensor:
    """[N*Ho*Wo, 3*k*k] input patches in torch's (ci, kh, kw) order; zeros outside the image (leading pads as given)."""
    x = x_nhwc.permute(0, 3, 1, 2)
    N, _, H, W = x.shape
    bottom = max((Ho - 1) * stride + k - (H + pad_top), 0)
    right = max((Wo - 1) * stride + k - (W + pad_left), 0)
    xp = F.pad(x, (pad_left, right, pad_top, bottom))
    cols = F.unfold(xp, k, stride=stride)                       # [N, 3*k*k, L]
    hh = (xp.shape[2] - k) // stride + 1
    ww = (xp.shape[3] - k) // stride + 1
    cols = cols.reshape(N, 3 * k * k, hh, ww)[:, :, :Ho, :Wo]
    return cols.permute(0, 2, 3, 1).reshape(N * Ho * Wo, 3 * k * k)


def stem_bwd_formula(g: torch.Tensor, y: torch.Tensor, x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float,
                     pad_top: int, pad_left: int):
    """g, y: [N,Ho,Wo,C]; x: [N,H,W,3]; all float64.  BatchNorm in training mode + SiLU.
    Returns dict(dw [C,3,3,3], dgamma, dbeta, s1 = sum dz, s2 = sum dz yh, mean, rstd)."""
    N, Ho, Wo, C = y.shape
    M = N * Ho * Wo
    yf, gf = y.reshape(M, C), g.reshape(M, C)
    mean = yf.mean(0)
    var = ((yf - mean) ** 2).mean(0)
    rstd = 1.0 / torch.sqrt(var + eps)
    yh = (yf - mean) * rstd
    z = gamma * yh + beta
    sg = torch.sigmoid(z)
    dz = gf * sg * (1.0 + z * (1.0 - sg))
    s1, s2 = dz.sum(0), (dz * yh).sum(0)
    P = patches(x, Ho, Wo, pad_top, pad_left)
    A, B, S = dz.t() @ P, yh.t() @ P, P.sum(0)
    dw = (gamma * rstd)[:, None] * (A - (s1 / M)[:, None] * S[None, :] - (s2 / M)[:, None] * B)
    return {"dw": dw.reshape(C, 3, 3, 3), "dgamma": s2, "dbeta": s1, "s1": s1, "s2": s2, "mean": mean, "rstd": rstd}
