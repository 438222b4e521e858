"""The float64 reference of the class-weighted and focal cross entropy (dfd_ce_loss_w, ABI 147): include/dfd_hip.h's formulas in
torch on the CPU, with autograd for the gradient, and the closed-form gradient written out beside it.

  q[n][j] = (1 - eps) * (j == t[n]) + eps / J          (index targets)     or     t[n][j] * (1 - eps) + eps / J
  row[n]  = -sum_j w[j] q[n][j] (1 - p[n][j])^gamma logp[n][j]             ((1 - p)^0 = 1, also at p = 1)
  loss    = sum_n row[n] / D,    D = sum_n w[t[n]] (index targets) or N (probability targets);   NaN at D = 0, as in torch

Terms whose q is 0 are masked with torch.where, not multiplied: the reference stays finite beside a -inf logit, in the value and in
the gradient (the masked branch is fed a harmless stand-in, so autograd never forms 0 * inf either)."""

from __future__ import annotations

import torch


def smoothed_targets(targets: torch.Tensor, J: int, eps: float) -> torch.Tensor:
    """q, float64 [N, J]."""
    if targets.is_floating_point():
        return targets.double() * (1.0 - eps) + eps / J
    q = torch.full((targets.numel(), J), eps / J, dtype=torch.float64)
    q[torch.arange(targets.numel()), targets] += 1.0 - eps
    return q


def denominator(targets: torch.Tensor, w: torch.Tensor, N: int) -> torch.Tensor:
    if targets.is_floating_point():
        return torch.tensor(float(N), dtype=torch.float64)
    return w.double()[targets].sum()


def _parts(logits: torch.Tensor, q: torch.Tensor):
    """(p, logp, live): softmax, log-softmax with the dead classes (q == 0) replaced by 0 before anything multiplies them."""
    live = q != 0
    logp = torch.log_softmax(logits, 1)
    return torch.where(live, logp.exp(), torch.zeros_like(logp)), torch.where(live, logp, torch.zeros_like(logp)), live


def rows(logits: torch.Tensor, targets: torch.Tensor, w: torch.Tensor | None, eps: float, gamma: float) -> torch.Tensor:
    """row[n], float64 [N]; `logits` is float64 [N, J] (it may require a gradient)."""
    N, J = logits.shape
    w = torch.ones(J, dtype=torch.float64) if w is None else w.double()
    q = smoothed_targets(targets, J, eps)
    p, logp, live = _parts(logits, q)
    if gamma == 0:
        m = torch.ones_like(p)
    else:
        omp = (1.0 - p).clamp_min(0.0)
        safe = torch.where(omp > 0, omp, torch.ones_like(omp))          # 0^gamma = 0 without a 0 * inf in its derivative
        m = torch.where(omp > 0, safe ** gamma, torch.zeros_like(omp))
    return -torch.where(live, w[None, :] * q * m * logp, torch.zeros_like(logp)).sum(1)


def loss(logits: torch.Tensor, targets: torch.Tensor, w: torch.Tensor | None, eps: float, gamma: float) -> torch.Tensor:
    N, J = logits.shape
    ww = torch.ones(J, dtype=torch.float64) if w is None else w.double()
    D = denominator(targets, ww, N)
    if float(D) == 0.0:                     # torch: the weighted mean of the target terms is 0 / 0, whatever label smoothing adds
        return torch.full((), float("nan"), dtype=torch.float64) + 0.0 * logits.sum()
    return rows(logits, targets, w, eps, gamma).sum() / D


def loss_and_grad(logits: torch.Tensor, targets: torch.Tensor, w: torch.Tensor | None, eps: float, gamma: float):
    """(loss, d loss / d logits) in float64 from logits of any float dtype, by autograd."""
    l64 = logits.detach().double().requires_grad_(True)
    out = loss(l64, targets, w, eps, gamma)
    (grad,) = torch.autograd.grad(out, l64)
    return out.detach(), grad


def closed_form_grad(logits: torch.Tensor, targets: torch.Tensor, w: torch.Tensor | None, eps: float, gamma: float) -> torch.Tensor:
    """(g - p * G) / D with g = w q (gamma (1 - p)^(gamma - 1) p logp - (1 - p)^gamma), the bracket 0 at p = 1 when gamma > 0."""
    logits = logits.detach().double()
    N, J = logits.shape
    ww = torch.ones(J, dtype=torch.float64) if w is None else w.double()
    q = smoothed_targets(targets, J, eps)
    p_all = torch.softmax(logits, 1)
    p, logp, live = _parts(logits, q)
    if gamma == 0:
        bracket = -torch.ones_like(p)
    else:
        omp = (1.0 - p).clamp_min(0.0)
        safe = torch.where(omp > 0, omp, torch.ones_like(omp))
        bracket = torch.where(omp > 0, gamma * safe ** (gamma - 1.0) * p * logp - safe ** gamma, torch.zeros_like(omp))
    g = torch.where(live, ww[None, :] * q * bracket, torch.zeros_like(p))
    return (g - p_all * g.sum(1, keepdim=True)) / denominator(targets, ww, N)
