"""Per-tensor comparison of a bf16 gradient against the f32 oracle's, for the network-level bf16 tests.

A global gradient cosine is dominated by the few largest tensors: a wrong gradient for one small tensor does not move it.
These helpers judge every tensor on its own scale, restricted to the tensors whose gradient carries signal:
  * its largest entry is at least 1e-4 of the network's largest gradient entry, and
  * it is not structurally zero: a bias whose oracle gradient is below 2e-3 of its sibling weight's (a conv bias in front of a
    training-mode BatchNorm, a bias shifting every key of a softmax row) holds float cancellation noise on both sides.
"""

from __future__ import annotations

import torch


def signal_names(ref_grads: dict[str, torch.Tensor]) -> list[str]:
    top = max(float(g.abs().max()) for g in ref_grads.values())
    out = []
    for name, g in ref_grads.items():
        m = float(g.abs().max())
        if m < 1e-4 * top:
            continue
        sib = name[:-4] + "weight" if name.endswith("bias") else None
        if sib in ref_grads and m < 2e-3 * float(ref_grads[sib].abs().max()):
            continue
        out.append(name)
    return out


def rel_l2(got: torch.Tensor, want: torch.Tensor) -> float:
    """||got - want|| / ||want|| in float64."""
    got, want = got.detach().double().cpu().flatten(), want.detach().double().cpu().flatten()
    return float((got - want).norm() / want.norm().clamp_min(1e-300))


def report(errs: dict[str, float], yard: dict[str, float] | None = None, top: int = 12) -> str:
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:top]
    rows = [f"  {e:.4f}" + (f" (yardstick {yard[n]:.4f})" if yard else "") + f"  {n}" for n, e in worst]
    return f"{len(errs)} tensors with signal, worst relative L2 gradient errors:\n" + "\n".join(rows)
