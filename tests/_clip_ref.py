"""Gradient clipping restated in numpy, for test_clip_cpu.py (pinned to torch there) and test_clip_gpu.py.

The norm is the exactly rounded one (squares and sum in f64 through math.fsum, one rounding to f32); the coefficient is
torch.nn.utils.clip_grad_norm_'s `max_norm / (norm + 1e-6)` clamped to 1, every operation rounded to f32."""

from __future__ import annotations

import itertools
import math

import numpy as np

_F32 = np.float32


def exact_sumsq(grads) -> float:
    """sum g^2 over all arrays of `grads`, exactly rounded to f64 (the square of an f32 is exact in f64)."""
    return math.fsum(itertools.chain.from_iterable(np.asarray(g, dtype=np.float64).ravel() ** 2 for g in grads))


def total_norm(grads, grad_scale: float = 1.0) -> np.float32:
    """float32(sqrt(sum g^2)) * float32(grad_scale), each rounded to f32."""
    return _F32(_F32(math.sqrt(exact_sumsq(grads))) * _F32(grad_scale))


def coef(norm, limit: float) -> np.float32:
    """min(limit / (norm + 1e-6), 1) with f32 roundings after the addition and after the division."""
    denom = _F32(_F32(norm) + _F32(1e-6))
    with np.errstate(divide="ignore", invalid="ignore"):
        c = _F32(_F32(limit) / denom)
    return _F32(1.0) if np.isnan(c) else min(c, _F32(1.0))         # fminf(NaN, 1) = 1


def scale(grads, c) -> list[np.ndarray]:
    """Norm mode: every gradient times the f32 coefficient, one rounding."""
    return [(np.asarray(g, dtype=_F32) * _F32(c)).astype(_F32) for g in grads]


def clamp(grads, limit: float) -> list[np.ndarray]:
    """Value mode: every element clamped to [-limit, limit] (the limit rounded to f32)."""
    return [np.clip(np.asarray(g, dtype=_F32), -_F32(limit), _F32(limit)) for g in grads]


def within_one_ulp(got, want) -> bool:
    got, want = _F32(got), _F32(want)
    return bool(abs(np.float64(got) - np.float64(want)) <= np.float64(np.spacing(want)))
