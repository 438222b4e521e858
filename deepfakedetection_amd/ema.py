"""Exponential moving average (EMA) of the weights: one dfd_ema_update launch per optimizer step.

`ModelEma(model, shadow)` keeps `shadow` — a second instance of the same architecture (built by the same registry
builder, on the same device and memory format) — as an exponential moving average of `model`:

    d_k = min(decay, (1 + k) / (10 + k))     with warm-up (TF ExponentialMovingAverage's num_updates rule)
    d_k = decay                              without
    shadow <- shadow + (1 - d_k) * (model - shadow)          for the k-th update, k = 1, 2, ...

over every floating entry of the state dict (trainable and frozen parameters, BatchNorm running statistics); integer
buffers (`num_batches_tracked`) are copied.  The shadow is never a `copy.deepcopy` of a live HIP module: its
__dict__ holds derived-weight caches and graph objects that carry raw addresses of the original.

The whole update is ONE multi-tensor kernel over a chunk table of int64 rows {src, dst, count, kind}, built once and
uploaded through pinned memory (rebuilt only when an address changes).  The weight 1 - d_k lives in device memory:
`prepare()` advances k and uploads it, `update()` launches — so `update()` can be captured in the training step's
hipGraph next to HipAdamW (graph_step.GraphedTrainStep) and every replay sees that step's weight.  `step()` is both, for
the eager loop.
"""

from __future__ import annotations

import torch
from torch import nn

from . import kernels as K
from ._lib import EMA_COPY, EMA_LERP, EMA_TABLE_COLS

_CHUNK = 4096          # elements (kind 0) or 8-byte words (kind 1) per workgroup


def decay_at(k: int, decay: float, warmup: bool = True) -> float:
    """d_k of the k-th update (k >= 1)."""
    return min(decay, (1.0 + k) / (10.0 + k)) if warmup else decay


def weight_at(k: int, decay: float, warmup: bool = True) -> float:
    """w_k = float32(1 - d_k), computed in float64: the value the kernel reads."""
    return float(torch.tensor(1.0 - decay_at(k, decay, warmup), dtype=torch.float64).float())


def _dense(t: torch.Tensor) -> bool:
    return t.is_contiguous() or (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last))


class ModelEma:
    """EMA of `model`'s state dict kept in `shadow` (which is then `.module`)."""

    def __init__(self, model: nn.Module, shadow: nn.Module, decay: float = 0.9999, warmup: bool = True) -> None:
        if not 0.0 < decay < 1.0:
            raise ValueError(f"EMA decay must lie in (0, 1), got {decay}")
        if model is shadow:
            raise ValueError("the EMA shadow must be a separate module instance")
        self.decay, self.warmup = float(decay), bool(warmup)
        self.model, self.module = model, shadow
        self.updates = 0
        shadow.load_state_dict(model.state_dict())      # in place: the shadow's tensors keep their addresses
        shadow.requires_grad_(False)
        shadow.eval()
        src, dst = model.state_dict(keep_vars=True), shadow.state_dict(keep_vars=True)
        if list(src) != list(dst):
            raise ValueError("model and EMA shadow have different state-dict keys")
        self._pairs: list[tuple[torch.Tensor, torch.Tensor, int]] = []
        for name, s in src.items():
            d = dst[name]
            if s.shape != d.shape or s.dtype != d.dtype:
                raise ValueError(f"EMA: {name}: model {tuple(s.shape)} {s.dtype} vs shadow {tuple(d.shape)} {d.dtype}")
            if not (s.is_cuda and d.is_cuda and s.device == d.device):
                raise RuntimeError(f"EMA: {name}: model and shadow must live on the same HIP device (no CPU fallback)")
            if s.stride() != d.stride() or not _dense(s):
                raise RuntimeError(f"EMA: {name}: model and shadow need the same dense memory layout")
            if s.numel() == 0:
                continue
            if s.dtype == torch.float32:
                kind = EMA_LERP
            elif not s.dtype.is_floating_point and not s.dtype.is_complex and s.numel() * s.element_size() % 8 == 0:
                kind = EMA_COPY
            else:
                raise RuntimeError(f"EMA: {name}: no kernel for {s.dtype} tensors of {s.numel()} elements")
            self._pairs.append((s.detach(), d.detach(), kind))
        self.device = self._pairs[0][0].device if self._pairs else None
        self._w = torch.zeros(1, dtype=torch.float32, device=self.device) if self._pairs else None
        self._cached: K.AddressTable | None = None
        self._table()                               # built outside any capture: a capture cannot allocate it

    def _table(self) -> K.AddressTable:
        flat = [t for s, d, _ in self._pairs for t in (s, d)]      # what the table points at
        cached = self._cached
        if cached is not None and cached.valid_for(flat):
            return cached
        rows = []
        for s, d, kind in self._pairs:
            n, esz = (s.numel(), 4) if kind == EMA_LERP else (s.numel() * s.element_size() // 8, 8)
            for off in range(0, n, _CHUNK):
                rows.append([s.data_ptr() + esz * off, d.data_ptr() + esz * off, min(_CHUNK, n - off), kind])
        assert len(rows[0]) == EMA_TABLE_COLS
        if (cached is None or len(rows) != cached.dev.shape[0]) and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ModelEma: the table grew under stream capture; rebuild the captured step")
        table = self._cached = K.AddressTable(flat)
        table.upload(rows, self.device, cached)
        return table

    def decay_at(self, k: int) -> float:
        return decay_at(k, self.decay, self.warmup)

    @torch.no_grad()
    def prepare(self) -> None:
        """Advance the update counter and upload this update's weight w_k to device memory (before every replay)."""
        self.updates += 1
        if self._w is not None:
            # pageable source: host-synchronous staging, like HipAdamW.prepare_step()
            self._w.copy_(torch.tensor([weight_at(self.updates, self.decay, self.warmup)], dtype=torch.float32))

    @torch.no_grad()
    def update(self) -> None:
        """One dfd_ema_update launch on the current stream with the weight prepare() uploaded (capturable)."""
        if not self._pairs:
            return
        if self.updates == 0:
            raise RuntimeError("ModelEma.update() needs prepare() first")
        K.ema_update(self._table(), self._w)

    def step(self) -> None:
        """prepare() + update(): one EMA update after an eager optimizer step."""
        self.prepare()
        self.update()

    @torch.no_grad()
    def reset(self) -> None:
        """Start over as a copy of the model (update count 0)."""
        self.module.load_state_dict(self.model.state_dict())
        self.updates = 0

    def state_dict(self) -> dict:
        return {"module": self.module.state_dict(), "updates": self.updates}

    @torch.no_grad()
    def load_state_dict(self, state: dict) -> None:
        self.module.load_state_dict(state["module"])        # copies in place: the table stays valid
        self.updates = int(state["updates"])


__all__ = ["ModelEma", "decay_at", "weight_at"]
