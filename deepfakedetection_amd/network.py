"""What the three HIP networks share around a forward pass: where parameters live, the Philox state, the NHWC input, the
derived-weight caches and the eval-mode BatchNorm batch.  The arithmetic is in the family's own module and functions."""

from __future__ import annotations

import warnings

import torch
from torch import nn

from .functions import BNRef, bn_eval_batch


def _bnref(bn: nn.BatchNorm2d) -> BNRef:
    return BNRef(bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.momentum, bn.eps)


def compute_dtype(device_type: str = "cuda") -> torch.dtype:
    """bf16 inside an autocast region, f32 outside."""
    try:
        enabled = torch.is_autocast_enabled(device_type)
    except TypeError:  # older signature
        enabled = torch.is_autocast_enabled()
    if not enabled:
        return torch.float32
    amp = torch.get_autocast_dtype(device_type) if hasattr(torch, "get_autocast_dtype") else torch.get_autocast_gpu_dtype()
    if amp != torch.bfloat16:
        warnings.warn("dfd HIP engine computes autocast regions in bf16 (fp16 autocast requested)", stacklevel=3)
    return torch.bfloat16


class HipNetwork(nn.Module):
    """Base of HipEfficientNet, HipEfficientFormerV2 and HipFasterViT."""

    def to(self, *args, **kwargs):
        """`.to(memory_format=torch.channels_last)` (trainers/efficientnet.py:409, trainers/efficientformer_v2.py:328) is
        accepted and ignored for the PARAMETERS: the kernels read weights in torch's default [O][I][kh][kw]
        layout, while activations are NHWC inside the engine whatever the input's strides."""
        kwargs.pop("memory_format", None)
        args = tuple(a for a in args if not isinstance(a, torch.memory_format))
        return super().to(*args, **kwargs) if (args or kwargs) else self

    def rng(self, device: torch.device):
        """This network's Philox state on `device` (created on first use, seeded from torch.initial_seed())."""
        from . import kernels as K

        cur = self.__dict__.get("_rng_obj")
        if cur is None or cur.state.device != device:
            cur = self.__dict__["_rng_obj"] = K.DeviceRng(device)
        return cur

    def nhwc_input(self, x: torch.Tensor) -> torch.Tensor:
        """float[N,3,H,W] of any memory format -> the f32 [N,H,W,3] view the first kernel reads."""
        if not x.is_cuda:
            raise RuntimeError(f"{type(self).__name__} runs on a HIP device only (no CPU fallback); move the input with .to('cuda')")
        return x.detach().float().contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)

    def _derived(self, dt: torch.dtype, sources: list[torch.Tensor], build, mx: bool = False) -> list:
        """The `.out` table of this network's kernels.DerivedWeights (mx: kernels.MxWeights) of `sources` in dtype `dt`,
        refreshed by its ONE batched launch.  build() makes the entry; it is made again only when a source moved (e.g. after
        .to())."""
        # one cache entry PER DTYPE (key dt, or ("mx", dt)): the trainer alternates bf16 training and f32 evaluation, and a
        # captured hipGraph holds raw pointers into its entry, so an entry is never freed by a train/eval switch; the
        # buffers are ordinary (non-inference) tensors even when first built under torch.inference_mode()
        key = ("mx", dt) if mx else dt
        caches = self.__dict__.setdefault("_derived_caches", {})
        cache = caches.get(key)
        if cache is None or not cache.valid_for(sources, dt):
            with torch.inference_mode(False):
                cache = caches[key] = build()
        cache.refresh()
        return cache.out

    def pass_scope(self):
        """Every forward() runs inside: eval-mode BatchNorm coefficient blocks (and FasterViT's identity statistics) are
        recorded on the first pass per (mode, dtype) and come from one batched launch from the second pass on."""
        return bn_eval_batch(self.__dict__, (self.training, compute_dtype()))

    def end_pass(self, counters: list, device: torch.device) -> None:
        if self.training:
            self.rng(device).tick(counters)         # one launch: every counter += 1, Philox offset += 1


__all__ = ["HipNetwork", "compute_dtype"]
