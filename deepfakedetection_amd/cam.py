"""Grad-CAM heatmaps and overlays for a whole batch on the device (reference web_ui.py:241-305).

The reference runs one `pytorch_grad_cam.GradCAM` per model on a single image and draws the overlay with
`show_cam_on_image` in host numpy.  Here the same arithmetic runs for a batch:

    forward (f32, eval) with a hook on the target layer   hooks.py: the three families' unfused `_hooked_*` paths
    backward of sum_n logits[n, target_n]                 ClassifierOutputTarget
    map   max(0, sum_c mean_hw(grad) * act)               dfd_gradcam_map   (csrc/dfd_cam.hip)
    heatmap + overlay                                     dfd_cam_render    (cv2 INTER_LINEAR resize, min-max scaling, blend)

    with GradCam(model) as cam:
        result = cam(images, overlay=True)      # result.heatmap f32 [N, H, W], result.overlay uint8 [N, H, W, 3]

`python -m deepfakedetection_amd.cam --config config/inference_mi355x.yaml --out DIR IMG...` writes what web_ui.py exports
without Gradio: one labelled panel per `selection` model, side by side, as a PNG per image.
"""

from __future__ import annotations

import argparse
import functools
from dataclasses import dataclass
from pathlib import Path
from typing import Any, Sequence

import numpy as np
import torch
from torch import nn

from . import kernels as K

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
CLASS_LABELS = {0: "fake", 1: "real"}                 # web_ui.py CLASS_LABELS


@functools.lru_cache(maxsize=1)
def default_lut() -> np.ndarray:
    """The colour map, RGB uint8 [256, 3]: matplotlib's `jet` sampled at 256 points and rounded to uint8.  Close to cv2's
    COLORMAP_JET (what show_cam_on_image uses) but not verified equal to it: cv2 is not a dependency of this package."""
    from matplotlib import colormaps

    rgba = colormaps["jet"].resampled(256)(np.arange(256))
    lut = np.round(rgba[:, :3] * 255.0).astype(np.uint8)
    lut.flags.writeable = False
    return lut


def resolve_target(model: nn.Module) -> nn.Module:
    """web_ui._resolve_cam_target: `_conv_head` if the model has one, else the last nn.Conv2d of model.modules()."""
    head = getattr(model, "_conv_head", None)
    if isinstance(head, nn.Module):
        return head
    last = None
    for m in model.modules():
        if isinstance(m, nn.Conv2d):
            last = m
    if last is None:
        raise RuntimeError("No Conv2d layer found for Grad-CAM target.")
    return last


@dataclass
class CamResult:
    logits: torch.Tensor                 # f32 [N, classes]
    probs: torch.Tensor                  # softmax, f32 [N, classes]
    preds: torch.Tensor                  # arg-max, int64 [N]
    heatmap: torch.Tensor                # f32 [N, H, W] in [0, 1]
    overlay: torch.Tensor | None = None  # uint8 [N, H, W, 3] (RGB), when asked for


class GradCam:
    """pytorch_grad_cam.GradCAM(model, target_layers=[target]) for a batch, on the HIP kernels.

    Inside the `with` block a forward hook sits on the target layer, which switches the model's owner of that layer to its
    unfused, differentiable eval path (hooks.py); on exit the hook is removed and the fused path is back.  `images` is a
    normalised f32 NCHW batch on the device or a `data.collate_raw` batch (resized and normalised on the device, as
    orchestrator.class_probabilities does); it is processed `batch_size` images at a time.  No CPU fallback."""

    def __init__(self, model: nn.Module, target_layer: nn.Module | None = None, mean: Sequence[float] = IMAGENET_MEAN,
                 std: Sequence[float] = IMAGENET_STD, batch_size: int = 32, lut: np.ndarray | None = None,
                 image_weight: float = 0.5) -> None:
        self.model = model
        self.target = target_layer if target_layer is not None else resolve_target(model)
        self.mean, self.std = [float(v) for v in mean], [float(v) for v in std]
        self.batch_size = max(1, int(batch_size))
        self.lut = np.asarray(default_lut() if lut is None else lut, dtype=np.uint8)
        if self.lut.shape != (256, 3):
            raise ValueError(f"lut must be uint8 [256, 3], got {self.lut.shape}")
        self.image_weight = float(image_weight)
        self._handle = None
        self._act: torch.Tensor | None = None
        self._grad: torch.Tensor | None = None

    def __enter__(self) -> GradCam:
        self._handle = self.target.register_forward_hook(self._keep_activation)
        return self

    def __exit__(self, *exc: Any) -> None:
        if self._handle is not None:
            self._handle.remove()
            self._handle = None
        self._act = self._grad = None

    def _keep_activation(self, module: nn.Module, inputs: Any, output: torch.Tensor) -> None:
        if not output.requires_grad:
            return
        self._act = output
        output.register_hook(self._keep_gradient)

    def _keep_gradient(self, grad: torch.Tensor) -> None:
        self._grad = grad

    def __call__(self, images, targets: torch.Tensor | Sequence[int] | None = None, overlay: bool = False) -> CamResult:
        if self._handle is None:
            raise RuntimeError("GradCam is a context manager: use `with GradCam(model) as cam: cam(images)`")
        if self.model.training:
            raise RuntimeError("GradCam needs the model in eval mode (the hooked paths exist in eval only)")
        device = next(self.model.parameters()).device
        if device.type != "cuda":
            raise RuntimeError("GradCam runs on the HIP device only (no CPU fallback)")
        if isinstance(images, (tuple, list)):          # data.collate_raw batch: resize / crop / normalise on the device
            from .orchestration.orchestrator import _GPU_EVAL_TAIL

            with torch.no_grad():
                images = _GPU_EVAL_TAIL(images, device)
        if not isinstance(images, torch.Tensor) or not images.is_cuda:
            raise RuntimeError("GradCam needs the input batch on the HIP device (no CPU fallback)")
        if images.dim() != 4 or images.shape[1] != 3 or images.dtype != torch.float32:
            raise ValueError(f"expected a normalised f32 [N, 3, H, W] batch, got {tuple(images.shape)} {images.dtype}")
        if targets is not None:
            targets = torch.as_tensor(targets, dtype=torch.int64).to(device).flatten()
            if targets.numel() != images.shape[0]:
                raise ValueError(f"{targets.numel()} targets for {images.shape[0]} images")
        mean_std = torch.tensor(self.mean + self.std, dtype=torch.float32, device=device)
        lut = torch.from_numpy(self.lut.copy()).to(device) if overlay else None
        parts = [self._chunk(images[i:i + self.batch_size], None if targets is None else targets[i:i + self.batch_size],
                             mean_std, lut) for i in range(0, images.shape[0], self.batch_size)]
        return CamResult(*(torch.cat([p[k] for p in parts]) for k in range(4)),
                         overlay=torch.cat([p[4] for p in parts]) if overlay else None)

    def _chunk(self, x: torch.Tensor, targets: torch.Tensor | None, mean_std: torch.Tensor, lut: torch.Tensor | None):
        self._act = self._grad = None
        with torch.enable_grad(), torch.autocast("cuda", enabled=False):
            logits = self.model(x)
        if self._act is None:
            raise RuntimeError("the Grad-CAM target layer produced no differentiable activation in this forward")
        logits32 = logits.detach().float().contiguous()
        probs, preds = K.softmax_argmax(logits32, True)
        chosen = preds if targets is None else targets
        seed = logits.gather(1, chosen.view(-1, 1)).sum()            # ClassifierOutputTarget, summed over the batch
        torch.autograd.grad(seed, self._act)                         # the tensor hook keeps the gradient
        act, grad = self._act.detach(), self._grad
        self._act = self._grad = None
        if grad is None:
            raise RuntimeError("no gradient reached the Grad-CAM target layer")
        cam = K.gradcam_map(act.permute(0, 2, 3, 1).contiguous(), grad.permute(0, 2, 3, 1).contiguous().to(act.dtype))
        heat, over = K.cam_render(cam, (x.shape[2], x.shape[3]), x if lut is not None else None, mean_std, lut, self.image_weight)
        return logits32, probs, preds, heat, over


def label_panel(rgb_u8: np.ndarray, text: str) -> np.ndarray:
    """web_ui._add_label: white text with a black outline at the top-left corner."""
    from PIL import Image, ImageDraw, ImageFont

    img = Image.fromarray(rgb_u8)
    ImageDraw.Draw(img).text((6, 6), text, fill=(255, 255, 255), stroke_width=2, stroke_fill=(0, 0, 0),
                             font=ImageFont.load_default())
    return np.asarray(img)


def class_label(index: int, labels: dict | None = None) -> str:
    labels = labels or {}
    return str(labels.get(str(index), labels.get(index, CLASS_LABELS.get(index, f"class_{index}"))))


def export_panels(config_path: Path, images: Sequence[Path], out_dir: Path) -> list[Path]:
    """One PNG per image: a labelled Grad-CAM overlay per `selection` model, side by side (web_ui.py:117-130, :286-303)."""
    from PIL import Image

    from .orchestration.orchestrator import (
        _first_set, _resolve_weights, build_eval_transforms, console, load_config, load_model, resolve_transform_mapping,
    )
    from .orchestration.model_registry import get_model_spec
    from .orchestration.train_env import as_bool

    config = load_config(config_path)
    data_cfg = config.get("data") or {}
    device = torch.device(config.get("device") or "cuda")
    if device.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("Grad-CAM export runs on the HIP device only (no CPU fallback)")
    models_cfg = config.get("models") or {}
    names = [str(n) for n in (config.get("selection") or list(models_cfg))]
    bundles = []
    for name in names:
        cfg = models_cfg.get(name)
        if cfg is None:
            console.print(f"[bold yellow]Skipping unknown model[/]: {name}")
            continue
        infer_cfg = cfg.get("inference") or {}
        size = int(_first_set(infer_cfg.get("img_size"), data_cfg.get("img_size"), get_model_spec(name).default_image_size))
        num_classes = int(cfg.get("num_classes", data_cfg.get("num_classes", 2)))
        model = load_model(name, num_classes, _resolve_weights(infer_cfg, name, console), device, size)
        toggles = resolve_transform_mapping({"name": name, **cfg}, phase="eval")
        normalize = as_bool((toggles or {}).get("val_normalize", True))
        bundles.append((cfg.get("display_name") or cfg.get("label") or name, model, build_eval_transforms(size, toggles=toggles),
                        IMAGENET_MEAN if normalize else (0.0, 0.0, 0.0), IMAGENET_STD if normalize else (1.0, 1.0, 1.0)))
    if not bundles:
        raise RuntimeError("No models available for Grad-CAM export.")
    out_dir.mkdir(parents=True, exist_ok=True)
    written = []
    for path in images:
        with Image.open(path) as pil:
            pil = pil.convert("RGB")
            panels = []
            for display, model, transform, mean, std in bundles:
                x = transform(pil).unsqueeze(0).to(device)
                with GradCam(model, mean=mean, std=std) as cam:
                    r = cam(x, overlay=True)
                cls = int(r.preds[0])
                conf = float(r.probs[0, cls]) * 100.0
                panels.append(label_panel(r.overlay[0].cpu().numpy(), f"{display} {class_label(cls, data_cfg.get('class_labels'))} ({conf:.1f}%)"))
        heights = {p.shape[0] for p in panels}
        if len(heights) != 1:
            raise ValueError(f"panels of different heights {sorted(heights)}: give the models one img_size")
        dest = out_dir / f"{Path(path).stem}__cam.png"
        Image.fromarray(np.concatenate(panels, axis=1)).save(dest, format="PNG", optimize=True)
        console.print(f"[bold green]Saved[/]: {dest}")
        written.append(dest)
    return written


def main(argv: Sequence[str] | None = None) -> None:
    parser = argparse.ArgumentParser(description="Grad-CAM panels of the configured models, side by side (MI355X engine)")
    parser.add_argument("--config", type=Path, default=Path("config/inference_mi355x.yaml"))
    parser.add_argument("--out", type=Path, required=True)
    parser.add_argument("images", type=Path, nargs="+")
    args = parser.parse_args(argv)
    export_panels(args.config.resolve(), args.images, args.out)


if __name__ == "__main__":
    main()


__all__ = ["CamResult", "GradCam", "default_lut", "export_panels", "label_panel", "resolve_target"]
