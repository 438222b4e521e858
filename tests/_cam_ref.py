"""CPU restatement of the Grad-CAM arithmetic of csrc/dfd_cam.hip in numpy f32, operation by operation.

pytorch_grad_cam's GradCAM with one target layer (get_cam_weights, get_cam_image, np.maximum, scale_cam_image with
cv2.resize INTER_LINEAR, aggregate_multi_layers) and show_cam_on_image(img, mask, use_rgb=True): the reference's
web_ui.py:275-282.  Neither pytorch_grad_cam nor cv2 is a dependency, so their steps are written out here; numpy 2 has
weak Python scalars (NEP 50), so `1e-7 + max` and `255 * mask` stay f32 as they do in those libraries.
"""

from __future__ import annotations

import numpy as np

F32 = np.float32


def gradcam_map_f64(act: np.ndarray, grad: np.ndarray) -> np.ndarray:
    """act, grad [N, HW, C] -> max(0, sum_c mean_p(grad) * act) [N, HW], in float64 (the tolerance yardstick of dfd_gradcam_map)."""
    a, g = act.astype(np.float64), grad.astype(np.float64)
    w = g.sum(axis=1) / g.shape[1]
    return np.maximum((a * w[:, None, :]).sum(axis=2), 0.0)


def gradcam_map_f32(act: np.ndarray, grad: np.ndarray) -> np.ndarray:
    """The same map as pytorch_grad_cam computes it (f32 numpy), for the end-to-end comparison."""
    a, g = act.astype(F32), grad.astype(F32)
    w = np.mean(g, axis=1)
    return np.maximum((w[:, None, :] * a).sum(axis=2), F32(0))


def _coeffs(dst: int, src: int) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """cv2 INTER_LINEAR coefficients: scale = 1 / (dst / src) in double, fx = f32((d + 0.5) * scale - 0.5), floor, f = fx - sx;
    sx < 0 and sx >= src - 1 clamp with f = 0."""
    scale = 1.0 / (dst / src)
    s0 = np.empty(dst, np.int64)
    s1 = np.empty(dst, np.int64)
    a0 = np.empty(dst, F32)
    a1 = np.empty(dst, F32)
    for d in range(dst):
        fx = F32((d + 0.5) * scale - 0.5)
        sx = int(np.floor(fx))
        f = F32(fx - F32(sx))
        if sx < 0:
            sx, f = 0, F32(0)
        if sx >= src - 1:
            sx, f = src - 1, F32(0)
        s0[d], s1[d] = sx, min(sx + 1, src - 1)
        a0[d], a1[d] = F32(1) - f, f
    return s0, s1, a0, a1


def resize_linear(img: np.ndarray, H: int, W: int) -> np.ndarray:
    """cv2.resize(img, (W, H), interpolation=INTER_LINEAR) of an f32 [h, w] map: horizontal pass, then vertical."""
    img = img.astype(F32)
    h, w = img.shape
    x0, x1, a0, a1 = _coeffs(W, w)
    tmp = img[:, x0] * a0[None, :] + img[:, x1] * a1[None, :]
    y0, y1, b0, b1 = _coeffs(H, h)
    return tmp[y0, :] * b0[:, None] + tmp[y1, :] * b1[:, None]


def scale_cam(img: np.ndarray) -> np.ndarray:
    """pytorch_grad_cam.utils.image.scale_cam_image without the resize, one map."""
    img = img - np.min(img)
    return img / (F32(1e-7) + np.max(img))


def heatmap(cam: np.ndarray, H: int, W: int) -> np.ndarray:
    """Low-resolution ReLU'd map [h, w] -> the float heatmap [H, W]."""
    scaled = resize_linear(scale_cam(cam.astype(F32)), H, W)
    return scale_cam(np.maximum(scaled, F32(0)))


def to_rgb(x: np.ndarray, mean, std) -> np.ndarray:
    """web_ui._tensor_to_rgb: normalised f32 [3, H, W] -> HWC f32 in [0, 1]."""
    m = np.asarray(mean, F32)[:, None, None]
    s = np.asarray(std, F32)[:, None, None]
    return np.clip(x.astype(F32) * s + m, F32(0), F32(1)).transpose(1, 2, 0)


def overlay(img: np.ndarray, mask: np.ndarray, lut: np.ndarray, image_weight: float = 0.5) -> np.ndarray:
    """show_cam_on_image(img, mask, use_rgb=True) with the colour map given as an RGB uint8 [256, 3] table."""
    heat = np.float32(lut[np.uint8(255 * mask)]) / 255
    cam = (1 - image_weight) * heat + image_weight * img
    cam = cam / np.max(cam)
    return np.uint8(255 * cam)


def render(cam: np.ndarray, image: np.ndarray | None, mean, std, lut: np.ndarray | None, H: int, W: int,
           image_weight: float = 0.5) -> tuple[np.ndarray, np.ndarray | None]:
    """cam [N, h, w] f32 (+ normalised input [N, 3, H, W]) -> (heatmap [N, H, W] f32, overlay [N, H, W, 3] uint8 or None)."""
    heats = np.stack([heatmap(c, H, W) for c in cam])
    if image is None:
        return heats, None
    return heats, np.stack([overlay(to_rgb(x, mean, std), m, lut, image_weight) for x, m in zip(image, heats)])
