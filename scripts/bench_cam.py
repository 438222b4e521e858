"""Grad-CAM throughput: forward + hooked backward + dfd_gradcam_map + dfd_cam_render (heatmap and overlay), images/s.

    python scripts/bench_cam.py [--models efficientnet_b0,efficientformerv2_s1,faster_vit_0_224] [--batches 64,256]
                                [--steps 10] [--warmup 3] [--kernels-only]

One JSON line per (model, batch): end-to-end images/s of `GradCam(model)(x, overlay=True)` timed with device events after
warm-up, and the two new kernels on their own (device events around repeated launches on the model's target-layer shape):
dfd_gradcam_map's bytes from shapes (2 N HW C elt + N HW 4) and its fraction of the 8 TB/s HBM peak.  Random weights,
f32 eval, 224 px.  For the kernels' times from the profiler run the script under `rocprofv3 --kernel-trace --stats`
with --kernels-only.
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch  # noqa: E402

HBM_PEAK = 8.0e12            # MI355X HBM3E, bytes/s


def _events(fn, steps: int, warmup: int) -> float:
    """ms per call"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def bench(name: str, batch: int, steps: int, warmup: int, kernels_only: bool) -> dict:
    from deepfakedetection_amd import kernels as K
    from deepfakedetection_amd.cam import GradCam, default_lut, resolve_target
    from deepfakedetection_amd.orchestration.model_registry import get_model_spec

    torch.manual_seed(0)
    model = get_model_spec(name).builder(name, 2).cuda().eval()
    x = torch.randn(batch, 3, 224, 224, device="cuda")
    line: dict = {"model": name, "batch": batch, "size": 224}
    if not kernels_only:
        with GradCam(model, batch_size=batch) as cam:
            ms = _events(lambda: cam(x, overlay=True), steps, warmup)
        line["cam_ms_per_batch"] = round(ms, 3)
        line["cam_images_per_s"] = round(batch * 1e3 / ms, 1)
    # the target layer's shape: one hooked forward
    shape = {}

    def keep_shape(module, inputs, output):
        shape["s"] = tuple(output.shape)

    handle = resolve_target(model).register_forward_hook(keep_shape)
    with torch.no_grad():
        model(x[:1])
    handle.remove()
    _, C, h, w = shape["s"]
    act = torch.randn(batch, h, w, C, device="cuda").abs()
    grad = torch.randn(batch, h, w, C, device="cuda") * 1e-2
    map_ms = _events(lambda: K.gradcam_map(act, grad), max(steps, 20), warmup)
    low = K.gradcam_map(act, grad)
    lut = torch.from_numpy(default_lut().copy()).cuda()
    mean_std = torch.tensor([0.485, 0.456, 0.406, 0.229, 0.224, 0.225], device="cuda")
    render_ms = _events(lambda: K.cam_render(low, (224, 224), x, mean_std, lut), max(steps, 20), warmup)
    map_bytes = 2 * batch * h * w * C * 4 + batch * h * w * 4
    line.update({"target": [C, h, w], "map_us": round(map_ms * 1e3, 2), "map_bytes": map_bytes,
                 "map_hbm_fraction": round(map_bytes / (map_ms * 1e-3) / HBM_PEAK, 4), "render_us": round(render_ms * 1e3, 2)})
    return line


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--models", default="efficientnet_b0,efficientformerv2_s1,faster_vit_0_224")
    ap.add_argument("--batches", default="64,256")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true", help="skip the end-to-end timing (profiler runs)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_cam.py needs the MI355X"
    for name in args.models.split(","):
        for batch in (int(b) for b in args.batches.split(",")):
            print(json.dumps(bench(name, batch, args.steps, args.warmup, args.kernels_only)), flush=True)


if __name__ == "__main__":
    main()
