"""dfd_gradcam_map / dfd_cam_render on the MI355X against the numpy restatement (tests/_cam_ref.py): the map within f32
summation error of a float64 restatement, bitwise reproducible; the heatmap and the overlay bit for bit; bad shapes refused."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import _cam_ref as R

pytestmark = pytest.mark.gpu

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def _K():
    from deepfakedetection_amd import kernels

    return kernels


def _inputs(N, HW, C, seed):
    g = torch.Generator().manual_seed(seed)
    act = torch.randn(N, HW, C, generator=g).abs() * torch.rand(1, 1, C, generator=g)     # post-activation-like, mixed scales
    grad = torch.randn(N, HW, C, generator=g) * 1e-2 + 2e-3
    return act, grad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("HW", [1, 4, 49, 196])
@pytest.mark.parametrize("C", [8, 200, 1280, 2048])
def test_gradcam_map_matches_float64(HW, C, dtype):
    K = _K()
    act, grad = _inputs(3, HW, C, seed=HW * 7919 + C)
    act, grad = act.to(dtype), grad.to(dtype)                       # the bf16 case compares against the rounded inputs
    side = {1: (1, 1), 4: (2, 2), 49: (7, 7), 196: (14, 14)}[HW]
    got = K.gradcam_map(act.view(3, *side, C).cuda(), grad.view(3, *side, C).cuda()).cpu().numpy().reshape(3, HW)
    a, g = act.double().numpy(), grad.double().numpy()
    want = R.gradcam_map_f64(a, g)
    # summation error is relative to the sum of magnitudes, not to a (possibly cancelling) result
    scale = (np.abs(a) * np.abs(g.mean(axis=1))[:, None, :]).sum(axis=2).max()
    err = np.abs(got - want).max() / scale
    assert err <= 1e-5, f"rel {err:.2e}"
    assert (got >= 0).all()


def test_gradcam_map_is_bitwise_reproducible():
    K = _K()
    act, grad = _inputs(16, 49, 1280, seed=3)
    a, g = act.view(16, 7, 7, 1280).cuda(), grad.view(16, 7, 7, 1280).cuda()
    first = K.gradcam_map(a, g)
    for _ in range(2):
        assert torch.equal(K.gradcam_map(a, g), first)


def _lut_dev():
    from deepfakedetection_amd.cam import default_lut

    lut = default_lut()
    return lut, torch.from_numpy(lut.copy()).cuda()


@pytest.mark.parametrize("h,w,H,W", [(7, 7, 224, 224), (14, 14, 224, 224), (7, 7, 96, 128), ("const", 7, 224, 224)])
def test_cam_render_is_bitwise_equal_to_the_reference(h, w, H, W):
    K = _K()
    N = 3
    g = torch.Generator().manual_seed(21)
    if h == "const":
        h = 7
        cam = torch.full((N, h, w), 0.625)
    else:
        cam = torch.relu(torch.randn(N, h, w, generator=g))
    image = torch.randn(N, 3, H, W, generator=g) * 1.2
    lut, lut_d = _lut_dev()
    mean_std = torch.tensor(MEAN + STD, dtype=torch.float32).cuda()
    heat, over = K.cam_render(cam.cuda(), (H, W), image.cuda(), mean_std, lut_d, 0.5)
    want_heat, want_over = R.render(cam.numpy(), image.numpy(), MEAN, STD, lut, H, W, 0.5)
    np.testing.assert_array_equal(heat.cpu().numpy(), want_heat)
    np.testing.assert_array_equal(over.cpu().numpy(), want_over)
    heat_only, none = K.cam_render(cam.cuda(), (H, W))
    assert none is None and torch.equal(heat_only, heat)
    if float(cam.max()) == float(cam.min()):
        assert not heat.any()


def test_bad_shapes_are_refused():
    from deepfakedetection_amd import _lib

    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    act = torch.zeros(2, 49, 64, device="cuda")
    cam = torch.zeros(2, 49, device="cuda")
    heat = torch.zeros(2, 224, 224, device="cuda")
    ws = torch.zeros(2 * 7 * 224, device="cuda")
    p = lambda t: t.data_ptr()                                          # noqa: E731
    EINVAL, EWORKSPACE = -1, -4
    assert lib.dfd_gradcam_map(p(act), p(act), 0, 0, 49, 64, p(cam), s) == EINVAL        # N = 0
    assert lib.dfd_gradcam_map(p(act), p(act), 0, 2, 0, 64, p(cam), s) == EINVAL         # HW = 0
    assert lib.dfd_gradcam_map(p(act), p(act), 0, 2, 49, 0, p(cam), s) == EINVAL         # C = 0
    assert lib.dfd_gradcam_map(p(act), p(act), 0, 2, 1, 16385, p(cam), s) == EINVAL     # C beyond the LDS table
    assert lib.dfd_gradcam_map(p(act), p(act), 7, 2, 49, 64, p(cam), s) == EINVAL        # dtype
    ok = lib.dfd_cam_render_ws(2, 7, 7, 224, 224)
    assert lib.dfd_cam_render(p(cam), 2, 0, 7, 224, 224, None, None, None, 0.5, p(heat), None, p(ws), ok, s) == EINVAL
    assert lib.dfd_cam_render(p(cam), 2, 7, 7, 224, -1, None, None, None, 0.5, p(heat), None, p(ws), ok, s) == EINVAL
    assert lib.dfd_cam_render(p(cam), 2, 7, 7, 224, 224, None, None, None, 0.5, p(heat), p(heat), p(ws), ok, s) == EINVAL  # overlay without image
    assert lib.dfd_cam_render(p(cam), 2, 7, 7, 224, 224, None, None, None, 0.5, p(heat), None, p(ws), ok - 4, s) == EWORKSPACE
    assert lib.dfd_cam_render(p(cam), 2, 7, 7, 224, 224, None, None, None, 0.5, p(heat), None, None, ok, s) == EWORKSPACE
    with pytest.raises(ValueError):
        _K().gradcam_map(act.view(2, 7, 7, 64), act.view(2, 7, 7, 64).bfloat16())
    torch.cuda.synchronize()
