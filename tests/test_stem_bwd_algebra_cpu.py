"""The algebra of a ONE-pass stem backward, in float64 on the CPU: the stem has no data gradient, so the BatchNorm-backward map can
be applied to the pixel sums — the weight gradient assembled from A = sum dz patch, B = sum yh patch, S = sum patch and the two
BatchNorm-backward means equals autograd through conv2d + BatchNorm (training) + SiLU, also when the convolution output sits far
from zero (|mean| >> sigma), where a form built on the raw y would cancel.  tests/_stem_bwd_ref.py is also the float64 reference of
tests/test_stem_bwd_fused_gpu.py.  (The shipped kernel does NOT use this factoring: it rounds dz and the mapped gradient exactly as
the kernels it replaces, so that the stem's gradient keeps its bits — DESIGN.md section 9.)"""

import pytest
import torch
import torch.nn.functional as F

from tests._stem_bwd_ref import stem_bwd_formula

EPS = 1e-5


@pytest.mark.parametrize("shift", [0.0, 50.0])
def test_combined_weight_gradient_equals_autograd(shift):
    gen = torch.Generator().manual_seed(5)
    N, H, W, C = 2, 12, 12, 16
    x = torch.randn(N, 3, H, W, generator=gen, dtype=torch.float64)
    w = (0.3 * torch.randn(C, 3, 3, 3, generator=gen, dtype=torch.float64)).requires_grad_()
    gamma = (1.0 + 0.3 * torch.randn(C, generator=gen, dtype=torch.float64)).requires_grad_()
    beta = (0.2 * torch.randn(C, generator=gen, dtype=torch.float64)).requires_grad_()
    g = torch.randn(N, C, H // 2, W // 2, generator=gen, dtype=torch.float64)
    y = F.conv2d(x, w, stride=2, padding=1) + shift               # [2,16,6,6]; the shift is a convolution bias
    out = F.silu(F.batch_norm(y, None, None, gamma, beta, training=True, eps=EPS))
    (out * g).sum().backward()
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).contiguous()
    got = stem_bwd_formula(nhwc(g), nhwc(y), nhwc(x), gamma.detach(), beta.detach(), EPS, 1, 1)
    for name, want in (("dw", w.grad), ("dgamma", gamma.grad), ("dbeta", beta.grad)):
        err = float((got[name] - want).abs().max())
        assert err <= 1e-10, f"{name} (shift {shift}): {err:.3e}"
