"""The stem's weight gradient straight from the incoming gradient (csrc/dfd_stem.hip: k_stem_wgrad_fused, ABI 152; the sums from
dfd_act_bn_bwd with dz = NULL) against

  (a) the three-launch path with a stored dz on the same inputs: K.act_bn_bwd -> K.bn_bwd_finalize -> K.stem_conv_wgrad, and
  (b) the float64 formula of tests/_stem_bwd_ref.py fed with the same bf16 inputs.

dW, dgamma and dbeta may be no farther from (b) than twice the distance of (a) from (b) (max abs over the reference's RMS), and the
two BatchNorm-backward sums agree with act_bn_bwd's to rel 1e-5 of the largest sum.  The kernel recomputes dz rounding for rounding
and keeps the grid and the summation order of k_stem_wgrad_mfma, so on the default grid everything is in fact BIT-IDENTICAL to (a),
which is asserted; a squeezed grid (the entry's max_rows: workgroups walk several steps) changes the summation order and is held to
the factor 2.  Two runs give the same bits."""

import pytest
import torch

from tests._stem_bwd_ref import stem_bwd_formula

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
EPS = 1e-5


def _k():
    from deepfakedetection_amd import kernels as K
    return K


def _silu() -> int:
    from deepfakedetection_amd._lib import ACT_SILU
    return ACT_SILU


def _inputs(N, H, W, C, seed):
    gen = torch.Generator().manual_seed(seed)
    Ho, Wo = H // 2, W // 2
    x = torch.randn(N, H, W, 3, generator=gen)
    y = (torch.randn(N, Ho, Wo, C, generator=gen) * (0.5 + torch.rand(C, generator=gen)) + 0.7 * torch.randn(C, generator=gen)).to(BF)
    g = torch.randn(N, Ho, Wo, C, generator=gen).to(BF)
    gamma = 1.0 + 0.3 * torch.randn(C, generator=gen)
    beta = 0.2 * torch.randn(C, generator=gen)
    return x, y, g, gamma, beta


_cache = {}


def _case(N, H, W, C, pad):
    """Inputs on the device, the float64 reference (b) and the three-launch path (a) of one case, computed once."""
    key = (N, H, W, C, pad)
    if key in _cache:
        return _cache[key]
    K = _k()
    x, y, g, gamma, beta = _inputs(N, H, W, C, 100 + N + H + W + C + pad)
    ref = stem_bwd_formula(g.double(), y.double(), x.double(), gamma.double(), beta.double(), EPS, pad, pad)
    mean, rstd = ref["mean"], ref["rstd"]
    st = torch.stack([gamma.double() * rstd, beta.double() - mean * gamma.double() * rstd, mean, rstd]).float().cuda()
    d = dict(x=x.cuda(), y=y.cuda(), g=g.cuda(), gamma=gamma.cuda(), beta=beta.cuda(), st=st, ref=ref, M=N * (H // 2) * (W // 2))
    dz, parts, n = K.act_bn_bwd(d["g"], d["y"], None, None, st, _silu())
    rows = parts[: n * 2 * C].view(n, 2 * C).clone()
    coef, dgamma, dbeta, _, _ = K.bn_bwd_finalize(parts, n, d["M"], d["gamma"], d["beta"], None, st, True)
    dw = K.stem_conv_wgrad(d["x"], dz, d["y"], coef, 3, 2, pad, pad)
    torch.cuda.synchronize()
    d["a"] = dict(dw=dw.cpu(), dgamma=dgamma.cpu(), dbeta=dbeta.cpu(), sums=rows.double().sum(0).cpu(), rows=rows.cpu())
    _cache[key] = d
    return d


def _fused(d, pad, max_rows=0):
    K = _k()
    C = d["y"].shape[3]
    assert K.stem_bwd_fused_ok(d["x"], d["y"], 3, 2, pad, pad), "the entry point declined a shape it should serve"
    dz, parts, n = K.act_bn_bwd(d["g"], d["y"], None, None, d["st"], _silu(), want_dz=False)
    assert dz is None
    rows = parts[: n * 2 * C].view(n, 2 * C).clone()
    coef, dgamma, dbeta, _, _ = K.bn_bwd_finalize(parts, n, d["M"], d["gamma"], d["beta"], None, d["st"], True)
    dw = K.stem_bwd_fused(d["x"], d["g"], d["y"], d["st"], _silu(), coef, 3, 2, pad, pad, None, max_rows)
    torch.cuda.synchronize()
    return dict(dw=dw.cpu(), dgamma=dgamma.cpu(), dbeta=dbeta.cpu(), sums=rows.double().sum(0).cpu(), rows=rows.cpu())


def _dist(got, want):
    want = want.double()
    return float((got.double() - want).abs().max() / want.pow(2).mean().sqrt())


def _judge(d, got, what):
    ref, a = d["ref"], d["a"]
    for name in ("dw", "dgamma", "dbeta"):
        da, df = _dist(a[name], ref[name]), _dist(got[name], ref[name])
        print(f"{what} {name}: three-launch {da:.3e}  fused {df:.3e}")
        assert df <= 2.0 * da, f"{what} {name}: fused {df:.3e} > 2 x three-launch {da:.3e}"
    err = float((got["sums"] - a["sums"]).abs().max())
    scale = float(a["sums"].abs().max())
    print(f"{what} BN sums: max abs diff {err:.3e} of {scale:.3e}")
    assert err <= 1e-5 * scale, f"{what}: BN-backward sums differ by {err:.3e} (largest {scale:.3e})"


# Ho = 15 (a partial last row group), Wo = 18 / 34 (no multiple of 32), Wo = 112; (1,8,288,32): g / y and x vectors beyond the
# prefetched ones (the in-step loops); pad 1 = timm, pad 0 = lukemelas "same" (trailing pad only)
SHAPES = [(2, 16, 16, 16), (3, 20, 36, 32), (2, 30, 68, 32), (1, 224, 224, 32), (1, 8, 288, 32)]


@pytest.mark.parametrize("pad", [1, 0])
@pytest.mark.parametrize("shape", SHAPES)
def test_fused_against_three_launches_and_float64(shape, pad):
    d = _case(*shape, pad)
    got = _fused(d, pad)
    _judge(d, got, f"{shape} pad {pad}")
    again = _fused(d, pad)
    for name in ("dw", "dgamma", "dbeta", "rows"):
        assert torch.equal(got[name], again[name]), f"{name}: two runs differ"
        assert torch.equal(got[name], d["a"][name]), f"{name}: not the bits of the path with a stored dz"


@pytest.mark.parametrize("shape,max_rows", [((3, 20, 36, 32), 4), ((2, 30, 68, 32), 7), ((1, 224, 224, 32), 5)])
def test_squeezed_grid_walks_several_steps(shape, max_rows):
    """15 / 16 / 56 steps on 4 / 7 / 5 workgroups: every workgroup prefetches and walks several steps, and not all the same number."""
    N, H = shape[0], shape[1]
    steps = N * ((H // 2 + 1) // 2)
    assert steps > max_rows
    d = _case(*shape, 1)
    got = _fused(d, 1, max_rows)
    _judge(d, got, f"{shape} on {max_rows} workgroups")
    again = _fused(d, 1, max_rows)
    assert torch.equal(got["dw"], again["dw"]) and torch.equal(got["dgamma"], again["dgamma"])


def _stem_names(C):
    """Kernel-wrapper names a StemFunction backward with C output channels reports to the profile sink."""
    from deepfakedetection_amd.arch import ConvGeom
    from deepfakedetection_amd.functions import BNRef, StemCtx, StemFunction

    K = _k()
    gen = torch.Generator().manual_seed(C)
    x = torch.randn(2, 32, 32, 3, generator=gen).cuda()
    w = (0.3 * torch.randn(C, 3, 3, 3, generator=gen)).cuda().requires_grad_()
    gamma, beta = torch.ones(C).cuda().requires_grad_(), torch.zeros(C).cuda().requires_grad_()
    bn = BNRef(torch.zeros(C).cuda(), torch.ones(C).cuda(), None, 0.1, EPS)
    out = StemFunction.apply(x, w, gamma, beta, StemCtx(ConvGeom(3, 2, 1, 1), bn, BF, True))
    sink = []
    K.set_profile_sink(sink)
    try:
        out.float().square().sum().backward()
        torch.cuda.synchronize()
    finally:
        K.set_profile_sink(None)
    assert torch.isfinite(w.grad).all() and float(w.grad.abs().max()) > 0
    return [rec[0] for rec in sink]


def test_declined_shape_runs_the_three_launches():
    K = _k()
    x, y, g, gamma, beta = _inputs(2, 32, 32, 40, 9)
    assert not K.stem_bwd_fused_ok(x.cuda(), y.cuda(), 3, 2, 1, 1)
    names = _stem_names(40)
    assert "act_bn_bwd" in names and "stem_conv_wgrad" in names and "stem_bwd_fused" not in names, names
    names = _stem_names(32)
    assert "act_bn_bwd" in names and "stem_bwd_fused" in names and "stem_conv_wgrad" not in names, names


def test_captured_step_replays_the_eager_gradients():
    """EfficientNet-B0, batch 4 at 64 px: three optimizer cycles eagerly and with the captured step replayed give the same
    gradients and the same model."""
    from deepfakedetection_amd.efficientnet import HipEfficientNet
    from deepfakedetection_amd.graph_step import GraphedTrainStep
    from deepfakedetection_amd.optim import HipAdamW, HipCrossEntropyLoss

    gen = torch.Generator().manual_seed(3)
    batches = [(torch.randn(4, 3, 64, 64, generator=gen), torch.randint(0, 2, (4,), generator=gen)) for _ in range(3)]

    def run(graph: bool):
        torch.manual_seed(11)
        model = HipEfficientNet("b0", "timm", 2).cuda().train()
        opt = HipAdamW(model.parameters(), lr=1e-3, weight_decay=5e-2)
        step = GraphedTrainStep(model, HipCrossEntropyLoss(0.1), opt, accum_steps=1)
        if not graph:
            step.failed = True
        for xb, yb in batches:
            step.micro_batch(xb.cuda().contiguous(memory_format=torch.channels_last), yb.cuda(), first=True, last=True)
            step.optimizer_step()
        torch.cuda.synchronize()
        return model, step

    m_e, s_e = run(False)
    m_g, s_g = run(True)
    assert s_e.replays == 0 and not s_g.failed and s_g.replays > 0
    for (name, a), (_, b) in zip(m_e.named_parameters(), m_g.named_parameters()):
        assert (a.grad is None) == (b.grad is None), name
        assert a.grad is None or torch.equal(a.grad, b.grad), f"gradient of {name}"
    for (name, a), (_, b) in zip(m_e.state_dict().items(), m_g.state_dict().items()):
        assert torch.equal(a, b), name
