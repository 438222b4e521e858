"""BASELINE config 2 at its own size (EfficientNet-B0, batch 256, 224 px, bf16) — the shapes the benchmark runs.

The kernel tests of tests/test_ops_gpu.py use shapes the CPU oracle finishes in milliseconds; the persistent-grid
kernels, their 20-bit magic divisions and `int` work counters are exercised here at M = 3,211,264 rows and
616 MB tensors (round-1 review, "What's weak" item 3):

  * block 1 of B0 (16 -> 96 -> 24 channels, 112 -> 56 px, k3 s2) kernel by kernel at N = 256 through the same
    reference functions and tolerances as test_ops_gpu.py;
  * one full bf16-autocast training step at N = 256 against the f32 oracle: logits, loss, BatchNorm running
    statistics of the stem and blocks 0-2 (f32 statistics of the large tensors);
  * a 20-step f32 loss curve against the oracle;
  * every MBConv block of B0 in bf16 against an emulation of the kernels' rounding points, two bf16 ulps.
"""

from __future__ import annotations

import pytest
import torch
import torch.nn.functional as F

from oracle import ops_ref as R
from tests import test_ops_gpu as T

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
N_BASE = 256


def _hip():
    from deepfakedetection_amd.efficientnet import HipEfficientNet
    from deepfakedetection_amd.optim import HipAdamW, HipCrossEntropyLoss

    return HipEfficientNet, HipAdamW, HipCrossEntropyLoss


# ------------------------------------------------------------------ block 1 kernel by kernel at N = 256
@pytest.mark.parametrize("mode", [0, 3])
def test_expand_gemm_3_2_million_rows(mode):
    """16 -> 96 at 112x112x256: forward (mode 0, with BN statistics) and the data-gradient form (mode 3: affine2
    prologue + residual) of the wave-autonomous kernel."""
    T._pwconv_fwd_case((N_BASE, 112 * 112, 16, 96), mode, BF)


def test_expand_dgrad_shape_3_2_million_rows():
    T._pwconv_fwd_case((N_BASE, 112 * 112, 96, 16), 3, BF)


def test_project_gemm_with_gate_800k_rows():
    T._pwconv_fwd_case((N_BASE, 56 * 56, 96, 24), 2, BF)


def test_depthwise_forward_616_megabyte_input():
    T.test_dwconv_fwd((N_BASE, 112, 112, 96, 3, 2, 1, 1), BF)


def test_depthwise_backward_616_megabyte_input():
    T.test_dwconv_bwd((N_BASE, 112, 112, 96, 3, 2, 1, 1), BF)


@pytest.mark.parametrize("case", [(N_BASE, 112 * 112, 96, 16), (N_BASE, 56 * 56, 24, 96)])
def test_weight_gradients_at_baseline_rows(case):
    T.test_pwconv_wgrad_large_m(case)


def test_rowpasses_at_baseline_rows():
    T.test_rowpass((N_BASE, 112, 112, 96), BF)


# ------------------------------------------------------------------ the whole step at N = 256
def _pair(seed=5, variant="b0", flavour="timm"):
    from oracle.effnet_ref import EfficientNetRef

    Hip, _, _ = _hip()
    torch.manual_seed(seed)
    ref = EfficientNetRef(variant, flavour, 2)
    hip = Hip(variant, flavour, 2)
    hip.load_state_dict(ref.state_dict())
    return ref, hip.cuda()


def rel_err(got, want):
    got, want = got.detach().float().cpu(), want.detach().float().cpu()
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-12)


def test_full_training_step_at_the_benchmark_configuration():
    _full_step(_pair(), N_BASE, ("bn1", "blocks.0.0.bn1", "blocks.0.0.bn2", "blocks.1.0.bn1", "blocks.1.0.bn2", "blocks.1.0.bn3",
                                 "blocks.1.1.bn1", "blocks.1.1.bn2", "blocks.2.0.bn1"))


def test_b3_training_step_at_the_reference_configuration():
    """The reference's own model, efficientnet_b3 (efficientnet_pytorch flavour: static TF-SAME padding from the nominal 300 px,
    BN eps 1e-3), at its batch 64 and 224 px (config/train.yaml): 1x1 layers of 3 k .. 50 k rows and widths 136 / 232 / 816 /
    1392, where the ring-kernel planner and the depthwise occupancy classes choose differently from B0 at 256.  On top of the
    global cosine every gradient with signal is judged on its own, against the oracle's own bf16 autocast gradient of the same
    tensor (the yardstick): relative L2 error <= 2 x the yardstick's + 0.02.  Measured at this seed: 315 tensors carry
    signal; the engine's worst is 0.69 for _blocks.0._bn2.bias (yardstick 0.64), its largest ratio 1.44 (_blocks.1._bn2.weight);
    gradient cosine 0.978 against the yardstick's 0.965 — 26 random-init blocks amplify bf16 rounding further
    than B0's 16, so the global cosine is bounded by min(0.98, the yardstick's)."""
    _full_step(_pair(variant="b3", flavour="lukemelas"), 64, ("_bn0", "_blocks.0._bn1", "_blocks.0._bn2", "_blocks.2._bn0",
                                                              "_blocks.2._bn1", "_blocks.2._bn2", "_blocks.3._bn0"), per_tensor=True)


def _full_step(pair, n, bn_names, per_tensor=False):
    from tests._grad_signal import rel_l2, report, signal_names

    _, _, HipCE = _hip()
    ref, hip = pair
    ref.train(); hip.train()
    g = torch.Generator().manual_seed(1)                                  # bench.py's generator seed
    x = torch.randn(n, 3, 224, 224, generator=g).contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 2, (n,), generator=g)
    ref_logits = ref(x)
    ref_loss = F.cross_entropy(ref_logits, y, label_smoothing=0.1)
    with torch.autocast("cuda", dtype=BF):
        logits = hip(x.cuda(), [None] * len(hip.block_list()), None)
        loss = HipCE(0.1)(logits, y.cuda())
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(logits).all()
    # bf16 yardstick: the oracle itself under CPU bf16 autocast against its f32 self.  ONE such run is one realisation of bf16
    # rounding noise amplified through 80 random-init layers; another summation order anywhere in the network is another realisation
    # of the same noise (VERDICT r3 "what's weak" 2), so the yardstick is drawn several times — two memory formats (different oneDNN
    # kernels) x two batch orders (different order of the BatchNorm sums) — and the bound is their maximum plus their spread (at
    # least 15 % of their mean: four samples under-estimate the spread of a maximum over 512 logits).
    import copy

    yards = []
    with torch.no_grad(), torch.autocast("cpu", dtype=BF):
        for fmt in (torch.channels_last, torch.contiguous_format):
            for flip in (False, True):
                xi = (x.flip(0) if flip else x).contiguous(memory_format=fmt)
                auto = copy.deepcopy(ref)(xi).float()
                yards.append(rel_err(auto.flip(0) if flip else auto, ref_logits))
    spread = max(max(yards) - min(yards), 0.15 * sum(yards) / len(yards))
    bound = max(yards) + spread
    err = rel_err(logits, ref_logits)
    print(f"logits rel err {err:.4f}; the oracle's own bf16 autocast, four realisations: {[round(v, 4) for v in yards]} -> bound {bound:.4f}; "
          f"loss {float(loss):.5f} vs {float(ref_loss):.5f}")
    assert err <= max(bound, 2e-2), (err, yards, bound)
    assert abs(float(loss) - float(ref_loss)) <= 2e-2 * max(1.0, abs(float(ref_loss)))
    # BatchNorm running statistics of the large early layers: f32 sums over 3.2 M bf16 values per channel
    rb, hb = dict(ref.named_buffers()), dict(hip.named_buffers())
    for name in bn_names:
        for stat in ("running_mean", "running_var"):
            a, b = hb[f"{name}.{stat}"].float().cpu(), rb[f"{name}.{stat}"]
            scale = float(b.abs().max())
            assert float((a - b).abs().max()) <= 2e-2 * scale + 1e-4, (name, stat, float((a - b).abs().max()), scale)
    # every parameter received a finite gradient through the persistent grids
    for name, p in hip.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
    ga = torch.cat([p.grad.float().cpu().flatten() for _, p in hip.named_parameters()])
    ref_loss.backward()
    rp = dict(ref.named_parameters())
    gb = torch.cat([rp[n].grad.flatten() for n, _ in hip.named_parameters()])
    cos = float(torch.dot(ga, gb) / (ga.norm() * gb.norm()))
    print(f"gradient cosine vs f32 oracle at N={n}: {cos:.4f}")
    cos_floor = 0.98
    if per_tensor:
        rg = {name: p.grad for name, p in ref.named_parameters()}
        hg = dict(hip.named_parameters())
        auto = copy.deepcopy(ref)
        auto.zero_grad(set_to_none=True)
        with torch.autocast("cpu", dtype=BF):
            F.cross_entropy(auto(x), y, label_smoothing=0.1).backward()
        ag = dict(auto.named_parameters())
        gc = torch.cat([ag[nm].grad.float().flatten() for nm, _ in hip.named_parameters()]).double()
        cos_yard = float(torch.dot(gc, gb.double()) / (gc.norm() * gb.double().norm()))
        print(f"the oracle's own bf16 autocast: gradient cosine {cos_yard:.4f}")
        cos_floor = min(cos_floor, cos_yard)
        names = signal_names(rg)
        errs = {name: rel_l2(hg[name].grad, rg[name]) for name in names}
        yard = {name: rel_l2(ag[name].grad, rg[name]) for name in names}
        print(report(errs, yard, top=30))
        print("largest ratios to the yardstick:", sorted(((round(errs[k] / yard[k], 3), k) for k in names), reverse=True)[:8])
        assert len(names) >= 0.5 * len(rg), (len(names), len(rg))
        bad = sorted(((errs[k], yard[k], k) for k in names if errs[k] > 2 * yard[k] + 0.02), reverse=True)
        assert not bad, bad[:8]
    assert cos >= cos_floor, (cos, cos_floor)


def test_twenty_step_loss_curve_f32():
    """Same seed, same inputs, same dropout uniforms, f32 on both sides: the loss curves must track each other
    (SURVEY.md section 7 step 7).  AdamW lr 1e-3 so that 20 steps move the loss visibly."""
    _, HipAdamW, HipCE = _hip()
    ref, hip = _pair(seed=9)
    ref.train(); hip.train()
    N, size = 8, 96
    g = torch.Generator().manual_seed(4)
    xs = [torch.randn(N, 3, size, size, generator=g) for _ in range(4)]
    ys = [torch.randint(0, 2, (N,), generator=g) for _ in range(4)]
    opt_r = torch.optim.AdamW(ref.parameters(), lr=1e-3, weight_decay=5e-2)
    opt_h = HipAdamW(hip.parameters(), lr=1e-3, weight_decay=5e-2)
    crit = HipCE(0.1)
    p = ref.dropout
    curve = []
    for step in range(20):
        x, y = xs[step % 4], ys[step % 4]
        u = torch.rand((N, 1280), generator=g)
        opt_r.zero_grad(set_to_none=True)
        lr_ = F.cross_entropy(ref(x, None, (u >= p).float() / (1 - p)), y, label_smoothing=0.1)
        lr_.backward()
        opt_r.step()
        opt_h.zero_grad(set_to_none=True)
        lh = crit(hip(x.cuda(), [None] * len(hip.block_list()), u.cuda()), y.cuda())
        lh.backward()
        opt_h.step()
        curve.append((float(lr_), float(lh)))
    worst = max(abs(a - b) / max(1.0, abs(a)) for a, b in curve)
    print("loss curve (oracle, hip):", [(round(a, 4), round(b, 4)) for a, b in curve[::4]], "worst rel dev", worst)
    assert curve[-1][0] < curve[0][0]                      # it trained
    assert worst <= 5e-3, curve


# ------------------------------------------------------------------ per-block bf16 with the kernels' rounding points
def _block_ref_bf16(blk, x, eps):
    """MBConv forward (training-mode BN, no drop-connect) with a rounding to bf16 wherever the kernels store or
    stage a value: raw conv outputs, the activated tensor staged in LDS / loaded into MFMA fragments, the gated
    project operand, the block output.  Statistics are f32 sums over the ROUNDED raw tensors, as in the kernels.
    Both flavours: timm (symmetric k // 2 padding) and efficientnet_pytorch (the block's static TF-SAME padding, which may be
    asymmetric: (0, 1) for the 3x3 stride-2 layers of B3); eps is the flavour's BatchNorm eps."""
    rd = BF
    c = blk.c
    lm = hasattr(blk, "_depthwise_conv")

    def st_of(y, bn):
        return R.bn_state(y, bn.weight.detach(), bn.bias.detach(), eps)

    N, H, W, _ = x.shape
    if lm:
        expand, expand_bn, dw, dw_bn, proj, proj_bn = (getattr(blk, n, None) for n in ("_expand_conv", "_bn0", "_depthwise_conv", "_bn1",
                                                                                        "_project_conv", "_bn2"))
        se_r, se_e = blk._se_reduce, blk._se_expand
        pl, pr, pt, pb = c.pad_dw
    else:
        if c.expand != 1:
            expand, expand_bn, dw, dw_bn, proj, proj_bn = blk.conv_pw, blk.bn1, blk.conv_dw, blk.bn2, blk.conv_pwl, blk.bn3
        else:
            expand, expand_bn, dw, dw_bn, proj, proj_bn = None, None, blk.conv_dw, blk.bn1, blk.conv_pw, blk.bn2
        se_r, se_e = blk.se.conv_reduce, blk.se.conv_expand
        pl = pr = pt = pb = c.k // 2
    if c.expand != 1:
        w = expand.weight.detach().flatten(1)
        y1 = R.rnd(x @ R.rnd(w, rd).t(), rd)
        st1 = st_of(y1, expand_bn)
        dw_in, dw_st, dw_act = y1, st1, R.ACT_SILU
    else:
        dw_in, dw_st, dw_act = x, None, 0
    k, s = c.k, c.stride
    Ho, Wo = (H + pt + pb - k) // s + 1, (W + pl + pr - k) // s + 1
    y2 = R.dwconv_fwd(dw_in, dw_st, dw_act, dw.weight.detach(), k, s, pt, pl, Ho, Wo, rd)
    st2 = st_of(y2, dw_bn)
    a2 = R.rnd(R.act_fwd(st2[0] * y2 + st2[1], R.ACT_SILU), rd)
    pooled = a2.mean((1, 2))
    _, gate = R.se_fc(pooled, se_r.weight.detach().flatten(1), se_r.bias.detach(),
                      se_e.weight.detach().flatten(1), se_e.bias.detach(), R.ACT_SILU)
    A = R.rnd(a2 * gate[:, None, None, :], rd)
    y3 = R.rnd(A @ R.rnd(proj.weight.detach().flatten(1), rd).t(), rd)
    st3 = st_of(y3, proj_bn)
    out = st3[0] * y3 + st3[1]
    if c.stride == 1 and c.cin == c.cout:
        out = out + x
    return R.rnd(out, rd)


@pytest.mark.parametrize("index", list(range(16)))
def test_every_b0_block_in_bf16_within_two_ulps_of_the_rounding_emulation(index):
    res = {0: 56, 1: 56, 2: 28, 3: 28, 4: 14, 5: 14, 6: 14, 7: 14, 8: 14, 9: 14, 10: 14, 11: 14, 12: 7, 13: 7, 14: 7, 15: 7}[index]
    _block_in_bf16(_pair(seed=21), index, res, 1e-5)


def _b3_block_inputs():
    """Input side of each B3 block at half the 224-px map size (as the B0 cases use), at least 7: 56 for stage 0 ... 7."""
    from oracle.effnet_ref import build_cfg

    size, out = 112, []
    for c in build_cfg("b3", "lukemelas")[2]:
        out.append(max(size // 2, 7))
        size = -(-size // c.stride)
    return out


@pytest.mark.parametrize("index", list(range(26)))
def test_every_b3_block_in_bf16_within_two_ulps_of_the_rounding_emulation(index):
    """The reference's model: efficientnet_pytorch B3 blocks (static TF-SAME padding computed for 300 px, asymmetric (0, 1) on
    the 3x3 stride-2 layers; BN eps 1e-3; SE widths 6 .. 96; widths 24 .. 2304)."""
    _block_in_bf16(_pair(seed=22, variant="b3", flavour="lukemelas"), index, _b3_block_inputs()[index], 1e-3)


def _block_in_bf16(pair, index, res, eps):
    ref, hip = pair
    rblk, hblk = ref.block_list()[index], hip.block_list()[index]
    c = rblk.c
    g = torch.Generator().manual_seed(100 + index)
    x = torch.randn(8, res, res, c.cin, generator=g).to(BF)
    # non-trivial BN affine parameters on both sides
    with torch.no_grad():
        hp = dict(hblk.named_parameters())
        for n1, p1 in rblk.named_parameters():
            if ".bn" in n1 or n1.startswith("bn") or n1.startswith("_bn"):
                v = 0.6 + 0.8 * torch.rand(p1.shape, generator=g) if n1.endswith("weight") else torch.randn(p1.shape, generator=g) * 0.2
                p1.copy_(v); hp[n1].copy_(v.cuda())
    rblk.train(); hblk.train()
    assert all(m.eps == eps for m in rblk.modules() if isinstance(m, torch.nn.BatchNorm2d))
    want = _block_ref_bf16(rblk, x.float(), eps)
    got = hblk.run(x.cuda(), None, None)
    assert got.dtype == BF
    scale = float(want.abs().max())
    err = float((got.float().cpu() - want).abs().max()) / scale
    assert err <= 1.6e-2, f"block {index}: {err:.4f} of max |out| {scale:.3f} (two bf16 ulps = 1.6e-2)"
