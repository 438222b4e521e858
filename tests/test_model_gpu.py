"""Network-level parity on the MI355X: HipEfficientNet against the CPU oracle.

The bar (BASELINE.json north_star): logits within 1e-3 relative in f32 and bit-exact
arg-max class indices on a seeded batch; gradients / optimizer step compared tensor by
tensor; bf16 (autocast) compared against the f32 oracle with bf16-appropriate tolerance,
written at each assert.  Weights travel through state_dict(), so the third-party key
compatibility is exercised as well.
"""

from __future__ import annotations

import os

import pytest
import torch

from oracle.effnet_ref import EfficientNetRef

pytestmark = pytest.mark.gpu


def _hip():
    from deepfakedetection_amd.efficientnet import HipEfficientNet
    from deepfakedetection_amd.optim import HipAdamW, HipCrossEntropyLoss

    return HipEfficientNet, HipAdamW, HipCrossEntropyLoss


def rel_err(got: torch.Tensor, want: torch.Tensor) -> float:
    got, want = got.detach().float().cpu(), want.detach().float().cpu()
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-12)


def make_pair(variant, flavour, classes, seed=5):
    HipEfficientNet, _, _ = _hip()
    torch.manual_seed(seed)
    ref = EfficientNetRef(variant, flavour, classes)
    hip = HipEfficientNet(variant, flavour, classes)
    missing = hip.load_state_dict(ref.state_dict(), strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    return ref, hip.cuda()


def warm_running_stats(ref, size, steps=3):
    ref.train()
    g = torch.Generator().manual_seed(99)
    with torch.no_grad():
        for _ in range(steps):
            ref(torch.randn(8, 3, size, size, generator=g))


@pytest.mark.parametrize("variant,flavour,size", [("b0", "timm", 224), ("b3", "lukemelas", 224), ("b3", "lukemelas", 160)])
def test_eval_logits_f32(variant, flavour, size):
    torch.manual_seed(1)
    HipEfficientNet, _, _ = _hip()
    ref = EfficientNetRef(variant, flavour, 2)
    warm_running_stats(ref, size)
    ref.eval()
    hip = HipEfficientNet(variant, flavour, 2)
    hip.load_state_dict(ref.state_dict())
    hip = hip.cuda().eval()
    x = torch.randn(8, 3, size, size, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        want = ref(x)
    with torch.inference_mode():
        got_cl = hip(x.cuda().to(memory_format=torch.channels_last))     # training-style input
        got_nchw = hip(x.cuda())                                          # inference-style input (orchestrator.class_probabilities)
    assert rel_err(got_cl, want) <= 1e-3, rel_err(got_cl, want)            # north_star: logits within 1e-3 rel f32
    assert torch.equal(got_cl.cpu(), got_nchw.cpu())
    assert torch.equal(got_cl.argmax(1).cpu(), want.argmax(1))            # bit-exact class indices


def oracle_batch(ref, flavour, N, size, seed):
    """A seeded batch with the drop-connect masks and head-dropout uniforms both sides use: (x, y, masks, u)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, 3, size, size, generator=g)
    y = torch.randint(0, 2, (N,), generator=g)
    masks = []
    for b in ref.block_list():
        c = b.c
        if c.stride == 1 and c.cin == c.cout and c.drop_connect > 0:
            keep = 1 - c.drop_connect
            masks.append(torch.floor(keep + torch.rand(N, generator=g)) / keep)
        else:
            masks.append(None)
    feat = ref._fc.in_features if flavour == "lukemelas" else ref.classifier.in_features
    u = torch.rand((N, feat), generator=g)
    return x, y, masks, u


def ref_backward(ref, batch):
    x, y, masks, u = batch
    N = x.shape[0]
    p = ref.dropout
    logits = ref(x, [None if m is None else m.view(N, 1, 1, 1) for m in masks], (u >= p).float() / (1 - p))
    loss = torch.nn.functional.cross_entropy(logits, y, label_smoothing=0.1)
    loss.backward()
    return logits, loss


def hip_backward(hip, crit, batch):
    x, y, masks, u = batch
    logits = hip(x.cuda().to(memory_format=torch.channels_last), [None if m is None else m.cuda() for m in masks], u.cuda())
    loss = crit(logits, y.cuda())
    loss.backward()
    return logits, loss


def assert_grads_match(hip, want_grads: dict, label=""):
    """Every HIP gradient against the oracle's, tensor by tensor (test_train_step_f32's yardstick); returns the floor."""
    # a BN bias that feeds (through a 1x1 conv) another training-mode BN has an exactly-zero
    # gradient; both sides then hold rounding noise (~1e-8), so errors are floored at 1e-5 of
    # the largest gradient in the network
    gmax = max(float(g.abs().max()) for g in want_grads.values())
    floor = 1e-5 * gmax
    bad = []
    report = []
    for name, prm in hip.named_parameters():
        assert prm.grad is not None, name
        want = want_grads[name]
        err = float((prm.grad.float().cpu() - want).abs().max())
        wmax = float(want.abs().max())
        report.append((err / max(wmax, 1e-30), wmax / gmax, name))
        if err > 5e-3 * wmax + floor:
            bad.append((name, err, wmax))
    # f32 vs f32, different summation orders through ~80 layers of BN backward
    assert not bad, (label, len(bad), bad[-12:])
    # per-tensor report ("what's weak" 4): every tensor whose gradient carries signal (largest entry at
    # least 1e-4 of the network's largest) is within 5e-3 of its OWN scale, squeeze-excite weights included; the
    # floor above only ever decides for tensors below that share (structurally zero gradients)
    loud = [(r, share, n) for r, share, n in report if share >= 1e-4]
    assert loud and all(r <= 5e-3 for r, _, n in loud), (label, sorted(loud, reverse=True)[:8])
    quiet = [n for _, share, n in report if share < 1e-4]
    if os.environ.get("DFD_GRAD_REPORT"):
        print("\n[grad report]", label, "tensors", len(report), "quiet", quiet)
        for r, share, n in sorted(report, reverse=True)[:12]:
            print(f"   rel {r:.2e}  share {share:.2e}  {n}")
    return floor


@pytest.mark.parametrize("variant,flavour,size", [("b0", "timm", 96), ("b3", "lukemelas", 64)])
def test_train_step_f32(variant, flavour, size):
    _, HipAdamW, HipCrossEntropyLoss = _hip()
    ref, hip = make_pair(variant, flavour, 2)
    ref.train(); hip.train()
    N = 8
    batch = oracle_batch(ref, flavour, N, size, seed=2)
    ref_logits, ref_loss = ref_backward(ref, batch)
    logits, loss = hip_backward(hip, HipCrossEntropyLoss(0.1), batch)
    assert rel_err(logits, ref_logits) <= 1e-3
    assert abs(float(loss) - float(ref_loss)) <= 1e-4 * max(1.0, abs(float(ref_loss)))
    ref_params = dict(ref.named_parameters())
    floor = assert_grads_match(hip, {n: p.grad for n, p in ref_params.items()}, f"{variant} {flavour}")
    ref_bufs = dict(ref.named_buffers())
    for name, buf in hip.named_buffers():
        if buf.dtype.is_floating_point:
            # running means of exactly-zero-mean channels are rounding noise (~1e-10): absolute floor
            err = float((buf.float().cpu() - ref_bufs[name]).abs().max())
            assert err <= 1e-4 * float(ref_bufs[name].abs().max()) + 1e-6, (name, err)
        else:
            assert int(buf) == int(ref_bufs[name]), name
    # optimizer step (trainers/efficientnet.py:487-491 hyper-parameters).  The first AdamW step
    # is lr*g/(|g|+eps): it amplifies the relative error of near-zero gradients, so exactness
    # of the update rule is tested on identical gradients in test_ops_gpu.py::test_adamw_matches_torch
    # and here only where the gradient carries signal.
    opt_ref = torch.optim.AdamW(ref.parameters(), lr=1e-4, weight_decay=5e-2)
    opt_hip = HipAdamW(hip.parameters(), lr=1e-4, weight_decay=5e-2, use_arena=False)
    before = {n: p.detach().clone().cpu() for n, p in hip.named_parameters()}
    opt_ref.step(); opt_hip.step()
    for name, prm in hip.named_parameters():
        gref = ref_params[name].grad
        mask = gref.abs() > 1e-3 * float(gref.abs().max()) + floor
        got_upd = (prm.detach().cpu() - before[name])[mask]
        want_upd = (ref_params[name].detach() - before[name])[mask]
        if mask.any():
            assert float((got_upd - want_upd).abs().max()) <= 2e-2 * 1e-4, name     # 2 % of lr
    sd = opt_hip.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}


def test_arena_gradients_are_adopted_in_place():
    """Backward kernels write into the gradient arena and autograd adopts those views as
    .grad (no copies): fixed addresses for the fused AdamW table and the DP all-reduce."""
    _, HipAdamW, HipCrossEntropyLoss = _hip()
    _, hip = make_pair("b0", "timm", 2)
    hip.train()
    opt = HipAdamW(hip.parameters(), lr=1e-4, weight_decay=5e-2)
    x = torch.randn(4, 3, 64, 64, generator=torch.Generator().manual_seed(8)).cuda()
    y = torch.zeros(4, dtype=torch.int64).cuda()
    grads = []
    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        HipCrossEntropyLoss(0.1)(hip(x, [None] * len(hip.block_list()), None), y).backward()
        assert opt.arena.holds_all_grads()
        grads.append(opt.arena.flat.clone())
        opt.step()
    assert torch.isfinite(grads[0]).all() and float(grads[0].abs().max()) > 0
    # gradient accumulation: a second backward without zero_grad must ADD, not overwrite
    opt.zero_grad(set_to_none=True)
    HipCrossEntropyLoss(0.1)(hip(x, [None] * len(hip.block_list()), None), y).backward()
    once = opt.arena.flat.clone()
    hip.eval()   # freeze BN statistics so both passes see the same function
    hip.train()
    HipCrossEntropyLoss(0.1)(hip(x, [None] * len(hip.block_list()), None), y).backward()
    twice = opt.arena.flat
    assert rel_err(twice, 2 * once) <= 1e-5


def test_weight_gradient_sums_as_passengers_give_the_same_bits():
    """kernels.sum_batch hands a block's weight-gradient slab sums to later launches (passenger workgroups of act_bn_bwd) and flushes
    the rest at the end of the backward pass: the arena must hold the same bits as with two launches per block, and a second backward
    that ACCUMULATES (temporary destinations that autograd adds) must not defer."""
    from deepfakedetection_amd import kernels as K
    _, HipAdamW, HipCrossEntropyLoss = _hip()
    _, hip = make_pair("b0", "timm", 2)
    hip.train()
    opt = HipAdamW(hip.parameters(), lr=1e-4, weight_decay=5e-2)
    x = torch.randn(8, 3, 96, 96, generator=torch.Generator().manual_seed(18)).cuda()
    y = torch.zeros(8, dtype=torch.int64).cuda()
    was = K.PASSENGER_SUMS, K.passenger_sums_enabled
    got = []
    try:
        for flag in (True, False, True):
            K.PASSENGER_SUMS, K.passenger_sums_enabled = flag, True
            hip.eval(); hip.train()
            opt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss = HipCrossEntropyLoss(0.1)(hip(x, [None] * len(hip.block_list()), None), y)
            loss.backward()
            assert opt.arena.holds_all_grads()
            got.append(opt.arena.flat.clone())
    finally:
        K.PASSENGER_SUMS, K.passenger_sums_enabled = was
    assert torch.isfinite(got[0]).all() and float(got[0].abs().max()) > 0
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2])


@pytest.mark.parametrize("variant,flavour,size", [("b0", "timm", 96), ("b3", "lukemelas", 64)])
def test_arena_train_step_f32_through_deferred_sums(variant, flavour, size, monkeypatch):
    """The production gradient path against the oracle: HipAdamW's gradient arena, so every weight-gradient slab sum of a block is
    deferred (kernels.sum_batch) and rides along with later launches as passenger workgroups (or the end-of-backward flush).  The
    same step with passengers off (two launches per block) must give the same bits, and without deferral (each sum at once) the same
    oracle match.  Then one accumulation cycle: a second micro-batch without zero_grad sums into temporary destinations that autograd
    adds to the arena, against the oracle's summed gradients of the two batches."""
    from deepfakedetection_amd import kernels as K
    assert K.PASSENGER_SUMS and K.passenger_sums_enabled, "the default gradient path is switched off"
    _, HipAdamW, HipCrossEntropyLoss = _hip()
    ref, hip = make_pair(variant, flavour, 2)
    ref.train(); hip.train()
    N = 8
    first, second = oracle_batch(ref, flavour, N, size, seed=2), oracle_batch(ref, flavour, N, size, seed=22)
    ref_backward(ref, first)
    want1 = {n: p.grad.clone() for n, p in ref.named_parameters()}
    ref_backward(ref, second)                                   # accumulates, like the HIP cycle below
    want12 = {n: p.grad.clone() for n, p in ref.named_parameters()}
    crit = HipCrossEntropyLoss(0.1)
    opt = HipAdamW(hip.parameters(), lr=1e-4, weight_decay=5e-2)
    assert opt.arena is not None
    got = {}
    for mode, switch in (("passengers", None), ("no passengers", "PASSENGER_SUMS"), ("no deferral", "_DEFER_SUMS")):
        with monkeypatch.context() as m:
            if switch:
                m.setattr(K, switch, False)
            opt.zero_grad(set_to_none=True)
            ends = K.deferred_ends[0]
            hip_backward(hip, crit, first)
            torch.cuda.synchronize()
            deferred = K.deferred_ends[0] - ends
        if mode == "passengers":
            assert deferred >= len(hip.block_list()), f"only {deferred} batches were deferred"
        else:
            assert deferred == 0, (mode, deferred)
        assert K._passenger_keep == [] and K._passenger_task is None, mode
        assert opt.arena.holds_all_grads(), mode
        got[mode] = opt.arena.flat.clone()
        assert_grads_match(hip, want1, f"{variant} {flavour} {mode}")
    assert torch.equal(got["passengers"], got["no passengers"])
    # accumulation cycle, passengers on: the first micro-batch defers into the arena slots, the second cannot
    opt.zero_grad(set_to_none=True)
    hip_backward(hip, crit, first)
    hip_backward(hip, crit, second)
    torch.cuda.synchronize()
    assert opt.arena.holds_all_grads() and K._passenger_keep == []
    assert_grads_match(hip, want12, f"{variant} {flavour} accumulated")


class _FailingBackward(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        raise RuntimeError("injected backward failure")


@pytest.mark.parametrize("where", ["head", "middle", "second"])
def test_failed_backward_leaves_no_parked_sums(where, monkeypatch):
    """A backward pass that raises never runs its end-of-backward callbacks, so the flush of the sums it parked never comes.  The next
    clean step must still produce every gradient exactly (the bits of a fresh model's step with passengers off) and leave nothing
    parked.  The failure is injected at the output of one block: near the head, in the middle, or at the second block, so that the
    pass dies with different batches parked."""
    from deepfakedetection_amd import kernels as K
    assert K.PASSENGER_SUMS and K.passenger_sums_enabled, "the default gradient path is switched off"
    _, HipAdamW, HipCrossEntropyLoss = _hip()
    crit = HipCrossEntropyLoss(0.1)
    g = torch.Generator().manual_seed(31)
    x = torch.randn(4, 3, 64, 64, generator=g).cuda().to(memory_format=torch.channels_last)
    y = torch.randint(0, 2, (4,), generator=g).cuda()

    def clean_step(hip, opt):
        hip.__dict__.pop("_rng_obj", None)                  # the same drop-connect / dropout draws as a fresh model
        opt.zero_grad(set_to_none=True)
        crit(hip(x), y).backward()
        torch.cuda.synchronize()
        assert opt.arena.holds_all_grads()
        return opt.arena.flat.clone()

    _, fresh = make_pair("b0", "timm", 2)
    fresh.train()
    with monkeypatch.context() as m:
        m.setattr(K, "PASSENGER_SUMS", False)
        want = clean_step(fresh, HipAdamW(fresh.parameters(), lr=1e-4, weight_decay=5e-2))

    _, hip = make_pair("b0", "timm", 2)
    hip.train()
    opt = HipAdamW(hip.parameters(), lr=1e-4, weight_decay=5e-2)
    blocks = hip.block_list()
    k = {"head": len(blocks) - 2, "middle": len(blocks) // 2, "second": 1}[where]        # (the last block: its batch is parked first)
    handle = blocks[k].register_forward_hook(lambda mod, inp, out: _FailingBackward.apply(out))
    try:
        opt.zero_grad(set_to_none=True)
        loss = crit(hip(x), y)
        handle.remove()
        parked = K.deferred_ends[0]
        with pytest.raises(RuntimeError, match="injected backward failure"):
            loss.backward()
        assert K.deferred_ends[0] > parked                  # the failed pass did leave batches behind
        torch.cuda.synchronize()
        got = clean_step(hip, opt)
        assert K._passenger_keep == [] and K._passenger_task is None
        assert torch.equal(got, want), int((got != want).sum())
    finally:
        handle.remove()
        K.drop_passengers()


def test_bf16_autocast_train_close_to_f32_oracle():
    _, _, HipCrossEntropyLoss = _hip()
    ref, hip = make_pair("b0", "timm", 2)
    ref.train(); hip.train()
    N, size = 16, 128
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, 3, size, size, generator=g)
    y = torch.randint(0, 2, (N,), generator=g)
    ref_logits = ref(x)
    torch.nn.functional.cross_entropy(ref_logits, y, label_smoothing=0.1).backward()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        logits = hip(x.cuda().to(memory_format=torch.channels_last), [None] * len(hip.block_list()), None)
        loss = HipCrossEntropyLoss(0.1)(logits, y.cuda())
    loss.backward()
    assert logits.dtype == torch.float32
    # bf16 activations (8 significant bits) through 80+ layers amplify rounding-order differences, so
    # the yardstick is the framework's own bf16 path: the oracle under torch.autocast("cpu", bf16) differs
    # from its f32 self by ~0.10 of the logit range here; the HIP engine must not be worse than that
    import copy

    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
        auto_logits = copy.deepcopy(ref)(x)
    yard = rel_err(auto_logits.float(), ref_logits)
    got_err = rel_err(logits, ref_logits)
    assert got_err <= max(1.25 * yard, 5e-2), (got_err, yard)
    ref_params = dict(ref.named_parameters())
    # direction of the whole gradient, and of every tensor that carries real signal
    # (exactly-zero BN-bias gradients hold only rounding noise: skipped by norm)
    ga = torch.cat([p.grad.float().cpu().flatten() for _, p in hip.named_parameters()])
    gb = torch.cat([ref_params[n].grad.flatten() for n, _ in hip.named_parameters()])
    cos_all = float(torch.dot(ga, gb) / (ga.norm() * gb.norm()))
    assert cos_all >= 0.98, cos_all
    low = []
    for name, prm in hip.named_parameters():
        a, b = prm.grad.float().cpu().flatten(), ref_params[name].grad.flatten()
        if b.norm() > 1e-4 * gb.norm():
            c = float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-30))
            if c < 0.9:
                low.append((name, round(c, 3)))
    assert not low, low


def test_head_only_warmup_matches_oracle():
    """Warm-up phase of the reference: only `_fc` trains (trainers/efficientnet.py:433-437)."""
    ref, hip = make_pair("b3", "lukemelas", 2)
    ref.train(); hip.train()
    for model in (ref, hip):
        for name, prm in model.named_parameters():
            prm.requires_grad = "_fc" in name
    x = torch.randn(4, 3, 64, 64, generator=torch.Generator().manual_seed(4))
    nb = len(hip.block_list())
    ref(x, None, None).sum().backward()
    hip(x.cuda(), [None] * nb, None).sum().backward()
    assert hip._conv_head.weight.grad is None and hip._blocks[0]._depthwise_conv.weight.grad is None
    assert rel_err(hip._fc.weight.grad, ref._fc.weight.grad) <= 1e-3
    assert rel_err(hip._fc.bias.grad, ref._fc.bias.grad) <= 1e-3


def test_cpu_input_raises():
    HipEfficientNet, _, _ = _hip()
    model = HipEfficientNet("b0", "timm", 2).cuda()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model(torch.randn(1, 3, 32, 32))


def test_reproducible_bitwise():
    """Reductions use fixed-order partial slabs, never float atomics: same inputs, same bits."""
    _, _, HipCrossEntropyLoss = _hip()
    _, hip = make_pair("b0", "timm", 2)
    hip.train()
    x = torch.randn(8, 3, 96, 96, generator=torch.Generator().manual_seed(6)).cuda()
    y = torch.zeros(8, dtype=torch.int64).cuda()
    outs = []
    for _ in range(2):
        hip.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            logits = hip(x, [None] * len(hip.block_list()), None)
            HipCrossEntropyLoss(0.1)(logits, y).backward()
        outs.append((logits.detach().clone(), hip.conv_stem.weight.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("variant,flavour,attr", [("b0", "timm", "conv_head"), ("b3", "lukemelas", "_conv_head")])
def test_grad_cam_hooks_on_head_conv(variant, flavour, attr):
    """web_ui.py:96-114 picks `_conv_head` (or the last nn.Conv2d) and pytorch_grad_cam hangs a forward hook on
    it that keeps the output activation and registers a gradient hook on it.  With hooks present the engine runs
    the head unfused (eval mode): activation and its gradient must match the oracle's."""
    ref, hip = make_pair(variant, flavour, 2)
    # calibrated running statistics (fresh ones let the signal die out in eval mode)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(4, 3, 96, 96, generator=g)
    bns = [m for m in ref.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    for m in bns:
        m.momentum = 1.0
    ref.train()
    with torch.no_grad():
        ref(x)
    hip.load_state_dict(ref.state_dict())
    ref.eval(); hip.eval()

    kept = {}

    def make_hook(tag):
        def hook(module, inputs, output):
            kept[tag + "_act"] = output
            if output.requires_grad:
                output.register_hook(lambda grad: kept.__setitem__(tag + "_grad", grad))
        return hook

    h1 = getattr(ref, attr).register_forward_hook(make_hook("ref"))
    h2 = getattr(hip, attr).register_forward_hook(make_hook("hip"))
    try:
        ref_logits = ref(x)
        ref_logits[:, 1].sum().backward()
        hip_logits = hip(x.cuda())
        hip_logits[:, 1].sum().backward()
    finally:
        h1.remove(); h2.remove()
    assert rel_err(hip_logits, ref_logits) <= 1e-3
    assert tuple(kept["hip_act"].shape) == tuple(kept["ref_act"].shape)            # NCHW, like the third-party module
    assert rel_err(kept["hip_act"], kept["ref_act"]) <= 1e-3
    assert rel_err(kept["hip_grad"], kept["ref_grad"]) <= 2e-3
    # without hooks the fused path is back
    assert rel_err(hip(x.cuda()), ref_logits) <= 1e-3


@pytest.mark.gpu
def test_eval_batchnorm_coefficients_from_one_batched_launch_track_the_buffers():
    """Eval forward: all 49 BatchNorm coefficient blocks come from one batched launch (kernels.BNEvalBatch, from the second
    pass on); the result is the per-layer path's, also after running statistics and affine parameters changed in place
    (no stale cache), and a block run on its own never uses the network's precomputed blocks."""
    from deepfakedetection_amd import functions

    def no_active_batch():
        return getattr(functions._bn_batch_tls, "batch", None) is None

    HipEfficientNet, _, _ = _hip()
    torch.manual_seed(5)
    m = HipEfficientNet("b0", "timm", 2).cuda().eval()
    x = torch.randn(4, 3, 96, 96, device="cuda")
    with torch.inference_mode():
        a, b = m(x), m._forward(x)                        # batched coefficients vs one kernel per layer
        assert torch.equal(a, b)
        assert no_active_batch()
    with torch.no_grad():
        for bn in [mod for mod in m.modules() if isinstance(mod, torch.nn.BatchNorm2d)][::5]:
            bn.running_mean.add_(0.3)
            bn.running_var.mul_(1.7)
            bn.weight.mul_(0.9)
    with torch.inference_mode():
        c, d = m(x), m._forward(x)
        assert torch.equal(c, d) and not torch.equal(a, c)
        assert no_active_batch()
        # the second eval pass replayed the first one's recording: stem 1, head 1, 16 blocks of which the first has no expand BN
        batch = m.__dict__["_bn_eval_batches"][(False, torch.float32)]
        assert len(batch.keys) == 49 and batch.ok
        blk = m.block_list()[3]
        h = torch.randn(2, 12, 12, blk.plan.cin, device="cuda")
        assert torch.isfinite(blk(h)).all()               # standalone: per-layer path
        with pytest.raises(RuntimeError, match="HIP device"):
            m(x.cpu())                                    # raises inside forward(): the pass scope is left all the same
        assert no_active_batch()


@pytest.mark.gpu
@pytest.mark.parametrize("variant,flavour", [("b0", "timm"), ("b3", "lukemelas")])
def test_inference_form_of_the_blocks_matches_the_training_form_kernels(variant, flavour, monkeypatch):
    """model.eval() without autograd runs the producer-side BatchNorm + activation chain (dfd_pwconv_fwd_eval,
    dfd_dwconv_fwd_eval, dfd_se_fwd_parts); DFD_EVAL_FUSED=0 keeps the raw-output + consumer-prologue chain.  Same
    per-stage arithmetic — only the squeeze-excite mean is added in another (fixed) order."""
    ref, hip = make_pair(variant, flavour, 2, seed=11)
    warm_running_stats(ref, 96)
    hip.load_state_dict(ref.state_dict())
    hip = hip.cuda().eval()
    x = torch.randn(6, 3, 128, 128, generator=torch.Generator().manual_seed(4)).cuda().to(memory_format=torch.channels_last)
    from deepfakedetection_amd import kernels

    calls = []
    real = kernels.dwconv_eval
    monkeypatch.setattr(kernels, "dwconv_eval", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    out = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("DFD_EVAL_FUSED", flag)
        calls.clear()
        with torch.inference_mode():
            f32 = hip(x)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                b16 = hip(x)
            again = hip(x)
        assert torch.equal(f32, again)
        assert len(calls) == (0 if flag == "0" else 3 * len(hip.block_list())), (flag, len(calls))    # the form that was asked for ran
        out[flag] = (f32.float().cpu(), b16.float().cpu())
    assert rel_err(out["1"][0], out["0"][0]) <= 1e-5, rel_err(out["1"][0], out["0"][0])
    assert rel_err(out["1"][1], out["0"][1]) <= 2e-2, rel_err(out["1"][1], out["0"][1])
    ref.eval()
    with torch.no_grad():
        want = ref(x.cpu().contiguous())
    assert rel_err(out["1"][0], want) <= 1e-3
    # with autograd on (fine-tuning a frozen, eval-mode backbone) the training-form chain still runs and keeps its tensors
    monkeypatch.setenv("DFD_EVAL_FUSED", "1")
    calls.clear()
    y = hip(x)
    assert not calls
    y.sum().backward()
    grads = [p.grad for p in hip.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads)
    assert rel_err(y, out["0"][0]) <= 1e-6
