"""Gradients of the autograd stages must not depend on which OTHER inputs are frozen.

Every stage of functions.py / vit_functions.py / fastervit_functions.py that holds a "conv (+bias) + BatchNorm [+ LayerScale]"
layer (and HATFunction) is built as its oracle test builds it (tests/test_efformer_gpu.py, tests/test_fastervit_gpu.py,
tests/test_model_gpu.py: same modules, smallest parametrisation), run once in f32 with every input trainable, and then again
with each tensor input frozen alone, each trainable alone, x frozen, and (EfficientFormerV2) the reference fine-tune's
pattern.  In every case a trainable input's gradient is bit for bit the baseline's, a frozen input's .grad is None, and no
gradient holds a NaN from an unwritten buffer.  Three whole-model cases repeat this with a gradient arena, whose slots are
pre-filled with NaN: a slot that was claimed but not written, or written by the wrong launch, shows at once.
"""

from __future__ import annotations

import pytest
import torch

from tests.test_efformer_gpu import nhwc
from tests.test_efformer_gpu import randomise as randomise_ef
from tests.test_fastervit_gpu import randomise as randomise_fv

pytestmark = pytest.mark.gpu

FINE_TUNE_KEYS = ("stages.3", "blocks.3", "layer4", "bneck", "features.6", "classifier", "head")     # test_truncated_backward_...


@pytest.fixture(scope="module")
def ef():
    from deepfakedetection_amd.efficientformer_v2 import HipEfficientFormerV2

    torch.manual_seed(0)
    hip = HipEfficientFormerV2("s1", 2, 224, drop_path_rate=0.0)
    randomise_ef(hip, 1)
    return hip.cuda()


@pytest.fixture(scope="module")
def fv():
    from deepfakedetection_amd.fastervit import HipFasterViT

    torch.manual_seed(0)
    hip = HipFasterViT("0", 2, 224, drop_path_rate=0.0)
    randomise_fv(hip, 1)
    return hip.cuda()


def rand(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


class Stage:
    """One stage on fixed inputs.  leaves: name -> leaf tensor (parameters and activations); forward() -> output(s)."""

    def __init__(self, leaves: dict, forward):
        self.leaves, self.forward, self.gouts = leaves, forward, None

    def grads(self, trainable) -> dict:
        for name, t in self.leaves.items():
            t.requires_grad_(name in trainable)
            t.grad = None
        outs = self.forward()
        outs = [o for o in (outs if isinstance(outs, tuple) else (outs,)) if o is not None]
        if self.gouts is None:
            self.gouts = [rand(7 + i, *o.shape).to(o.device, o.dtype) for i, o in enumerate(outs)]
        torch.autograd.backward(outs, self.gouts)
        torch.cuda.synchronize()
        return {name: None if t.grad is None else t.grad.detach().clone() for name, t in self.leaves.items()}


def compare(label, names, trainable, got, base) -> list:
    bad = []
    for name in names:
        if name not in trainable:
            if got[name] is not None:
                bad.append(f"{label}: frozen {name} received a gradient")
        elif got[name] is None:
            bad.append(f"{label}: trainable {name} received no gradient")
        elif bool(torch.isnan(got[name]).any()):
            bad.append(f"{label}: gradient of {name} holds NaN")
        elif not torch.equal(got[name], base[name]):
            bad.append(f"{label}: gradient of {name} differs from the all-trainable run in bits")
    return bad


def check_masks(stage: Stage, prefix: str | None = None, upstream_trainable: bool = False):
    """prefix: the stage's name in EfficientFormerV2 (adds the reference fine-tune's pattern; upstream_trainable: an earlier
    stage holds a trained parameter there, so x wants its gradient)."""
    names = list(stage.leaves)
    everything = set(names)
    base = stage.grads(everything)
    bad = compare("all trainable", names, everything, base, base)
    cases = [(f"{n} frozen alone", everything - {n}) for n in names] + [(f"{n} trainable alone", {n}) for n in names]
    if "x" in everything:
        cases.append(("x without requires_grad, all parameters trainable", everything - {"x"}))
    if prefix is not None:
        tuned = {n for n in names if n != "x" and any(k in f"{prefix}.{n}" for k in FINE_TUNE_KEYS)}
        if upstream_trainable and "x" in everything:
            tuned.add("x")
        if tuned:
            cases.append(("reference fine-tune pattern", tuned))
    for label, trainable in cases:
        bad += compare(label, names, trainable, stage.grads(trainable), base)
    assert not bad, f"{len(bad)} of {len(cases) * len(names)} checks failed:\n" + "\n".join(bad)


def module_stage(mod, x, call=None) -> Stage:
    leaves = {"x": x, **dict(mod.named_parameters())}
    return Stage(leaves, (lambda: mod(x)) if call is None else call)


TRAIN = pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])


# ------------------------------------------------------------------ EfficientFormerV2 (S1)
@TRAIN
def test_conv_stem(ef, train):
    from deepfakedetection_amd._lib import ACT_GELU
    from deepfakedetection_amd.network import _bnref
    from deepfakedetection_amd.vit_functions import ConvStemCtx, ConvStemFunction

    c1 = ef.stem.conv1
    img = nhwc(rand(2, 2, 3, 64, 64)).cuda()                      # the stem gives its image no gradient: not a leaf
    cfg = ConvStemCtx(2, 1, _bnref(c1.bn), torch.float32, train, ACT_GELU, None)
    check_masks(Stage(dict(c1.named_parameters()), lambda: ConvStemFunction.apply(img, *c1.tensors(), cfg)), "stem.conv1")


@TRAIN
def test_dense_conv_bn(ef, train):
    from deepfakedetection_amd._lib import ACT_GELU
    from deepfakedetection_amd.network import _bnref
    from deepfakedetection_amd.vit_functions import DenseConvBNFunction, DenseConvCtx

    c2 = ef.stem.conv2
    x = rand(3, 2, 32, 32, 16).cuda()
    cfg = DenseConvCtx(3, 2, _bnref(c2.bn), train, ACT_GELU, None)
    check_masks(module_stage(c2, x, lambda: DenseConvBNFunction.apply(x, *c2.tensors(), cfg)), "stem.conv2")


@TRAIN
@pytest.mark.parametrize("stage,block", [(0, 0), (2, 7), (3, 5)], ids=["conv_mlp", "attention_stride2", "attention"])
def test_block(ef, stage, block, train):
    """(0, 0): ConvMlpFunction at 56 x 56; (2, 7): AttentionFunction with stride + ConvMlp; (3, 5): AttentionFunction at 7 x 7."""
    blk = ef.stages[stage].blocks[block].train(train)
    dim, res = (32, 48, 120, 224)[stage], (56, 28, 14, 7)[stage]
    x = nhwc(rand(5, 4, dim, res, res)).cuda()
    check_masks(module_stage(blk, x), f"stages.{stage}.blocks.{block}", upstream_trainable=(stage, block) > (2, 3))


@TRAIN
@pytest.mark.parametrize("stage", [1, 3], ids=["conv", "conv_and_attention"])
def test_downsample(ef, stage, train):
    ds = ef.stages[stage].downsample.train(train)
    dim, res = (32, 48, 120)[stage - 1], (56, 28, 14)[stage - 1]
    x = nhwc(rand(6, 3, dim, res, res)).cuda()
    check_masks(module_stage(ds, x), f"stages.{stage}.downsample", upstream_trainable=stage == 3)


@TRAIN
@pytest.mark.parametrize("heads", [2, 1])
def test_tail(ef, fv, heads, train):
    from deepfakedetection_amd.network import _bnref
    from deepfakedetection_amd.vit_functions import TailCtx, TailFunction

    net = ef if heads == 2 else fv
    second = (net.head_dist.weight, net.head_dist.bias) if heads == 2 else (None, None)
    x = rand(8, 4, 7, 7, net.norm.weight.numel()).cuda()
    leaves = {"x": x, "norm.weight": net.norm.weight, "norm.bias": net.norm.bias, "head.weight": net.head.weight,
              "head.bias": net.head.bias}
    if heads == 2:
        leaves.update({"head_dist.weight": second[0], "head_dist.bias": second[1]})
    cfg = TailCtx(_bnref(net.norm), 0.0, train, None)
    fwd = lambda: TailFunction.apply(x, net.norm.weight, net.norm.bias, net.head.weight, net.head.bias, *second, None, cfg)   # noqa: E731
    check_masks(Stage(leaves, fwd), "" if heads == 2 else None, upstream_trainable=True)


# ------------------------------------------------------------------ FasterViT-0
@TRAIN
def test_conv_block(fv, train):
    blk, ds = fv.levels[0].blocks[-1].train(train), fv.levels[0].downsample.train(train)
    x = nhwc(rand(3, 3, 64, 56, 56)).cuda()
    leaves = {"x": x, **dict(blk.named_parameters()), **{f"downsample.{n}": p for n, p in ds.named_parameters()}}
    check_masks(Stage(leaves, lambda: ds(blk(x))))


@TRAIN
@pytest.mark.parametrize("level", [2, 3], ids=["carrier_tokens", "plain"])
def test_hat(fv, level, train):
    """The block of test_hat_block; its coordinate tables (position tables, attention biases) are computed once and handed
    in as leaves, so that they are frozen and trained one by one like HATFunction's other inputs."""
    from deepfakedetection_amd.fastervit import _window_maps
    from deepfakedetection_amd.fastervit_functions import coord_tables

    blk = fv.levels[level].blocks[1].train(train)
    dim = 64 << level
    B = 3
    nW = B * (4 if level == 2 else 1)
    x = rand(5, nW, 49, 1, dim).cuda()
    ct = rand(6, B, 16, 1, dim).cuda() if level == 2 else None
    maps = _window_maps(B, 14, torch.device("cuda"))[1:] if level == 2 else None
    with torch.no_grad():
        tables = [t.clone() for t in coord_tables(*blk.coord_jobs())]
    leaves = {"x": x, **{f"table{i}": t for i, t in enumerate(tables)},
              **{n: p for n, p in blk.named_parameters() if "pos_emb" not in n}}
    if ct is not None:
        leaves["ct"] = ct
    check_masks(Stage(leaves, lambda: blk(x, ct, maps, None, tables)))


@TRAIN
@pytest.mark.parametrize("sr_ratio", [2, 1], ids=["carrier_tokens", "plain"])
def test_hat_with_layer_scale(sr_ratio, train):
    """test_hat on a block with LayerScale (FasterViT-0 has none): gamma1..4 are leaves, so proj's and fc2's LayerScale gradients
    and the BatchNorm-shaped backward of fc2 go through every mask.  A stand-alone block at the smallest width its kernels take
    (dim 64, head dim 32); 3 images of 12 (carrier tokens: 14 x 14 maps) or 3 windows."""
    from deepfakedetection_amd.fastervit import HipHAT, _window_maps
    from deepfakedetection_amd.fastervit_functions import coord_tables

    torch.manual_seed(0)
    blk = HipHAT(dim=64, heads=2, sr_ratio=sr_ratio, drop_path=0.0, layer_scale=1e-5, index=0)
    randomise_fv(blk, 1)                                          # gammas: 0.2 .. 0.5
    blk = blk.cuda().train(train)
    carrier = sr_ratio > 1
    B = 3
    x = rand(5, B * (4 if carrier else 1), 49, 1, 64).cuda()
    ct = rand(6, B, 16, 1, 64).cuda() if carrier else None
    maps = _window_maps(B, 14, torch.device("cuda"))[1:] if carrier else None
    with torch.no_grad():
        tables = [t.clone() for t in coord_tables(*blk.coord_jobs())]
    leaves = {"x": x, **{f"table{i}": t for i, t in enumerate(tables)},
              **{n: p for n, p in blk.named_parameters() if "pos_emb" not in n}}
    assert {"gamma3", "gamma4"} | ({"gamma1", "gamma2"} if carrier else set()) <= set(leaves)
    if ct is not None:
        leaves["ct"] = ct
    check_masks(Stage(leaves, lambda: blk(x, ct, maps, None, tables)))


# ------------------------------------------------------------------ EfficientNet-B0
@pytest.fixture(scope="module")
def en():
    """flavour -> HipEfficientNet B0 as tests/test_model_gpu.py sets its models up: the oracle's initial weights and running
    statistics warmed up by three oracle training steps.  Head dropout off, so that two passes of the whole model agree."""
    from deepfakedetection_amd.efficientnet import HipEfficientNet
    from oracle.effnet_ref import EfficientNetRef
    from tests.test_model_gpu import warm_running_stats

    made = {}

    def get(flavour):
        if flavour not in made:
            torch.manual_seed(5)
            ref = EfficientNetRef("b0", flavour, 2)
            warm_running_stats(ref, 64)
            hip = HipEfficientNet("b0", flavour, 2, drop_rate=0.0)
            hip.load_state_dict(ref.state_dict())
            made[flavour] = hip.cuda()
        return made[flavour]

    return get


@TRAIN
@pytest.mark.parametrize("flavour", ["timm", "lukemelas"])       # symmetric padding / static-same padding with its lead pad
def test_efficientnet_stem(en, flavour, train):
    from deepfakedetection_amd.functions import StemCtx, StemFunction
    from deepfakedetection_amd.network import _bnref

    net = en(flavour)
    stem, stem_bn = net._parts()[:2]
    img = nhwc(rand(2, 2, 3, 32, 32)).cuda()                      # the stem gives its image no gradient: not a leaf
    cfg = StemCtx(net.plan.stem, _bnref(stem_bn), torch.float32, train, None)
    leaves = {"weight": stem.weight, "bn.weight": stem_bn.weight, "bn.bias": stem_bn.bias}
    check_masks(Stage(leaves, lambda: StemFunction.apply(img, stem.weight, stem_bn.weight, stem_bn.bias, cfg)))


@TRAIN
@pytest.mark.parametrize("flavour,index", [("timm", 0), ("timm", 1), ("timm", 2), ("timm", 3), ("lukemelas", 1)],
                         ids=["no_expand", "expand_stride2", "skip_row_scale", "k5_stride2", "lukemelas_stride2"])
def test_mbconv(en, flavour, index, train):
    """Block 0: no expand convolution, no skip; 1: expand, stride 2; 2: expand and skip, with a drop-connect scale handed in;
    3: 5 x 5, stride 2; block 1 of the lukemelas flavour for its asymmetric padding."""
    blk = en(flavour).block_list()[index].train(train)
    p = blk.plan
    assert (p.expand, p.skip, p.dw.kernel, p.dw.stride) == [(False, False, 3, 1), (True, False, 3, 2), (True, True, 3, 1),
                                                             (True, False, 5, 2)][index]
    x = rand(3, 3, 16, 16, p.cin).cuda()
    row_scale = torch.tensor([1.25, 0.0, 1.25]).cuda() if p.skip else None
    check_masks(module_stage(blk, x, lambda: blk.run(x, row_scale)))


@TRAIN
@pytest.mark.parametrize("dropout", [True, False], ids=["dropout", "no_dropout"])
def test_efficientnet_head(en, dropout, train):
    """The classifier's weight and bias are frozen and trained one by one like every other input: a bias trained next to a
    frozen weight gets its gradient."""
    from deepfakedetection_amd.functions import HeadCtx, HeadFunction
    from deepfakedetection_amd.network import _bnref

    _, _, _, head, head_bn, fc = en("timm")._parts()
    x = rand(4, 4, 7, 7, 320).cuda()
    u = torch.rand(4, 1280, generator=torch.Generator().manual_seed(9)).cuda() if dropout else None
    cfg = HeadCtx(_bnref(head_bn), 0.2, train, None, None)
    leaves = {"x": x, "conv_head.weight": head.weight, "bn2.weight": head_bn.weight, "bn2.bias": head_bn.bias,
              "classifier.weight": fc.weight, "classifier.bias": fc.bias}
    fwd = lambda: HeadFunction.apply(x, head.weight, head_bn.weight, head_bn.bias, fc.weight, fc.bias, u, cfg)   # noqa: E731
    check_masks(Stage(leaves, fwd))


# ------------------------------------------------------------------ whole models, gradients in arena slots
def _arena_grads(model, x, y, frozen: set) -> dict:
    from deepfakedetection_amd.optim import HipAdamW, HipCrossEntropyLoss

    for name, p in model.named_parameters():
        p.requires_grad_(name not in frozen)
        p.grad = None
    opt = HipAdamW([p for p in model.parameters() if p.requires_grad], lr=1e-4, weight_decay=5e-2)
    opt.zero_grad()
    opt.arena.flat.fill_(float("nan"))                 # a slot nobody writes stays NaN
    HipCrossEntropyLoss(0.1)(model(x), y).backward()
    torch.cuda.synchronize()
    assert opt.arena.holds_all_grads()
    slot = {id(p): s for p, s in zip(opt.arena.params, opt.arena.slots)}
    out = {name: (slot[id(p)].clone() if p.requires_grad else None) for name, p in model.named_parameters()}
    for name, p in model.named_parameters():
        assert p.requires_grad or p.grad is None, f"frozen {name} received a gradient"
        p.grad = None
    opt.arena.release()
    return out


def _check_model(model, layer: tuple):
    """layer: parameter names of one mid-network layer (its weight, bias, gamma, beta or the like), each frozen alone."""
    x = rand(1, 2, 3, 224, 224).cuda()
    y = torch.tensor([0, 1]).cuda()
    model.train()
    names = [n for n, _ in model.named_parameters()]
    base = _arena_grads(model, x, y, set())
    bad = compare("all trainable", names, set(names), base, base)
    for frozen in layer:
        assert frozen in base, frozen
        bad += compare(f"{frozen} frozen alone", names, set(names) - {frozen}, _arena_grads(model, x, y, {frozen}), base)
    for p in model.parameters():
        p.requires_grad_(True)
    assert not bad, "\n".join(bad)


def test_efficientnet_b0_with_an_arena(en):
    b = "blocks.3.0"                                              # the first block of the fourth stage: expand, 3 x 3, stride 2
    _check_model(en("timm"), (f"{b}.conv_pw.weight", f"{b}.bn1.weight", f"{b}.bn1.bias", f"{b}.se.conv_reduce.bias"))


def test_efficientformer_s0_with_an_arena():
    from deepfakedetection_amd.efficientformer_v2 import HipEfficientFormerV2

    torch.manual_seed(0)
    model = HipEfficientFormerV2("s0", 2, 224, drop_path_rate=0.0)
    randomise_ef(model, 1)
    q = "stages.2.blocks.5.token_mixer.q"                         # a 1x1 + BN layer of the last stride-2 attention block
    _check_model(model.cuda(), (f"{q}.conv.weight", f"{q}.conv.bias", f"{q}.bn.weight", f"{q}.bn.bias"))


def test_fastervit_0_with_an_arena():
    from deepfakedetection_amd.fastervit import HipFasterViT

    torch.manual_seed(0)
    model = HipFasterViT("0", 2, 224, drop_path_rate=0.0)
    randomise_fv(model, 1)
    b = "levels.1.blocks.0"                                       # the first ConvBlock of level 1
    h = "levels.2.blocks.1"                                       # a HAT block with carrier tokens: one LayerNorm parameter frozen takes
    #                                                               _ln_bwd off its adjacent-slot path, either side of the test
    _check_model(model.cuda(), (f"{b}.conv1.weight", f"{b}.conv1.bias", f"{b}.norm1.weight", f"{b}.norm1.bias",
                                f"{h}.norm1.weight", f"{h}.norm1.bias", f"{h}.attn.qkv.bias", f"{h}.mlp.fc1.bias",
                                f"{h}.mlp.fc2.weight", f"{h}.hat_norm2.bias"))
