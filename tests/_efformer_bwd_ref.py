"""One EfficientFormerV2 stage on fixed inputs, three ways: the oracle sub-module in float64 (the reference), the same sub-module
with f32 parameters under CPU bf16 autocast (the yardstick: what bf16 rounding alone costs each tensor) and the HIP sub-module
(the engine).  For tests/test_efformer_bf16_gpu.py; tests/test_efformer_bf16_ref_cpu.py checks the reference on its own.

The vocabulary is tests/_mbconv_bwd_ref.py's.  A case names a sub-module of oracle.efformer_ref.EfficientFormerV2Ref:
  block       stages[stage].blocks[block]: [x + m1 * ls1 * Attention2d(x)] then x + m2 * ls2 * ConvMlp(x)
  downsample  stages[stage].downsample: conv3x3 s2 + BN [+ the Attention2dDownsample branch]
  stem        ref.stem on a [N, 224, 224, 3] image (ConvStemFunction and DenseConvBNFunction); the engine takes no gradient for
              the image, so there is no `x.grad`
  tail        norm -> mean(H, W) -> [dropout] -> (head + head_dist) / 2; `scaled` hands in an explicit dropout draw u with
              p = 0.2, applied here as (u >= p) / (1 - p), which is what TailFunction's drop_u does
The sub-module is randomised with test_efformer_gpu.randomise under a seed derived from the case id; the 1x1 convolution weights
are then rounded to bf16-representable values, as kernels.prep_weights rounds them in the engine, so that weight rounding stays
out of the comparison (as in _mbconv_bwd_ref).  x and the output gradient hold bf16-representable values.

`scaled` block cases carry two DropPath row scales, written down below and not drawn: MIXER for the token-mixer branch and MLP
for the ConvMlp branch, both with dropped images (0.0: at least images 1 and N - 1) and kept ones (1 / 0.8).  The oracle takes
them through Block.forward(x, masks); the engine through HipBlock.forward(x, rng=fake) with hb.drop_path = 0.2, where the fake
generator asserts keep == 0.8 and stream id 2 * index + which — HipBlock._scale and its wiring are under test.

Structural zeros.  A tensor is structurally zero when its float64 gradient's largest entry is below 1e-9 of its sibling
weight's (measured 3e-16 .. 3e-13 against siblings of 1 .. 300).  expected_zeros() names them from the arithmetic:
  * training mode: every `*.conv.bias` (the batch mean of the BatchNorm behind it absorbs it), `k.bn.bias` and
    `talking_head1.bias` (they shift all keys of a softmax row equally), `stride_conv.bn.bias` (a per-channel constant in front
    of the 1x1 + batch-statistics BatchNorm of q, k and v) and the downsample's `q.local.bias` (likewise, in front of q.proj);
  * eval mode: `k.conv.bias`, `k.bn.bias` and `talking_head1.bias` only.
They are not left out: their error is ||got|| / ||ref[sibling]|| and their yardstick is the sibling's, so the bound reads
||got|| <= (FACTOR * yard[sibling] + FLOOR) * ||ref[sibling]||; exact_zeros() names those that must be exactly zero (the
`.conv.bias` of training mode, as test_efformer_gpu.check_param_grads demands).
"""

from __future__ import annotations

import copy
import functools
import zlib
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from tests._grad_signal import rel_l2

BF = torch.bfloat16
FLOOR = 2e-3                                                     # as tests/_mbconv_bwd_ref.py
KEEP = 0.8                                                       # DropPath keep probability of the scaled cases
P_DROP = 0.2                                                     # dropout probability of the scaled tail case
NC = 2
RES = (56, 28, 14, 7)
ZERO = 1e-9                                                      # structurally zero: below this fraction of the sibling weight's


@dataclass(frozen=True)
class Case:
    variant: str
    kind: str                                                    # block | downsample | stem | tail
    stage: int
    block: int
    n: int
    scaled: bool = False                                         # block: DropPath row scales; tail: a dropout draw
    train: bool = True

    @property
    def id(self) -> str:
        what = {"block": f"block{self.stage}.{self.block}", "downsample": f"downsample{self.stage}", "stem": "stem", "tail": "tail"}[self.kind]
        return (f"{self.variant}-{what}-n{self.n}" + ("" if self.train else "-eval")
                + (("-dropout" if self.kind == "tail" else "-scaled") if self.scaled else ""))

    @property
    def seed(self) -> int:
        return zlib.crc32(self.id.encode()) % (1 << 31)


# the cases of tests/test_efformer_bf16_gpu.py, each the smallest at which the path named still runs
CONVMLP = [Case("s1", "block", 0, 0, 63, scaled=True), Case("s1", "block", 0, 0, 63),     # 197,568 rows: fused expand backward
           Case("s1", "block", 0, 0, 62), Case("l", "block", 0, 4, 63),                    # its neighbours: 194,432 rows; C = 40
           Case("s1", "block", 2, 3, 64, scaled=True),                                     # 12,544 rows, C = 120: ring kernel
           Case("s1", "block", 3, 0, 37)]                                                  # 1,813 rows, C = 224
ATTENTION = [Case("s1", "block", 2, 7, 4), Case("s1", "block", 2, 7, 37, scaled=True), Case("s1", "block", 2, 7, 37),
             Case("s1", "block", 2, 7, 64, scaled=True), Case("s1", "block", 2, 7, 37, train=False),
             Case("s1", "block", 3, 5, 37, scaled=True), Case("s1", "block", 3, 5, 64),
             Case("s2", "block", 2, 8, 37), Case("l", "block", 3, 9, 37)]
DOWNSAMPLE = [Case("s1", "downsample", 1, 0, 16), Case("s1", "downsample", 3, 0, 4), Case("s1", "downsample", 3, 0, 37)]
STEM = [Case("s1", "stem", 0, 0, 4)]
TAIL = [Case("s1", "tail", 3, 0, 37), Case("s1", "tail", 3, 0, 37, scaled=True)]
CASES = CONVMLP + ATTENTION + DOWNSAMPLE + STEM + TAIL


def mixer_scale(n: int) -> torch.Tensor:
    """The token-mixer branch's row scale: images 1, N - 1 and every i with i % 7 == 2 are dropped."""
    return torch.tensor([0.0 if i in (1, n - 1) or i % 7 == 2 else 1.0 / KEEP for i in range(n)])


def mlp_scale(n: int) -> torch.Tensor:
    """The MLP branch's row scale: images 1, N - 1 and every i with i % 5 == 3 are dropped."""
    return torch.tensor([0.0 if i in (1, n - 1) or i % 5 == 3 else 1.0 / KEEP for i in range(n)])


class Tail(torch.nn.Module):
    """norm -> mean(H, W) -> [(u >= p) / (1 - p)] -> (head + head_dist) / 2 on the network's own norm, head and head_dist."""

    def __init__(self, net) -> None:
        super().__init__()
        self.norm, self.head, self.head_dist = net.norm, net.head, net.head_dist

    def forward(self, x: torch.Tensor, u: torch.Tensor | None = None) -> torch.Tensor:
        n = self.norm
        x = F.batch_norm(x, n.running_mean, n.running_var, n.weight, n.bias, self.training, n.momentum, n.eps).mean(dim=(2, 3))
        if u is not None:
            x = x * ((u >= P_DROP).to(x.dtype) / (1.0 - P_DROP))
        return (F.linear(x, self.head.weight, self.head.bias) + F.linear(x, self.head_dist.weight, self.head_dist.bias)) / 2


@dataclass
class Inputs:
    case: Case
    mod: torch.nn.Module                                         # the oracle sub-module, f32, randomised, in the case's mode
    x: torch.Tensor                                              # [N, H, W, C] f32 holding bf16 values
    g: torch.Tensor                                              # gradient of the output: [N, Ho, Wo, Co], tail [N, NC]; likewise
    masks: tuple | None                                          # (mixer or None, mlp) [N] f32 row scales of a scaled block
    u: torch.Tensor | None                                       # [N, C] f32 dropout draw of the scaled tail

    @property
    def attention(self) -> bool:
        return getattr(self.mod, "token_mixer", None) is not None or getattr(self.mod, "attn", None) is not None


@functools.lru_cache(maxsize=None)
def oracle_net(variant: str):
    from oracle.efformer_ref import EfficientFormerV2Ref

    torch.manual_seed(31)
    return EfficientFormerV2Ref(variant, NC, 224, drop_path_rate=0.0)


@functools.lru_cache(maxsize=None)
def hip_net(variant: str):
    from deepfakedetection_amd.efficientformer_v2 import HipEfficientFormerV2

    return HipEfficientFormerV2(variant, NC, 224, drop_path_rate=0.0)


def _sub(net, case: Case, tail_cls):
    if case.kind == "block":
        return net.stages[case.stage].blocks[case.block]
    if case.kind == "downsample":
        return net.stages[case.stage].downsample
    return net.stem if case.kind == "stem" else tail_cls(net)


@functools.lru_cache(maxsize=None)
def inputs(case: Case) -> Inputs:
    from oracle.efformer_ref import WIDTHS
    from tests.test_efformer_gpu import randomise

    mod = copy.deepcopy(_sub(oracle_net(case.variant), case, Tail))
    randomise(mod, case.seed)
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, torch.nn.Conv2d) and m.kernel_size == (1, 1) and m.in_channels > 8:      # (not the talking heads)
                m.weight.copy_(m.weight.to(BF).float())
    w = WIDTHS[case.variant]
    n = case.n
    xs, gs = {"block": lambda: ((n, RES[case.stage], RES[case.stage], w[case.stage]),) * 2,
              "downsample": lambda: ((n, RES[case.stage - 1], RES[case.stage - 1], w[case.stage - 1]), (n, RES[case.stage], RES[case.stage], w[case.stage])),
              "stem": lambda: ((n, 224, 224, 3), (n, 56, 56, w[0])),
              "tail": lambda: ((n, 7, 7, w[3]), (n, NC))}[case.kind]()
    gen = torch.Generator().manual_seed(case.seed + 1)
    x = torch.randn(xs, generator=gen).to(BF).float()
    g = torch.randn(gs, generator=gen).to(BF).float()
    masks = u = None
    if case.scaled and case.kind == "block":
        assert case.train
        mod.dp = 1.0 - KEEP
        masks = (mixer_scale(n) if mod.token_mixer is not None else None, mlp_scale(n))
    elif case.scaled:
        assert case.kind == "tail" and case.train
        u = torch.rand(n, w[3], generator=gen)
    return Inputs(case, mod.train(case.train), x, g, masks, u)


def nchw(t: torch.Tensor) -> torch.Tensor:
    return t.permute(0, 3, 1, 2) if t.dim() == 4 else t


def _oracle_pass(mod, inp: Inputs, dtype: torch.dtype) -> dict[str, torch.Tensor]:
    """Forward and backward of (a copy of) the oracle sub-module on contiguous NCHW inputs of `dtype`; everything in float64."""
    kind = inp.case.kind
    x = nchw(inp.x).to(dtype).contiguous().requires_grad_(kind != "stem")
    if kind == "block":
        out = mod(x, None if inp.masks is None else tuple(None if m is None else m.to(dtype) for m in inp.masks))
    elif kind == "tail":
        out = mod(x, inp.u)
    else:
        out = mod(x)
    out.backward(nchw(inp.g).to(out.dtype).contiguous())
    res = {"out": out, **({"x.grad": x.grad} if kind != "stem" else {}), **{name: p.grad for name, p in mod.named_parameters()}}
    return {name: t.detach().double() for name, t in res.items()}


def sibling(name: str) -> str:
    return name[:-4] + "weight"


def expected_zeros(case: Case, names) -> set[str]:
    """The structurally zero gradients among `names`, from the arithmetic (see the module docstring)."""
    ends = ("k.conv.bias", "k.bn.bias", "talking_head1.bias")
    if case.train:
        ends += (".conv.bias", "stride_conv.bn.bias", "q.local.bias")
    return {n for n in names if n.endswith(ends)}


def exact_zeros(case: Case, names) -> set[str]:
    """Those the engine must leave exactly zero: a convolution bias in front of a batch-statistics BatchNorm."""
    return {n for n in names if case.train and n.endswith(".conv.bias")}


@functools.lru_cache(maxsize=None)
def reference(case: Case):
    """(float64 tensors, yardstick, structural zeros): out, x.grad and every parameter gradient of the oracle sub-module in
    float64; per tensor the relative L2 error against them of the same sub-module with f32 parameters under CPU bf16 autocast
    on a contiguous NCHW input (for a structural zero: its sibling weight's); and the names that are structurally zero."""
    inp = inputs(case)
    ref = _oracle_pass(copy.deepcopy(inp.mod).double(), inp, torch.float64)
    with torch.autocast("cpu", dtype=BF):
        auto = _oracle_pass(copy.deepcopy(inp.mod), inp, torch.float32)
    zeros = frozenset(n for n in ref if n.endswith("bias") and sibling(n) in ref
                      and float(ref[n].abs().max()) < ZERO * float(ref[sibling(n)].abs().max()))
    yard = {n: rel_l2(auto[n], ref[n]) for n in ref if n not in zeros}
    yard.update({n: yard[sibling(n)] for n in zeros})
    return ref, yard, zeros


# ---------------------------------------------------------------------------------------------------------------- the engine
class FakeRng:
    """Stands in for kernels.DeviceRng in HipBlock.forward: hands back the case's row scale of the branch asked for."""

    def __init__(self, inp: Inputs, index: int) -> None:
        self.inp, self.index, self.calls = inp, index, []

    def drop_path_scale(self, n, keep, stream_id):
        which = stream_id - 2 * self.index
        assert n == self.inp.case.n and abs(keep - KEEP) < 1e-12 and which in (0, 1), (n, keep, stream_id, self.index)
        assert self.inp.masks[which] is not None, "a block without a token mixer asked for the token mixer's scale"
        self.calls.append(which)
        return self.inp.masks[which].cuda()


class HipTail(torch.nn.Module):
    """The tail as HipEfficientFormerV2._forward runs it, on the network's own norm, head and head_dist."""

    def __init__(self, net) -> None:
        super().__init__()
        self.norm, self.head, self.head_dist = net.norm, net.head, net.head_dist

    def forward(self, x, u=None):
        from deepfakedetection_amd.network import _bnref
        from deepfakedetection_amd.vit_functions import TailCtx, TailFunction

        cfg = TailCtx(_bnref(self.norm), P_DROP if u is not None else 0.0, self.training, None)
        return TailFunction.apply(x, self.norm.weight, self.norm.bias, self.head.weight, self.head.bias, self.head_dist.weight,
                                  self.head_dist.bias, u, cfg)


def _run_stem(stem, xh: torch.Tensor, dt: torch.dtype) -> torch.Tensor:
    """HipEfficientFormerV2.forward_features_nhwc's two stem stages on the f32 NHWC image."""
    from deepfakedetection_amd._lib import ACT_GELU
    from deepfakedetection_amd.network import _bnref
    from deepfakedetection_amd.vit_functions import ConvStemCtx, ConvStemFunction, DenseConvBNFunction, DenseConvCtx

    c1, c2, tr = stem.conv1, stem.conv2, stem.training
    h = ConvStemFunction.apply(xh, *c1.tensors(), ConvStemCtx(2, 1, _bnref(c1.bn), dt, tr, ACT_GELU, None))
    return DenseConvBNFunction.apply(h, *c2.tensors(), DenseConvCtx(3, 2, _bnref(c2.bn), tr, ACT_GELU, None))


def hip_module(case: Case):
    """The HIP sub-module of the case on the device, with the oracle sub-module's state."""
    mod = copy.deepcopy(_sub(hip_net(case.variant), case, HipTail))
    mod.load_state_dict(inputs(case).mod.state_dict(), strict=True)
    if case.scaled and case.kind == "block":
        mod.drop_path = 1.0 - KEEP
    return mod.cuda().train(case.train)


def engine(hmod, inp: Inputs, dtype: torch.dtype = BF) -> dict[str, torch.Tensor]:
    """out, x.grad and every parameter gradient of one forward and backward of the HIP sub-module, as the device left them
    (NHWC); errors() converts."""
    kind = inp.case.kind
    for p in hmod.parameters():
        p.grad = None
    x = inp.x.to(torch.float32 if kind == "stem" else dtype).cuda().requires_grad_(kind != "stem")
    if kind == "block":
        rng = FakeRng(inp, hmod.index) if inp.masks is not None else None
        out = hmod(x, rng)
        if rng is not None:
            assert rng.calls == ([0, 1] if inp.masks[0] is not None else [1]), rng.calls
    elif kind == "tail":
        out = hmod(x, None if inp.u is None else inp.u.cuda())
    else:
        out = hmod(x) if kind == "downsample" else _run_stem(hmod, x, dtype)
    out.backward(inp.g.to(out.dtype).cuda())
    torch.cuda.synchronize()
    res = {"out": out, **({"x.grad": x.grad} if kind != "stem" else {}), **{name: p.grad for name, p in hmod.named_parameters()}}
    missing = [name for name, t in res.items() if t is None]
    assert not missing, f"no gradient for {missing}"
    return {name: t.detach().clone() for name, t in res.items()}


def errors(got: dict, ref: dict, zeros=frozenset()) -> dict[str, float]:
    """Per tensor ||got - ref|| / ||ref||; for a structural zero ||got|| / ||ref[sibling]||."""
    assert set(got) == set(ref), set(got) ^ set(ref)
    errs = {}
    for name, want in ref.items():
        have = got[name]
        assert bool(torch.isfinite(have).all()), name
        have = nchw(have) if name in ("out", "x.grad") else have
        assert tuple(have.shape) == tuple(want.shape), (name, tuple(have.shape), tuple(want.shape))
        if name in zeros:
            errs[name] = float(have.double().norm().cpu() / ref[sibling(name)].norm())
        else:
            errs[name] = rel_l2(have, want)
    return errs


def ratio(err: float, yard: float) -> float:
    """The factor a tensor needs in `err <= factor * yardstick + FLOOR`."""
    return max(err - FLOOR, 0.0) / max(yard, 1e-300)


def table(errs: dict[str, float], yard: dict[str, float], zeros=frozenset()) -> str:
    rows = [f"  {errs[n]:.3e}  yardstick {yard[n]:.3e}  ratio {ratio(errs[n], yard[n]):5.2f}  {n}" + ("  (structural zero, on its sibling's scale)" if n in zeros else "")
            for n in errs]
    return "relative L2 error against float64, per tensor:\n" + "\n".join(rows)
