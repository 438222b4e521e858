"""One MBConv block on fixed inputs, three ways: the oracle block in float64 (the reference), the oracle block under CPU bf16
autocast (the yardstick: what bf16 rounding alone costs each tensor) and the HIP block (the engine).  For
tests/test_mbconv_bwd_bf16_gpu.py.

The inputs follow tests/test_fullsize_gpu._pair / _block_in_bf16 (same network seeds, same generator seed per block, BatchNorm
affine parameters randomised); on top of that the running statistics are randomised (they matter in eval mode) and the 1x1
convolution weights without bias — expand and project — are rounded to bf16-representable values, as kernels.prep_weights rounds
them in the engine, so that weight rounding stays out of the comparison.  The reference and the yardstick need no GPU.
"""

from __future__ import annotations

import copy
import functools
from dataclasses import dataclass

import torch

from tests._grad_signal import rel_l2

BF = torch.bfloat16
NETS = {"b0": ("timm", 21), "b3": ("lukemelas", 22)}            # variant -> flavour, seed of the test_fullsize_gpu block tests
FLOOR = 2e-3                                                     # test_ops_gpu.test_rowpass's tolerance of the f32 BatchNorm-backward sums
ACTIVATIONS = ("out", "x.grad")                                  # NHWC in the engine, NCHW in the oracle


@dataclass(frozen=True)
class Case:
    variant: str
    index: int
    n: int
    res: int
    train: bool = True
    scaled: bool = False                                         # a drop-connect row scale in {0, 1 / 0.8} is handed in

    @property
    def id(self) -> str:
        return f"{self.variant}_block{self.index}_{self.n}x{self.res}" + ("" if self.train else "_eval") + ("_row_scale" if self.scaled else "")


@dataclass
class Inputs:
    case: Case
    blk: torch.nn.Module                                         # the oracle block, f32, randomised, in the case's mode
    x: torch.Tensor                                              # [N, H, W, Cin] bf16
    g: torch.Tensor                                              # [N, Ho, Wo, Cout] bf16
    row_scale: torch.Tensor | None                               # [N] f32

    @property
    def skip(self) -> bool:
        c = self.blk.c
        return c.stride == 1 and c.cin == c.cout

    @property
    def cmid(self) -> int:
        return self.blk.c.cin * self.blk.c.expand


@functools.lru_cache(maxsize=None)
def oracle_net(variant: str):
    from oracle.effnet_ref import EfficientNetRef

    flavour, seed = NETS[variant]
    torch.manual_seed(seed)
    return EfficientNetRef(variant, flavour, 2)


@functools.lru_cache(maxsize=None)
def hip_net(variant: str):
    from deepfakedetection_amd.efficientnet import HipEfficientNet

    return HipEfficientNet(variant, NETS[variant][0], 2)


@functools.lru_cache(maxsize=None)
def inputs(case: Case) -> Inputs:
    blk = copy.deepcopy(oracle_net(case.variant).block_list()[case.index])
    c = blk.c
    g = torch.Generator().manual_seed(100 + case.index)
    x = torch.randn(case.n, case.res, case.res, c.cin, generator=g).to(BF)
    with torch.no_grad():
        for name, p in blk.named_parameters():
            if ".bn" in name or name.startswith("bn") or name.startswith("_bn"):
                p.copy_(0.6 + 0.8 * torch.rand(p.shape, generator=g) if name.endswith("weight") else torch.randn(p.shape, generator=g) * 0.2)
        for m in blk.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g))
            elif isinstance(m, torch.nn.Conv2d) and m.kernel_size == (1, 1) and m.bias is None:
                m.weight.copy_(m.weight.to(BF).float())
    left, right, top, bottom = c.pad_dw
    ho = (case.res + top + bottom - c.k) // c.stride + 1
    wo = (case.res + left + right - c.k) // c.stride + 1
    gout = torch.randn(case.n, ho, wo, c.cout, generator=g).to(BF)
    inp = Inputs(case, blk.train(case.train), x, gout, None)
    if case.scaled:
        assert inp.skip, "only a block with a skip connection takes a row scale"
        keep = torch.rand(case.n, generator=g) < 0.8
        keep[0], keep[1] = False, True                           # both values occur at every batch size
        inp.row_scale = keep.float() / 0.8
    return inp


def nchw(t: torch.Tensor) -> torch.Tensor:
    return t.permute(0, 3, 1, 2)


def _oracle_pass(blk, inp: Inputs, dtype: torch.dtype) -> dict[str, torch.Tensor]:
    """Forward and backward of (a copy of) the oracle block on contiguous NCHW inputs of `dtype`; everything in float64."""
    x = nchw(inp.x).to(dtype).contiguous().requires_grad_(True)
    mask = inp.row_scale.to(dtype).view(-1, 1, 1, 1) if inp.row_scale is not None else None
    if mask is None:
        out = blk(x)
    elif hasattr(blk, "_depthwise_conv"):
        out = blk(x, mask)
    else:                                                        # _BlockTimm.forward ignores its drop mask
        out = (blk(x) - x) * mask + x
    out.backward(nchw(inp.g).to(out.dtype).contiguous())
    res = {"out": out, "x.grad": x.grad, **{name: p.grad for name, p in blk.named_parameters()}}
    return {name: t.detach().double() for name, t in res.items()}


@functools.lru_cache(maxsize=None)
def reference(case: Case):
    """(float64 tensors, yardstick): out, x.grad and every parameter gradient of the oracle block in float64, and per tensor the
    relative L2 error against them of the same block with f32 parameters under CPU bf16 autocast on a contiguous NCHW input."""
    inp = inputs(case)
    ref = _oracle_pass(copy.deepcopy(inp.blk).double(), inp, torch.float64)
    with torch.autocast("cpu", dtype=BF):
        auto = _oracle_pass(copy.deepcopy(inp.blk), inp, torch.float32)
    return ref, {name: rel_l2(auto[name], ref[name]) for name in ref}


def hip_block(case: Case):
    """The HIP block of the case on the device, with the oracle block's state."""
    blk = copy.deepcopy(hip_net(case.variant).block_list()[case.index])
    blk.load_state_dict(inputs(case).blk.state_dict())
    return blk.cuda().train(case.train)


def engine(hblk, inp: Inputs, dtype: torch.dtype = BF, frozen=()) -> dict[str, torch.Tensor | None]:
    """out, x.grad and every parameter gradient of one forward and backward of the HIP block; `frozen`: names (or "x") that
    do not require a gradient, their entry is what autograd left in .grad."""
    x = inp.x.to(dtype).cuda().requires_grad_("x" not in frozen)
    for name, p in hblk.named_parameters():
        p.requires_grad_(name not in frozen)
        p.grad = None
    row_scale = inp.row_scale.cuda() if inp.row_scale is not None else None
    out = hblk.run(x, row_scale, None, None)
    out.backward(inp.g.to(dtype).cuda())
    torch.cuda.synchronize()
    res = {"out": out, "x.grad": x.grad, **{name: p.grad for name, p in hblk.named_parameters()}}
    for p in hblk.parameters():
        p.requires_grad_(True)
    return {name: None if t is None else t.detach().clone() for name, t in res.items()}


def errors(got: dict, ref: dict) -> dict[str, float]:
    assert set(got) == set(ref), set(got) ^ set(ref)
    errs = {}
    for name, want in ref.items():
        have = got[name]
        assert have is not None and bool(torch.isfinite(have).all()), name
        have = nchw(have) if name in ACTIVATIONS else have
        assert tuple(have.shape) == tuple(want.shape), (name, tuple(have.shape), tuple(want.shape))
        errs[name] = rel_l2(have, want)
    return errs


def ratio(err: float, yard: float) -> float:
    """The factor a tensor needs in `err <= factor * yardstick + FLOOR`."""
    return max(err - FLOOR, 0.0) / max(yard, 1e-300)


def table(errs: dict[str, float], yard: dict[str, float]) -> str:
    rows = [f"  {errs[n]:.3e}  yardstick {yard[n]:.3e}  ratio {ratio(errs[n], yard[n]):5.2f}  {n}" for n in errs]
    return "relative L2 error against float64, per tensor:\n" + "\n".join(rows)
