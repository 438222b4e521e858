"""One FasterViT stage on fixed inputs, three ways: the oracle sub-module in float64 (the reference), the same sub-module with
f32 parameters under CPU bf16 autocast (the yardstick: what bf16 rounding alone costs each tensor) and the HIP sub-module (the
engine).  For tests/test_fastervit_bf16_gpu.py; tests/test_fastervit_bf16_ref_cpu.py checks the reference on its own.

The vocabulary is tests/_efformer_bwd_ref.py's (and through it tests/_mbconv_bwd_ref.py's).  A case names a sub-module of
oracle.fastervit_ref.FasterViTRef:
  hat         levels[level].blocks[1].  Level 2: x [4 B, 49, C] window tokens and ct [B, 16, C] carrier tokens, two outputs and
              two input gradients (`out.x`, `out.ct`, `x.grad`, `ct.grad`); the oracle keeps the carrier tokens window-major and
              the engine row-major, so the reference converts with ct_window / ct_dewindow as test_fastervit_gpu._hat_block does
              and every tensor here is in the engine's order.  Level 3: x [B, 49, C] alone (`out`, `x.grad`).
  conv        levels[level].blocks[-1], a ConvBlock, in training or eval mode (gradients in both)
  downsample  levels[level].downsample: LayerNorm2d + conv3x3 s2
  tokens      levels[2].global_tokenizer: dw3x3 + AvgPool(5, 3) -> [B, 16, C] carrier tokens, row-major
  stem        patch_embed on a [N, 224, 224, 3] image; the engine takes no gradient for the image, so there is no `x.grad`
  tail        norm -> mean(H, W) -> head (TailFunction without head_dist)
The sub-module is randomised with test_fastervit_gpu.randomise under a seed derived from the case id; the qkv / proj / fc1 / fc2
Linear weights are then rounded to bf16-representable values, as kernels.prep_weights rounds them in the engine, so that weight
rounding stays out of the comparison.  x, ct and the output gradients hold bf16-representable values.  Maps are kept NHWC (the
engine's layout) here; the oracle sees contiguous NCHW copies.

`scaled` cases carry DropPath row scales, written down below and not drawn: window_scale per window for the window stream of a
HAT block, image_scale per image for its carrier stream and for a ConvBlock; dropped entries (0.0: at least indices 1 and n - 1)
and kept ones (1 / 0.8).  The oracle takes them through HAT.forward(x, ct, (m_ct, m_win)) / ConvBlock.forward(x, mask); the engine
through forward(..., rng=fake) with drop_path = 0.2, where the fake generator asserts keep == 0.8, the row count and the stream
id (4 * index for the window stream and the ConvBlock, 4 * index + 1 for the carrier stream) and records the call order.

Structural zeros.  A tensor is structurally zero when its float64 gradient's largest entry is below 1e-9 of its sibling
weight's.  expected_zeros() names them from the arithmetic:
  * a ConvBlock in training mode: `conv1.bias`, `conv2.bias` (the batch mean of the BatchNorm behind it absorbs them); the engine
    must leave them exactly zero (exact_zeros());
  * a HAT block: the k third of every `qkv.bias` (it shifts all keys of a softmax row equally).
They are not left out: their error is ||got|| / ||ref[sibling]|| and their yardstick is the sibling's.  So that the k third can be
judged at all, and so that a wrong k or v third cannot hide behind the other two, `qkv.weight` and `qkv.bias` are cut into their
q, k and v thirds (`attn.qkv.weight[q]`, ...), three tensors each; the sibling of `qkv.bias[k]` is `qkv.weight[k]`.
"""

from __future__ import annotations

import copy
import functools
import re
import zlib
from dataclasses import dataclass
from pathlib import Path

import torch
import torch.nn.functional as F

from tests._efformer_bwd_ref import BF, FLOOR, KEEP, ZERO, ratio, table          # noqa: F401  (shared vocabulary, re-exported)
from tests._grad_signal import rel_l2

NC = 2
RES = (56, 28, 14, 7)
WINDOW, SEQ_CT = 49, 16


@dataclass(frozen=True)
class Case:
    variant: str
    kind: str                                                    # hat | conv | downsample | tokens | stem | tail
    level: int
    n: int                                                       # images
    scaled: bool = False                                         # DropPath row scales (hat, conv)
    train: bool = True

    @property
    def id(self) -> str:
        what = self.kind + (str(self.level) if self.kind in ("hat", "conv", "downsample") else "")
        return f"fv{self.variant}-{what}-b{self.n}" + ("" if self.train else "-eval") + ("-scaled" if self.scaled else "")

    @property
    def seed(self) -> int:
        return zlib.crc32(self.id.encode()) % (1 << 31)

    @property
    def windows(self) -> int:
        """Windows of a hat case: 4 per image at level 2 (14 px), 1 at level 3."""
        return self.n * (4 if self.level == 2 else 1)


def _conv_cases(variant: str, level: int) -> list[Case]:
    return [Case(variant, "conv", level, 3), Case(variant, "conv", level, 3, scaled=True), Case(variant, "conv", level, 3, train=False)]


def conv3_tile_width() -> int:
    """C3_TW of csrc/dfd_conv3.hip: the width in pixels of the direct 3x3 kernel's output tile."""
    src = (Path(__file__).resolve().parents[1] / "deepfakedetection_amd" / "csrc" / "dfd_conv3.hip").read_text()
    return int(re.search(r"^#define\s+C3_TW\s+(\d+)", src, re.M).group(1))


def conv3_direct_grid(n: int, res: int, c: int) -> tuple[int, int] | None:
    """(work items, persistent grid) of dfd_conv3_direct for a C -> C 3x3 convolution of n res x res maps, None where the shape
    is not the direct kernel's (dfd_conv3.hip: C in {64, 96, 128} and Cout % 64 == 0; 7-row tiles where 7 divides the height
    and 8 does not, else 8-row tiles; 512 / (Cout / 64) workgroups)."""
    if c not in (64, 96, 128) or c % 64:
        return None
    th = 7 if (res % 8 and res % 7 == 0) else 8
    tw = conv3_tile_width()
    return n * ((res + th - 1) // th) * ((res + tw - 1) // tw), 512 // (c // 64)


def conv_implicit_parts(n: int, res: int, c: int) -> int:
    """Partial rows of the implicit-GEMM 3x3 convolution with statistics (dfd_pwconv.hip, conv_nt_launch)."""
    m = n * res * res
    bm = 64 if ((m + 127) // 128) * ((c + 127) // 128) < 256 else 128
    n_tiles = (c + (64 if c <= 64 else 128) - 1) // (64 if c <= 64 else 128)
    return min(max(2048 // n_tiles, 32), 1024, (m + bm - 1) // bm)


def _first_past_grid(res: int, c: int) -> int:
    """The smallest batch at which dfd_conv3_direct has more work items than workgroups: some workgroup walks a second tile and
    the last round is partial."""
    n = 1
    while conv3_direct_grid(n, res, c)[0] <= conv3_direct_grid(n, res, c)[1]:
        n += 1
    return n


B_PAST_GRID = {0: _first_past_grid(56, 64), 1: _first_past_grid(28, 128)}        # 19 (28 tiles per image, 512 workgroups), 33 (8, 256)

# the cases of tests/test_fastervit_bf16_gpu.py, each the smallest at which the path named still runs (its docstring has the tiers)
HAT2 = [Case("0", "hat", 2, 3), Case("0", "hat", 2, 3, scaled=True), Case("0", "hat", 2, 33, scaled=True),
        Case("0", "hat", 2, 97, scaled=True), Case("0", "hat", 2, 97),
        Case("1", "hat", 2, 33, scaled=True), Case("2", "hat", 2, 3),
        Case("3", "hat", 2, 3, scaled=True), Case("3", "hat", 2, 48, scaled=True), Case("3", "hat", 2, 47, scaled=True)]
HAT3 = [Case("0", "hat", 3, 3), Case("0", "hat", 3, 37, scaled=True), Case("0", "hat", 3, 68, scaled=True)]
CONV = (_conv_cases("0", 0) + _conv_cases("0", 1) + _conv_cases("2", 0) + _conv_cases("1", 0) + _conv_cases("3", 1)
        + [Case("0", "conv", 0, B_PAST_GRID[0], scaled=True), Case("0", "conv", 1, B_PAST_GRID[1], scaled=True)])
DOWNSAMPLE = [Case("0", "downsample", lv, n) for lv in (0, 1, 2) for n in (3, 5)]
TOKENS = [Case("0", "tokens", 2, 2), Case("0", "tokens", 2, 33)]
STEM = [Case("0", "stem", 0, 4), Case("1", "stem", 0, 4)]
TAIL = [Case("0", "tail", 3, 37)]
CASES = HAT2 + HAT3 + CONV + DOWNSAMPLE + TOKENS + STEM + TAIL


def window_scale(n: int) -> torch.Tensor:
    """The window stream's row scale: windows 1, n - 1 and every i with i % 7 == 2 are dropped."""
    return torch.tensor([0.0 if i in (1, n - 1) or i % 7 == 2 else 1.0 / KEEP for i in range(n)])


def image_scale(n: int) -> torch.Tensor:
    """The carrier stream's and the ConvBlock's row scale: images 1, n - 1 and every i with i % 5 == 3 are dropped."""
    return torch.tensor([0.0 if i in (1, n - 1) or i % 5 == 3 else 1.0 / KEEP for i in range(n)])


class Tail(torch.nn.Module):
    """norm -> mean(H, W) -> head on the network's own norm and head (FasterViTRef.forward behind the levels)."""

    def __init__(self, net) -> None:
        super().__init__()
        self.norm, self.head = net.norm, net.head

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        n = self.norm
        x = F.batch_norm(x, n.running_mean, n.running_var, n.weight, n.bias, self.training, n.momentum, n.eps).mean(dim=(2, 3))
        return F.linear(x, self.head.weight, self.head.bias)


@dataclass
class Inputs:
    case: Case
    mod: torch.nn.Module                                         # the oracle sub-module, f32, randomised, in the case's mode
    x: torch.Tensor                                              # f32 holding bf16 values: [nW, 49, C] (hat) or NHWC
    ct: torch.Tensor | None                                      # [B, 16, C] row-major carrier tokens of a level-2 hat case
    g: dict                                                      # output name -> its gradient, in the engine's order
    masks: tuple | None                                          # hat: (carrier or None, window); conv: (images,)

    @property
    def carrier(self) -> bool:
        return self.ct is not None


@functools.lru_cache(maxsize=None)
def oracle_net(variant: str):
    from oracle.fastervit_ref import FasterViTRef

    torch.manual_seed(31)
    return FasterViTRef(variant, NC, 224, drop_path_rate=0.0)


@functools.lru_cache(maxsize=None)
def hip_net(variant: str):
    from deepfakedetection_amd.fastervit import HipFasterViT

    return HipFasterViT(variant, NC, 224, drop_path_rate=0.0)


def _sub(net, case: Case, tail_cls):
    level = net.levels[case.level]
    return {"hat": lambda: level.blocks[1], "conv": lambda: level.blocks[-1], "downsample": lambda: level.downsample,
            "tokens": lambda: level.global_tokenizer, "stem": lambda: net.patch_embed, "tail": lambda: tail_cls(net)}[case.kind]()


def dim(case: Case) -> int:
    from oracle.fastervit_ref import CONFIGS

    return CONFIGS[case.variant][2] << case.level


@functools.lru_cache(maxsize=None)
def inputs(case: Case) -> Inputs:
    from tests.test_fastervit_gpu import randomise

    mod = copy.deepcopy(_sub(oracle_net(case.variant), case, Tail))
    holder = torch.nn.Module()                                   # randomise() goes by the names inside the network
    holder.add_module("patch_embed" if case.kind == "stem" else "sub", mod)
    randomise(holder, case.seed)
    with torch.no_grad():
        for name, m in mod.named_modules():
            if isinstance(m, torch.nn.Linear) and name.rsplit(".", 1)[-1] in ("qkv", "proj", "fc1", "fc2"):
                m.weight.copy_(m.weight.to(BF).float())
    c, n, r = dim(case), case.n, RES[case.level]
    xs, gs = {"hat": lambda: ((case.windows, WINDOW, c), {"out.x" if case.level == 2 else "out": (case.windows, WINDOW, c)}),
              "conv": lambda: ((n, r, r, c), {"out": (n, r, r, c)}),
              "downsample": lambda: ((n, r, r, c), {"out": (n, r // 2, r // 2, 2 * c)}),
              "tokens": lambda: ((n, r, r, c), {"out": (n, SEQ_CT, c)}),
              "stem": lambda: ((n, 224, 224, 3), {"out": (n, 56, 56, c)}),
              "tail": lambda: ((n, 7, 7, c), {"out": (n, NC)})}[case.kind]()
    gen = torch.Generator().manual_seed(case.seed + 1)
    x = torch.randn(xs, generator=gen).to(BF).float()
    ct = None
    if case.kind == "hat" and case.level == 2:
        ct = torch.randn((n, SEQ_CT, c), generator=gen).to(BF).float()
        gs["out.ct"] = (n, SEQ_CT, c)
    g = {name: torch.randn(shape, generator=gen).to(BF).float() for name, shape in gs.items()}
    masks = None
    if case.scaled:
        assert case.train and case.kind in ("hat", "conv")
        mod.dp = 1.0 - KEEP
        masks = (image_scale(n) if ct is not None else None, window_scale(case.windows)) if case.kind == "hat" else (image_scale(n),)
    return Inputs(case, mod.train(case.train), x, ct, g, masks)


def nchw(t: torch.Tensor) -> torch.Tensor:
    return t.permute(0, 3, 1, 2)


def nhwc(t: torch.Tensor) -> torch.Tensor:
    return t.permute(0, 2, 3, 1)


def cut_qkv(res: dict) -> dict:
    """`*.qkv.weight` and `*.qkv.bias` as their q, k and v thirds, three tensors each; everything else as it is."""
    out = {}
    for name, t in res.items():
        if name.endswith(("qkv.weight", "qkv.bias")):
            c = t.shape[0] // 3
            out.update({f"{name}[{part}]": t[i * c:(i + 1) * c] for i, part in enumerate("qkv")})
        else:
            out[name] = t
    return out


def _oracle_pass(mod, inp: Inputs, dtype: torch.dtype) -> dict[str, torch.Tensor]:
    """Forward and backward of (a copy of) the oracle sub-module on contiguous inputs of `dtype` in the oracle's layout; the
    results in float64 and in the engine's order."""
    from oracle.fastervit_ref import ct_dewindow, ct_window

    kind, n = inp.case.kind, inp.case.n
    masks = None if inp.masks is None else tuple(None if m is None else m.to(dtype) for m in inp.masks)
    if kind == "hat":
        x = inp.x.to(dtype).clone().requires_grad_()
        ct = inp.ct.to(dtype).clone().requires_grad_() if inp.carrier else None
        ct_in = ct_window(ct, 4, 4, 2).reshape(n, SEQ_CT, -1) if inp.carrier else None       # the package's window-major storage
        ox, oc = mod(x, ct_in, masks)
        if inp.carrier:
            oc = ct_dewindow(oc, 4, 4, 2)
            torch.autograd.backward([ox, oc], [inp.g["out.x"].to(ox.dtype), inp.g["out.ct"].to(oc.dtype)])
            res = {"out.x": ox, "out.ct": oc, "x.grad": x.grad, "ct.grad": ct.grad}
        else:
            ox.backward(inp.g["out"].to(ox.dtype))
            res = {"out": ox, "x.grad": x.grad}
    else:
        x = nchw(inp.x).to(dtype).contiguous().requires_grad_(kind != "stem")
        out = mod(x, masks[0]) if masks is not None else mod(x)
        if kind == "tokens":
            out = ct_dewindow(out, 4, 4, 2)                      # row-major, the order the engine keeps carrier tokens in
        g = inp.g["out"].to(out.dtype)
        out.backward(nchw(g).contiguous() if out.dim() == 4 else g)
        res = {"out": nhwc(out) if out.dim() == 4 else out, **({"x.grad": nhwc(x.grad)} if kind != "stem" else {})}
    res.update({name: p.grad for name, p in mod.named_parameters()})
    return cut_qkv({name: t.detach().double().contiguous() for name, t in res.items()})


def sibling(name: str) -> str:
    """`*.bias` -> `*.weight`, `*.bias[k]` -> `*.weight[k]`."""
    return name[:-7] + "weight" + name[-3:] if name.endswith("]") else name[:-4] + "weight"


def _is_bias(name: str) -> bool:
    return name.endswith("bias") or name[:-3].endswith("bias") and name.endswith("]")


def expected_zeros(case: Case, names) -> set[str]:
    """The structurally zero gradients among `names`, from the arithmetic (see the module docstring)."""
    if case.kind == "hat":
        return {n for n in names if n.endswith("qkv.bias[k]")}
    if case.kind == "conv" and case.train:
        return {n for n in names if n in ("conv1.bias", "conv2.bias")}
    return set()


def exact_zeros(case: Case, names) -> set[str]:
    """Those the engine must leave exactly zero: a convolution bias in front of a batch-statistics BatchNorm."""
    return {n for n in names if case.kind == "conv" and case.train and n in ("conv1.bias", "conv2.bias")}


OUTPUTS = ("out", "out.x", "out.ct", "x.grad", "ct.grad")


@functools.lru_cache(maxsize=None)
def reference(case: Case):
    """(float64 tensors, yardstick, structural zeros): the outputs, the input gradients and every parameter gradient of the
    oracle sub-module in float64; per tensor the relative L2 error against them of the same sub-module with f32 parameters under
    CPU bf16 autocast on contiguous inputs (for a structural zero: its sibling weight's); and the names that are structurally
    zero."""
    inp = inputs(case)
    ref = _oracle_pass(copy.deepcopy(inp.mod).double(), inp, torch.float64)
    with torch.autocast("cpu", dtype=BF):
        auto = _oracle_pass(copy.deepcopy(inp.mod), inp, torch.float32)
    zeros = frozenset(n for n in ref if _is_bias(n) and sibling(n) in ref
                      and float(ref[n].abs().max()) < ZERO * float(ref[sibling(n)].abs().max()))
    yard = {n: rel_l2(auto[n], ref[n]) for n in ref if n not in zeros}
    yard.update({n: yard[sibling(n)] for n in zeros})
    return ref, yard, zeros


# ---------------------------------------------------------------------------------------------------------------- the engine
class FakeRng:
    """Stands in for kernels.DeviceRng in HipHAT.forward / HipConvBlock.forward: hands back the case's row scale of the stream
    asked for (0: the window stream or the ConvBlock, 1: the carrier stream) and records the order of the calls."""

    def __init__(self, inp: Inputs, index: int) -> None:
        self.inp, self.index, self.calls = inp, index, []

    def drop_path_scale(self, n, keep, stream_id):
        case, which = self.inp.case, stream_id - 4 * self.index
        assert abs(keep - KEEP) < 1e-12 and which in (0, 1), (n, keep, stream_id, self.index)
        if case.kind == "conv":
            assert which == 0 and n == case.n, (n, stream_id, self.index)
            scale = self.inp.masks[0]
        elif which == 0:
            assert n == case.windows, f"window stream (id 4 * index): {n} rows, not the {case.windows} windows"
            scale = self.inp.masks[1]
        else:
            assert self.inp.carrier and n == case.n, f"carrier stream (id 4 * index + 1): {n} rows, not the {case.n} images"
            scale = self.inp.masks[0]
        self.calls.append(which)
        return scale.cuda()

    @property
    def expected_calls(self) -> list[int]:
        return [0, 1] if self.inp.carrier else [0]


class HipTail(torch.nn.Module):
    """The tail as HipFasterViT._forward runs it, on the network's own norm and head."""

    def __init__(self, net) -> None:
        super().__init__()
        self.norm, self.head = net.norm, net.head

    def forward(self, x):
        from deepfakedetection_amd.network import _bnref
        from deepfakedetection_amd.vit_functions import TailCtx, TailFunction

        cfg = TailCtx(_bnref(self.norm), 0.0, self.training, None)
        return TailFunction.apply(x, self.norm.weight, self.norm.bias, self.head.weight, self.head.bias, None, None, None, cfg)


def _run_stem(stem, xh: torch.Tensor, dt: torch.dtype) -> torch.Tensor:
    """HipFasterViT._forward's two patch-embed stages on the f32 NHWC image."""
    from deepfakedetection_amd._lib import ACT_RELU
    from deepfakedetection_amd.network import _bnref
    from deepfakedetection_amd.vit_functions import ConvStemCtx, ConvStemFunction, DenseConvBNFunction, DenseConvCtx

    c, tr = stem.conv_down, stem.training
    h = ConvStemFunction.apply(xh, c[0].weight, None, c[1].weight, c[1].bias, ConvStemCtx(2, 1, _bnref(c[1]), dt, tr, ACT_RELU, None))
    return DenseConvBNFunction.apply(h, c[3].weight, None, c[4].weight, c[4].bias, DenseConvCtx(3, 2, _bnref(c[4]), tr, ACT_RELU, None))


def hip_module(case: Case):
    """The HIP sub-module of the case on the device, with the oracle sub-module's state."""
    mod = copy.deepcopy(_sub(hip_net(case.variant), case, HipTail))
    mod.load_state_dict(inputs(case).mod.state_dict(), strict=True)
    if case.scaled:
        mod.drop_path = 1.0 - KEEP
    return mod.cuda().train(case.train)


def engine(hmod, inp: Inputs, dtype: torch.dtype = BF, after_forward=None) -> dict[str, torch.Tensor]:
    """The outputs, the input gradients and every parameter gradient of one forward and backward of the HIP sub-module, as the
    device left them, qkv cut into thirds.  after_forward: called between the two passes (the spies' forward counts)."""
    from deepfakedetection_amd.fastervit import _window_maps

    case, kind = inp.case, inp.case.kind
    for p in hmod.parameters():
        p.grad = None
    rng = FakeRng(inp, hmod.index) if inp.masks is not None else None
    dev = torch.device("cuda")
    if kind == "hat":
        c = inp.x.shape[-1]
        x = inp.x.to(dtype).cuda().view(case.windows, WINDOW, 1, c).requires_grad_()
        ct = inp.ct.to(dtype).cuda().view(case.n, SEQ_CT, 1, c).requires_grad_() if inp.carrier else None
        hx, hc = hmod(x, ct, _window_maps(case.n, 14, dev)[1:] if inp.carrier else None, rng)
        if after_forward is not None:
            after_forward()
        if inp.carrier:
            torch.autograd.backward([hx, hc], [inp.g["out.x"].to(hx.dtype).cuda().view(hx.shape), inp.g["out.ct"].to(hc.dtype).cuda().view(hc.shape)])
            res = {"out.x": hx, "out.ct": hc, "x.grad": x.grad, "ct.grad": ct.grad}
        else:
            assert hc is None
            hx.backward(inp.g["out"].to(hx.dtype).cuda().view(hx.shape))
            res = {"out": hx, "x.grad": x.grad}
    else:
        x = inp.x.to(torch.float32 if kind == "stem" else dtype).cuda().requires_grad_(kind != "stem")
        out = hmod(x, rng) if kind == "conv" else _run_stem(hmod, x, dtype) if kind == "stem" else hmod(x)
        if after_forward is not None:
            after_forward()
        out.backward(inp.g["out"].to(out.dtype).cuda().view(out.shape))
        res = {"out": out, **({"x.grad": x.grad} if kind != "stem" else {})}
    torch.cuda.synchronize()
    if rng is not None:
        assert rng.calls == rng.expected_calls, rng.calls
    res.update({name: p.grad for name, p in hmod.named_parameters()})
    missing = [name for name, t in res.items() if t is None]
    assert not missing, f"no gradient for {missing}"
    return cut_qkv({name: t.detach().clone() for name, t in res.items()})


def errors(got: dict, ref: dict, zeros=frozenset()) -> dict[str, float]:
    """Per tensor ||got - ref|| / ||ref||; for a structural zero ||got|| / ||ref[sibling]||.  Both sides are in the engine's
    order; the engine's token tensors carry a dummy axis ([n, T, 1, C]) the reference's do not."""
    assert set(got) == set(ref), set(got) ^ set(ref)
    errs = {}
    for name, want in ref.items():
        have = got[name]
        assert bool(torch.isfinite(have).all()), name
        assert have.numel() == want.numel() and tuple(d for d in have.shape if d != 1) == tuple(d for d in want.shape if d != 1), \
            (name, tuple(have.shape), tuple(want.shape))
        have = have.reshape(want.shape)
        if name in zeros:
            errs[name] = float(have.double().norm().cpu() / ref[sibling(name)].norm())
        else:
            errs[name] = rel_l2(have, want)
    return errs
