"""Every depthwise, stem and squeeze-excite geometry of the configurations the reference runs, derived from the layer plans and
the built modules (pure Python, no GPU).

Configurations: EfficientNet-B0 (timm) at 224 / 160 px, EfficientNet-B3 (efficientnet_pytorch: TF-SAME padding frozen at the
nominal 300 px) at 224 / 160 / 300 px, EfficientFormerV2-S0 / S1 / S2 at 224 / 160 px.  A geometry is what the engine hands the
kernels: the input map, the padding it passes (top == left == the layer's leading pad) and the output map it asks for.

Depthwise entries also carry how the model calls the kernels, because that picks the kernel instance:
  pro    activation of the BatchNorm prologue the forward (and the weight gradient) applies to its input: "silu" for the MBConv
         depthwise after an expand layer, None where the input is stored activated (or is the block input);
  epi    activation of the BatchNorm whose backward the data gradient applies as its epilogue (with statistics): "silu" (MBConv),
         "gelu" (the ConvMlp mid layer), None;
  stats  the forward takes BatchNorm statistics and the backward gets the BN-backward map (dz, y, coef); False for the
         attention-downsampling `local_q` (a plain convolution + bias);
  eval   the f32 inference form (dwconv_eval) serves the layer (EfficientNet MBConv blocks).
"""

from __future__ import annotations

import math
from typing import NamedTuple

from deepfakedetection_amd.arch import efficientnet_plan

ACTS = {None: 0, "silu": 1, "gelu": 3}          # oracle/ops_ref.py ACT_* codes


class Dw(NamedTuple):
    H: int
    W: int
    C: int
    k: int
    stride: int
    pt: int
    pl: int
    Ho: int
    Wo: int
    pro: str | None
    epi: str | None
    stats: bool
    eval: bool

    @property
    def geom(self) -> tuple:
        return (self.H, self.W, self.C, self.k, self.stride, self.pt, self.pl, self.Ho, self.Wo)


class Stem(NamedTuple):
    H: int
    W: int
    Cout: int
    k: int
    stride: int
    pt: int
    pl: int
    Ho: int
    Wo: int


class Se(NamedTuple):
    H: int
    W: int
    C: int
    R: int                 # squeeze-excite width


# name -> (family, variant, flavour, input size)
CONFIGS = {
    "b0_timm_224": ("efficientnet", "b0", "timm", 224),
    "b0_timm_160": ("efficientnet", "b0", "timm", 160),
    "b3_lukemelas_224": ("efficientnet", "b3", "lukemelas", 224),
    "b3_lukemelas_160": ("efficientnet", "b3", "lukemelas", 160),
    "b3_lukemelas_300": ("efficientnet", "b3", "lukemelas", 300),
    "efficientformerv2_s0_224": ("efficientformerv2", "s0", None, 224),
    "efficientformerv2_s0_160": ("efficientformerv2", "s0", None, 160),
    "efficientformerv2_s1_224": ("efficientformerv2", "s1", None, 224),
    "efficientformerv2_s1_160": ("efficientformerv2", "s1", None, 160),
    "efficientformerv2_s2_224": ("efficientformerv2", "s2", None, 224),
    "efficientformerv2_s2_160": ("efficientformerv2", "s2", None, 160),
}


def _uniq(items) -> list:
    return list(dict.fromkeys(items))


def _efficientnet(variant: str, flavour: str, size: int):
    plan = efficientnet_plan(variant, flavour)
    g = plan.stem
    h = g.out_size(size)
    stems = [Stem(size, size, plan.stem_out, g.kernel, g.stride, g.pad_lead, g.pad_lead, h, h)]
    dws, ses = [], []
    for b in plan.blocks:
        d = b.dw
        ho = d.out_size(h)
        act = "silu" if b.expand else None
        dws.append(Dw(h, h, b.cmid, d.kernel, d.stride, d.pad_lead, d.pad_lead, ho, ho, act, act, True, True))
        ses.append(Se(ho, ho, b.cmid, b.se_width))
        h = ho
    return stems, dws, ses


def _conv_out(size: int, conv) -> int:
    return (size + 2 * conv.padding[0] - conv.kernel_size[0]) // conv.stride[0] + 1


def _dw_module(h: int, conv, epi, stats: bool) -> Dw:
    assert conv.groups == conv.in_channels == conv.out_channels and conv.kernel_size[0] == conv.kernel_size[1]
    ho = _conv_out(h, conv)
    p = conv.padding[0]
    return Dw(h, h, conv.out_channels, conv.kernel_size[0], conv.stride[0], p, p, ho, ho, None, epi, stats, False)


def _efficientformer(variant: str, size: int):
    """Walks the built module tree (CPU parameters only): stem conv1, then per stage the attention-downsampling branch
    (`q.local`, `v_local`, both on the stage's input map), per block the attention's `stride_conv` / `v_local` and the ConvMlp
    mid layer."""
    from deepfakedetection_amd.efficientformer_v2 import HipEfficientFormerV2

    net = HipEfficientFormerV2(variant, 2, size)
    c1, c2 = net.stem.conv1.conv, net.stem.conv2.conv
    h1 = _conv_out(size, c1)
    p = c1.padding[0]
    stems = [Stem(size, size, c1.out_channels, c1.kernel_size[0], c1.stride[0], p, p, h1, h1)]
    h = _conv_out(h1, c2)
    dws = []
    for stage in net.stages:
        ds = stage.downsample
        if hasattr(ds, "conv"):
            if ds.attn is not None:
                dws.append(_dw_module(h, ds.attn.q.local, None, False))
                dws.append(_dw_module(h, ds.attn.v_local.conv, None, True))
            h = _conv_out(h, ds.conv.conv)
        for blk in stage.blocks:
            tm = blk.token_mixer
            if tm is not None:
                ha = h
                if tm.stride_conv is not None:
                    dws.append(_dw_module(h, tm.stride_conv.conv, None, True))
                    ha = _conv_out(h, tm.stride_conv.conv)
                assert tm.resolution == (ha, ha)
                dws.append(_dw_module(ha, tm.v_local.conv, None, True))
            dws.append(_dw_module(h, blk.mlp.mid.conv, "gelu", True))
    assert h == math.ceil(size / 32)
    return stems, dws, []


def config_layers(name: str):
    """(stems, depthwise layers, squeeze-excite layers) of one configuration, in network order, with repeats."""
    family, variant, flavour, size = CONFIGS[name]
    if family == "efficientnet":
        return _efficientnet(variant, flavour, size)
    return _efficientformer(variant, size)


def config_geometries(name: str):
    """The distinct (stems, depthwise, squeeze-excite) geometries of one configuration."""
    stems, dws, ses = config_layers(name)
    return _uniq(stems), _uniq(dws), _uniq(ses)


def all_geometries():
    """The distinct geometries over every configuration: (stems, depthwise, squeeze-excite)."""
    stems, dws, ses = [], [], []
    for name in CONFIGS:
        s, d, e = config_geometries(name)
        stems += s
        dws += d
        ses += e
    return _uniq(stems), _uniq(dws), _uniq(ses)
