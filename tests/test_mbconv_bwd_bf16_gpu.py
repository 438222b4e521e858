"""MBConvFunction in bf16, one block at a time, at the row counts where its backward changes kernels: every tensor on its own.

Each case runs one HIP block forward and backward on bf16 NHWC inputs (hblk.run, a fixed bf16 output gradient, optionally a
drop-connect row scale) and judges `out`, `x.grad` and EVERY parameter gradient (13, or 10 without an expand layer) against the
oracle block in float64 on the same values (tests/_mbconv_bwd_ref.py):

    rel_l2(engine, float64) <= FACTOR * yardstick + 2e-3

where the yardstick is the same oracle block under CPU bf16 autocast on a contiguous NCHW input against float64 — what bf16
rounding alone costs that tensor in a block this shallow (0.2 .. 13 %).  FACTOR is 2, as in
test_fullsize_gpu.test_b3_training_step_at_the_reference_configuration; 2e-3 is test_ops_gpu.test_rowpass's tolerance of the
f32 BatchNorm-backward sums and decides only for the project BatchNorm's bias, whose gradient is a plain f32 column sum
(yardstick 1e-7; 2e-3 with a row scale, which rounds the scaled gradient to bf16 on both sides).  No tensor is left out.

The cases are the smallest at which each path still runs:
  * >= 196,608 rows — fused expand backward (kernels.pwconv_bwd_fused), wave-autonomous weight gradient, panel-resident
    forward: B0 block 1 (training and eval mode with gradients), block 2 (skip; with and without a row scale: the fused kernel
    adds the UNSCALED gradient as its residual while BatchNorm takes the scaled one), block 3 (k5 s2), B3 block 2 (asymmetric
    TF-SAME padding, eps 1e-3);
  * their neighbours that must not take it: B3 block 3 (Cmid 192 > 144), B0 block 1 at 188,160 rows;
  * ring kernel, tile kernels and tiled weight gradient: B3 block 1 and B0 block 0 (no expand layer; with / without skip),
    B0 block 10 (12,544 rows, k5, skip), B0 block 15, B3 blocks 14, 19, 25 (widths 136, 232, 816, 1392: multiples of 8 only).
A spy counts the calls of kernels.pwconv_bwd_fused that return a result, so a silent fallback does not pass for the path under
test.  Three block-level equivalences are bit for bit: fused against the two kernels it replaces, frozen inputs at a fused
shape (the mask changes the kernel there), and the same call twice.

Measured on an MI355X, the largest factor a tensor of each case needs (max(err - 2e-3, 0) / yardstick; the bound allows 2):

    B0 block 1, 16 x 112^2 ............ 0.84 (bn1.bias)        B0 block 1, 15 x 112^2 ........ 0.81 (bn1.bias)
    B0 block 1, 16 x 112^2, eval ...... 0.65 (se.conv_expand.bias)
    B0 block 2, 63 x 56^2, row scale .. 1.02 (bn1.weight)      B3 block 1, 8 x 56^2, row scale  0.59 (_se_expand.bias)
    B0 block 2, 63 x 56^2 ............. 1.00 (bn1.bias)        B0 block 0, 8 x 56^2 ........... 0.45 (se.conv_expand.bias)
    B0 block 3, 63 x 56^2 ............. 0.74 (bn1.weight)      B0 block 10, 64 x 14^2 ......... 0.80 (bn1.weight)
    B3 block 2, 16 x 112^2 ............ 0.75 (_bn0.weight)     B0 block 15, 64 x 7^2 .......... 0.70 (bn1.weight)
    B3 block 3, 63 x 56^2, row scale .. 0.89 (_bn0.bias)       B3 block 14, 64 x 14^2, row scale 0.79 (_bn0.weight)
    B3 block 19, 64 x 7^2 ............. 0.70 (_bn0.weight)     B3 block 25, 64 x 7^2 .......... 0.73 (_bn0.weight)

No tensor needs a factor above 2.  The largest yardsticks are those of the expand BatchNorm of B0 block 2 (bn1.weight 0.13,
bn1.bias 0.10: gradients that nearly cancel over 197,568 rows); everywhere else they are 0.2 .. 6 %.  The same blocks through
the engine in f32 stay below 2e-6 on every tensor.  Mutations of MBConvFunction.backward (not committed) fail the bound: `None`
instead of `g` as the fused kernel's residual gives x.grad of B0 block 2 a ratio of 99 (with a row scale) and 119 (without); `g`
instead of `gb` to bn_bwd_reduce gives bn3.bias / _bn2.bias ratios of 132 .. 244 and bn3.weight / _bn2.weight 48 .. 68 in all four
row-scale cases (nine tensors of each are over the bound).
"""

from __future__ import annotations

import pytest
import torch

from tests import _mbconv_bwd_ref as M
from tests._mbconv_bwd_ref import Case

pytestmark = pytest.mark.gpu

FACTOR = 2.0                                                     # no tensor of any case needs more

FUSED = [Case("b0", 1, 16, 112), Case("b0", 1, 16, 112, train=False), Case("b0", 2, 63, 56, scaled=True), Case("b0", 2, 63, 56),
         Case("b0", 3, 63, 56), Case("b3", 2, 16, 112)]
NEIGHBOURS = [Case("b3", 3, 63, 56, scaled=True), Case("b0", 1, 15, 112)]
SMALL = [Case("b3", 1, 8, 56, scaled=True), Case("b0", 0, 8, 56), Case("b0", 10, 64, 14), Case("b0", 15, 64, 7),
         Case("b3", 14, 64, 14, scaled=True), Case("b3", 19, 64, 7), Case("b3", 25, 64, 7)]
CASES = FUSED + NEIGHBOURS + SMALL


def _ids(cases):
    return [c.id for c in cases]


class _FusedSpy:
    """Counts the calls of kernels.pwconv_bwd_fused that return a result while installed on the kernels module."""

    def __init__(self, monkeypatch):
        from deepfakedetection_amd import kernels as K

        self.served = 0
        fn = K.pwconv_bwd_fused

        def spy(*args, **kwargs):
            res = fn(*args, **kwargs)
            self.served += res is not None
            return res

        monkeypatch.setattr(K, "pwconv_bwd_fused", spy)


def _fused_shape(inp: M.Inputs) -> bool:
    """kernels.pwconv_bwd_fused_ok on the shapes and dtype of the block's (dz1, x)."""
    from deepfakedetection_amd import kernels as K

    if inp.blk.c.expand == 1:
        return False
    n, h, w, cin = inp.x.shape
    return K.pwconv_bwd_fused_ok(torch.empty((n, h, w, inp.cmid), dtype=M.BF, device="meta"), torch.empty((n, h, w, cin), dtype=M.BF, device="meta"))


def _same_bits(label: str, got: dict, base: dict, names) -> list[str]:
    bad = []
    for name in names:
        if got[name] is None or base[name] is None:
            bad.append(f"{label}: {name} received no gradient")
        elif not torch.equal(got[name], base[name]):
            bad.append(f"{label}: {name} differs in bits, max |diff| {float((got[name].float() - base[name].float()).abs().max()):.3e}")
    return bad


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_every_tensor_of_the_block_against_float64(monkeypatch, case):
    from deepfakedetection_amd import kernels as K

    inp = M.inputs(case)
    ref, yard = M.reference(case)
    assert len(ref) == (15 if inp.blk.c.expand != 1 else 12)
    spy = _FusedSpy(monkeypatch)
    got = M.engine(M.hip_block(case), inp)
    fused = case in FUSED
    assert _fused_shape(inp) == fused
    assert spy.served == (1 if fused else 0), spy.served
    if case.n * case.res ** 2 == 12544:                              # the ring kernel's row counts: both 1x1 layers of the block
        c = inp.blk.c
        assert c.stride == 1 and K._L().dfd_pw_ntd_plan(12544, c.cin, inp.cmid) > 0 and K._L().dfd_pw_ntd_plan(12544, inp.cmid, c.cout) > 0
    assert got["out"].dtype == M.BF and got["x.grad"].dtype == M.BF
    errs = M.errors(got, ref)
    print(f"{case.id}: " + M.table(errs, yard))
    worst = max(errs, key=lambda n: M.ratio(errs[n], yard[n]))
    print(f"{case.id}: largest ratio {M.ratio(errs[worst], yard[worst]):.2f} ({worst})")
    bad = [(n, errs[n], yard[n], round(M.ratio(errs[n], yard[n]), 2)) for n in errs
           if errs[n] > FACTOR * yard[n] + M.FLOOR]
    assert not bad, bad


@pytest.mark.parametrize("case", [FUSED[2], FUSED[5]], ids=_ids([FUSED[2], FUSED[5]]))
def test_fused_expand_backward_gives_the_bits_of_the_two_kernels(monkeypatch, case):
    """functions.py: the fused expand backward is "bit-identical to the two kernels below" — through the block, with the skip
    connection's unscaled gradient as residual (B0 block 2) and without a residual (B3 block 2)."""
    from deepfakedetection_amd import kernels as K

    inp, hblk = M.inputs(case), M.hip_block(case)
    spy = _FusedSpy(monkeypatch)
    base = M.engine(hblk, inp)
    assert spy.served == 1
    monkeypatch.setattr(K, "pwconv_bwd_fused_ok", lambda dz, x: False)
    two = M.engine(hblk, inp)
    assert spy.served == 1
    assert len(base) == 15
    bad = _same_bits("two kernels", two, base, base)
    assert not bad, "\n".join(bad)


def test_frozen_inputs_at_a_fused_shape(monkeypatch):
    """B0 block 1 at 200,704 rows: with x frozen, or the expand weight frozen, the block leaves the fused kernel for the two
    kernels; every gradient that is still wanted has the all-trainable run's bits and the frozen tensor gets none."""
    case = FUSED[0]
    inp, hblk = M.inputs(case), M.hip_block(case)
    spy = _FusedSpy(monkeypatch)
    base = M.engine(hblk, inp)
    assert spy.served == 1
    params = [n for n, _ in hblk.named_parameters()]
    assert len(params) == 13 and "conv_pw.weight" in params
    no_x = M.engine(hblk, inp, frozen=("x",))
    assert spy.served == 1 and no_x["x.grad"] is None
    bad = _same_bits("x frozen", no_x, base, ["out"] + params)
    no_w = M.engine(hblk, inp, frozen=("conv_pw.weight",))
    assert spy.served == 1 and no_w["conv_pw.weight"] is None
    bad += _same_bits("expand weight frozen", no_w, base, [n for n in base if n != "conv_pw.weight"])
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_the_same_call_twice_gives_the_same_bits(case):
    inp, hblk = M.inputs(case), M.hip_block(case)
    first = M.engine(hblk, inp)
    bad = _same_bits("second call", M.engine(hblk, inp), first, first)
    assert not bad, "\n".join(bad)
