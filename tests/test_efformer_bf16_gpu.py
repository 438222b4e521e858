"""Every EfficientFormerV2 stage in bf16, one sub-module at a time, with DropPath row scales: every tensor on its own.

Each case runs one HIP sub-module forward and backward on bf16 NHWC inputs (a fixed bf16 output gradient, optionally written-down
DropPath row scales through HipBlock.forward(x, rng=fake)) and judges `out`, `x.grad` and EVERY parameter gradient against the
oracle sub-module in float64 on the same values (tests/_efformer_bwd_ref.py; its CPU twin is test_efformer_bf16_ref_cpu.py):

    rel_l2(engine, float64) <= FACTOR * yardstick + 2e-3

where the yardstick is the same oracle sub-module with f32 parameters under CPU bf16 autocast against float64.  FACTOR 2 and the
floor 2e-3 are test_mbconv_bwd_bf16_gpu.py's, for its reasons; the floor decides for the plain column-sum biases (the downsample's
conv.bn.bias / proj.bn.bias, yardstick 6e-9 .. 6e-8).  No tensor is left out: a structurally zero gradient (the helper's docstring names
them) is judged on its sibling weight's scale, ||got|| <= (FACTOR * yard[sibling] + 2e-3) * ||ref[sibling]||, and a convolution
bias in front of a batch-statistics BatchNorm must be exactly zero.  The largest structural zero that is not exact measured
5.0e-3 of its sibling (token_mixer.k.bn.bias of S1 block (2,7) at N = 37 in eval mode, ratio 0.40).

The cases are the smallest at which the path named still runs:
  * ConvMlp: S1 block (0,0) at 63 x 56^2 = 197,568 rows (fused expand backward, with and without row scales: the fused kernel takes
    the UNSCALED gradient as residual while BatchNorm takes the scaled one), its neighbours that must not take it (62 x 56^2 =
    194,432 rows; L block (0,4), C = 40 > 32), S1 block (2,3) at 64 x 14^2 = 12,544 rows (C 120 -> 360: dfd_pw_ntd_plan puts fc1
    and fc2 on the ring kernel), S1 block (3,0) at 37 x 7^2 = 1,813 rows;
  * attention (the two-stage sums over _partial_rows(B) rows behind the talking-head and bias-table gradients): S1 block (2,7)
    (stride 2 + upsample) at N = 4 (one group), 37 (two groups, the second partial; scaled and not; eval mode with gradients:
    pwbn_fwd's gemm_bias_act branch), 64 (two full groups); S1 block (3,5) at 37 and 64; S2 block (2,8) (width 144) and L block
    (3,9) (width 384) at 37;
  * downsample: S1 stage 1 (dense 3x3 s2) at 16, S1 stage 3 (49 queries, 196 keys, dk 16, dv 64) at 4 and 37;
  * stem at 4 x 224^2 (ConvStemFunction, DenseConvBNFunction); tail at 37, with and without an explicit dropout draw (p 0.2).
Spies count the calls of kernels.pwconv_bwd_fused that return a result (1 at the fused shape, 0 at its neighbours) and of
kernels.attn_scores (2 in every attention case: forward scores and dT2 on the matrix cores; 0 in f32), so a silent fallback does
not pass for the path under test.

Measured on an MI355X, the largest factor a tensor of each case needs (max(err - 2e-3, 0) / yardstick; the bound allows 2):

    s1-block0.0-n63-scaled .. 1.79 (mlp.mid.bn.bias)               s1-block3.5-n37-scaled .. 0.83 (token_mixer.v.bn.weight)
    s1-block0.0-n63 ......... 1.03 (mlp.fc1.bn.weight)             s1-block3.5-n64 ......... 1.23 (token_mixer.talking_head2.bias)
    s1-block0.0-n62 ......... 0.81 (mlp.fc1.bn.weight)             s2-block2.8-n37 ......... 0.86 (token_mixer.talking_head2.bias)
    l-block0.4-n63 .......... 1.01 (mlp.fc1.bn.weight)             l-block3.9-n37 .......... 1.00 (token_mixer.talking_head2.bias)
    s1-block2.3-n64-scaled .. 0.83 (mlp.fc1.bn.weight)             s1-downsample1-n16 ...... 0.44 (x.grad)
    s1-block3.0-n37 ......... 0.64 (mlp.fc1.bn.weight)             s1-downsample3-n4 ....... 0.82 (attn.v.bn.weight)
    s1-block2.7-n4 .......... 0.78 (token_mixer.v.bn.weight)       s1-downsample3-n37 ...... 0.91 (attn.v.bn.weight)
    s1-block2.7-n37-scaled .. 1.08 (token_mixer.talking_head2.weight)   s1-stem-n4 ......... 0.67 (conv1.conv.weight)
    s1-block2.7-n37 ......... 0.76 (token_mixer.q.bn.bias)         s1-tail-n37 ............. 0.14 (x.grad)
    s1-block2.7-n64-scaled .. 1.02 (mlp.mid.bn.bias)               s1-tail-n37-dropout ..... 0.16 (x.grad)
    s1-block2.7-n37-eval .... 1.11 (x.grad)

No tensor needs a factor above 2, and the engine needed no fix.  The largest yardsticks are mlp.fc1.bn.weight's at 197,568 rows
(L block (0,4) 0.140, S1 block (0,0) 0.098, 0.048 with the row scales); everything else is 0.1 .. 3 %.  (mlp.mid.bn.bias of the
scaled S1 block (0,0): error 2.09e-2 against a yardstick of 1.06e-2.)

The same cases in f32 (test_the_same_cases_in_f32: every scaled case and every N = 37 attention case, under
test_efformer_gpu.py's 2e-4 / 1e-3 / 2e-3 in relative L2): the largest error of any tensor is 1.9e-6 (mlp.fc1.bn.weight of the
scaled S1 block (0,0)), `out` <= 5.3e-7, `x.grad` <= 4.8e-7.

Bit for bit: every case twice; the fused expand backward against the two kernels it replaces (kernels.pwconv_bwd_fused_ok forced
to False), with and without the row scales.

Mutations of vit_functions.py (not committed), each run against the bf16 and the f32 test; all fail both:
  1. `gb` instead of `g` as the residual of pwconv_bwd_fused / pwconv in ConvMlpFunction.backward: x.grad of all five scaled block
     cases is over the bound, ratio 169 (S1 block (0,0), fused) and 157 (block (2,3)); 104 .. 113 in the attention blocks, where
     every token-mixer gradient behind it follows (q.bn.weight 49 .. 50, attention_biases 42); f32 x.grad error 0.46 .. 0.48.
  2. row_scale not passed to pwbn_bwd for proj: in the three scaled attention cases x.grad ratio 39 .. 43, attention_biases 39 .. 40,
     q.bn.weight 42 .. 48, k.conv.weight 48; f32 errors 0.17 .. 0.18 (x.grad) and 0.37 .. 0.50 (token-mixer gradients).
  3. `dV` instead of K.add(dV, dv_loc) in AttentionFunction.backward: all eight attention block cases with N >= 37; x.grad ratio
     56 .. 89, v.conv.weight 44, v.bn.bias 21 .. 26, stride_conv.conv.weight 26; f32 errors 0.27 .. 0.38 (x.grad), 0.80 .. 0.89
     (v.conv.weight).
  4. K.sum_rows(dS_buf.view(-1), min(B, 32), ...) for the bias table: token_mixer.attention_biases alone, in all eight attention
     block cases with N >= 37; ratio 36 .. 49 at N = 37 and 69 .. 87 at N = 64; f32 error 0.29 .. 0.41 at N = 37, 0.69 at N = 64.
"""

from __future__ import annotations

import pytest
import torch

from tests import _efformer_bwd_ref as E

pytestmark = pytest.mark.gpu

FACTOR = 2.0
F32_TOL = {"out": 2e-4, "x.grad": 1e-3}                           # test_efformer_gpu's tolerances, here in relative L2
F32_PARAM_TOL = 2e-3

FUSED = [c for c in E.CONVMLP if (c.variant, c.n) == ("s1", 63)]
RING = [c for c in E.CONVMLP if c.stage == 2]
F32_CASES = [c for c in E.CASES if c.scaled or (c.n == 37 and c in E.ATTENTION + E.DOWNSAMPLE)]


def _ids(cases):
    return [c.id for c in cases]


class _Spy:
    """Counts the calls of kernels.<name> that return a result while installed on the kernels module."""

    def __init__(self, monkeypatch, name: str):
        from deepfakedetection_amd import kernels as K

        self.served = 0
        fn = getattr(K, name)

        def spy(*args, **kwargs):
            res = fn(*args, **kwargs)
            self.served += res is not None
            return res

        monkeypatch.setattr(K, name, spy)


def _attn_geometry(inp: E.Inputs):
    """(Nq, Nk, dk, dv) of the case's attention core."""
    a = inp.mod.token_mixer if inp.case.kind == "block" else inp.mod.attn
    return (a.N, a.N, a.key_dim, a.d) if inp.case.kind == "block" else (a.N2, a.N, a.key_dim, a.d)


def _same_bits(label: str, got: dict, base: dict) -> list[str]:
    return [f"{label}: {name} differs in bits, max |diff| {float((got[name].float() - base[name].float()).abs().max()):.3e}"
            for name in base if not torch.equal(got[name], base[name])]


@pytest.mark.parametrize("case", E.CASES, ids=_ids(E.CASES))
def test_every_tensor_against_float64(monkeypatch, case):
    from deepfakedetection_amd import kernels as K

    inp = E.inputs(case)
    ref, yard, zeros = E.reference(case)
    fused, scores = _Spy(monkeypatch, "pwconv_bwd_fused"), _Spy(monkeypatch, "attn_scores")
    got = E.engine(E.hip_module(case), inp, E.BF)
    if case in E.CONVMLP:
        assert fused.served == (1 if case in FUSED else 0), fused.served
    if case in RING:                                              # 12,544 rows: fc1 and fc2 on the LDS-DMA ring kernel
        c, cm = inp.mod.mlp.fc1.conv.in_channels, inp.mod.mlp.fc1.conv.out_channels
        rows = case.n * E.RES[case.stage] ** 2
        assert rows == 12544 and K._L().dfd_pw_ntd_plan(rows, c, cm) > 0 and K._L().dfd_pw_ntd_plan(rows, cm, c) > 0
    if inp.attention:                                             # the matrix-core products served: forward scores and dT2
        assert K.attn_mfma_supported(E.BF, *_attn_geometry(inp))
        assert scores.served == 2, scores.served
    else:
        assert scores.served == 0
    assert got["out"].dtype == (torch.float32 if case.kind == "tail" else E.BF)
    names = [n for n in ref if n not in ("out", "x.grad")]
    exact = E.exact_zeros(case, names)
    assert exact <= zeros
    nonzero = [n for n in exact if int(torch.count_nonzero(got[n]))]
    assert not nonzero, f"not exactly zero: {nonzero}"
    errs = E.errors(got, ref, zeros)
    print(f"{case.id}: " + E.table(errs, yard, zeros))
    worst = max(errs, key=lambda n: E.ratio(errs[n], yard[n]))
    print(f"{case.id}: largest ratio {E.ratio(errs[worst], yard[worst]):.2f} ({worst})")
    bad = [(n, errs[n], yard[n], round(E.ratio(errs[n], yard[n]), 2)) for n in errs if errs[n] > FACTOR * yard[n] + E.FLOOR]
    assert not bad, bad


@pytest.mark.parametrize("case", F32_CASES, ids=_ids(F32_CASES))
def test_the_same_cases_in_f32(monkeypatch, case):
    """The sharp test of the row-scale algebra, and of the f32 bgemm attention with more than one group in the two-stage sums."""
    inp = E.inputs(case)
    ref, _, zeros = E.reference(case)
    scores = _Spy(monkeypatch, "attn_scores")
    got = E.engine(E.hip_module(case), inp, torch.float32)
    assert scores.served == 0 and got["out"].dtype == torch.float32
    names = [n for n in ref if n not in ("out", "x.grad")]
    nonzero = [n for n in E.exact_zeros(case, names) if int(torch.count_nonzero(got[n]))]
    assert not nonzero, f"not exactly zero: {nonzero}"
    errs = E.errors(got, ref, zeros)
    worst = max(errs, key=errs.get)
    print(f"{case.id}: largest f32 error {errs[worst]:.3e} ({worst}); out {errs['out']:.3e}, x.grad {errs['x.grad']:.3e}")
    bad = [(n, errs[n]) for n in errs if errs[n] > F32_TOL.get(n, F32_PARAM_TOL)]
    assert not bad, bad


@pytest.mark.parametrize("case", E.CASES, ids=_ids(E.CASES))
def test_the_same_call_twice_gives_the_same_bits(case):
    inp, hmod = E.inputs(case), E.hip_module(case)
    first = E.engine(hmod, inp)
    bad = _same_bits("second call", E.engine(hmod, inp), first)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("case", FUSED, ids=_ids(FUSED))
def test_fused_expand_backward_gives_the_bits_of_the_two_kernels(monkeypatch, case):
    """ConvMlpFunction.backward hands the unscaled `g` as residual to the fused kernel and to the pwconv it replaces alike."""
    from deepfakedetection_amd import kernels as K

    inp, hmod = E.inputs(case), E.hip_module(case)
    spy = _Spy(monkeypatch, "pwconv_bwd_fused")
    base = E.engine(hmod, inp)
    assert spy.served == 1
    monkeypatch.setattr(K, "pwconv_bwd_fused_ok", lambda dz, x: False)
    two = E.engine(hmod, inp)
    assert spy.served == 1
    bad = _same_bits("two kernels", two, base)
    assert not bad, "\n".join(bad)
