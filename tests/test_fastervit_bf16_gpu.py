"""Every FasterViT stage in bf16, one sub-module at a time, with DropPath row scales, at its kernel tiers: every tensor on its own.

Each case runs one HIP sub-module forward and backward on bf16 inputs (fixed bf16 output gradients, optionally written-down
DropPath row scales through forward(..., rng=fake)) and judges the outputs, the input gradients and EVERY parameter gradient
against the oracle sub-module in float64 on the same values (tests/_fastervit_bwd_ref.py; its CPU twin is
test_fastervit_bf16_ref_cpu.py):

    rel_l2(engine, float64) <= FACTOR * yardstick + 2e-3

where the yardstick is the same oracle sub-module with f32 parameters under CPU bf16 autocast against float64.  FACTOR 2 and the
floor 2e-3 are test_mbconv_bwd_bf16_gpu.py's, for its reasons.  No tensor is left out: a structurally zero gradient is judged on
its sibling weight's scale, conv1.bias / conv2.bias of a training-mode ConvBlock must be exactly zero, and qkv.weight / qkv.bias
are judged as their q, k and v thirds (the k third of the bias is structurally zero; see the helper's docstring).

The cases are the smallest at which the path named runs; B is the number of images, a level-2 block has 4 B windows of 53 tokens
(M = 212 B rows), a level-3 block B windows of 49.  `plan` is dfd_gemm_plan's tile height for (qkv, proj, fc1, fc2) of the
window stream, 0 = not the fused kernel's shape; the carrier stream (16 B rows) is never fused at these sizes.
  HAT level 2, blocks[1]
    fv0 (C 256, head dim 32: wattn_fwd / wattn_bwd)  B 3 plain and scaled: plan (0, 0, 0, 0)
                                                     B 33 scaled: (128, 0, 128, 0); 132 windows = 33 wattn partial rows, the
                                                        second group of 32 holds a single row
                                                     B 97 scaled and plain: (256, 128, 256, 128), proj / fc2 at 161 tiles (160
                                                        is the threshold; B 96 gives 159): the production form of the block
    fv1 (C 320, head dim 40: bgemm + softmax rows)   B 33 scaled: (128, 0, 128, 0); sum_rows over 132 rows = 4 groups + 4 rows
    fv2 (C 384, head dim 48)                         B 3: none
    fv3 (C 512, head dim 64, gamma1..4)              B 3 scaled: none; B 48 scaled: (256, 128, 256, 128), proj / fc2 fused WITH
                                                        LayerScale and want_raw at exactly 160 tiles; B 47 scaled: (256, 0, 256,
                                                        0), 156 tiles
  HAT level 3, blocks[1] (no carrier tokens): fv0 B 3; B 37 scaled: none; B 68 scaled: (128, 0, 128, 0) (B 67: 156 tiles)
  ConvBlock, blocks[-1], B 3 plain, scaled and in eval mode with gradients: fv0 level 0 (C 64, 56 px) and level 1 (C 128, 28 px,
    7-row tiles) on dfd_conv3_direct; fv1 level 0 (C 80), fv3 level 1 (C 256) and ALSO fv2 level 0 (C 96) on the implicit GEMM:
    dfd_conv3_direct wants Cout % 64 == 0, so 96 -> 96 is not its shape, although C = 96 is among its input widths.
    fv0 level 0 at B 19 and level 1 at B 33, scaled: the first batches with more work items (28 / 8 tiles per image, C3_TW 16)
    than the persistent grid 512 / (Cout / 64): some workgroups walk two tiles, the last round is partial.  The path is asserted
    through the number of partial rows the training forward's convolutions report (the two kernels' grids differ).
  Downsample fv0 levels 0, 1, 2 at B 3 and 5; TokenInitializer fv0 at B 2 and 33; patch embed of fv0 (in_dim 64) and fv1
  (in_dim 32) at 4 images; the tail (TailFunction without head_dist) at 37.
Spies count the gemm_bias_act calls that return a result (forward: the number of non-zero plan entries, e.g. 4 at fv0 B 97, 2 at
B 33, 0 at B 3; backward: 0, the backward never calls it), wattn_fwd / wattn_bwd (fv0 in bf16: one per attention, 2 at level 2,
1 at level 3, no bgemm) against bgemm (every other head dim, and f32: 2 forward and 4 backward per attention), and the FakeRng
call order (window stream, then carrier stream).

Measured on an MI355X, the largest factor a tensor of each case needs (max(err - 2e-3, 0) / yardstick; the bound allows 2):

    fv0-hat2-b3 ........... 1.48 (ct.grad)           fv0-conv0-b3 / -scaled / -eval .. 0.74 / 0.64 / 0.55 (norm1.weight, norm1.bias)
    fv0-hat2-b3-scaled .... 0.70 (hat_norm2.weight)  fv0-conv1-b3 / -scaled / -eval .. 0.57 / 0.64 / 0.44 (norm1.*, conv1.weight)
    fv0-hat2-b33-scaled ... 1.10 (ct.grad)           fv2-conv0-b3 / -scaled / -eval .. 0.64 / 0.75 / 0.55 (norm1.*)
    fv0-hat2-b97-scaled ... 1.06 (ct.grad)           fv1-conv0-b3 / -scaled / -eval .. 0.70 / 0.72 / 0.45 (norm1.*, conv1.weight)
    fv0-hat2-b97 .......... 1.43 (ct.grad)           fv3-conv1-b3 / -scaled / -eval .. 0.58 / 0.66 / 0.45 (norm1.weight, conv1.weight)
    fv1-hat2-b33-scaled ... 0.89 (ct.grad)           fv0-conv0-b19-scaled ............ 0.68 (norm1.bias)
    fv2-hat2-b3 ........... 1.03 (ct.grad)           fv0-conv1-b33-scaled ............ 0.71 (norm1.bias)
    fv3-hat2-b3-scaled .... 0.84 (hat_norm2.weight)  fv0-downsample0/1/2 at b3 and b5 . 0.55 .. 0.56 (x.grad)
    fv3-hat2-b48-scaled ... 1.34 (ct.grad)           fv0-tokens-b2 / -b33 ............ 0.30 / 0.28 (out)
    fv3-hat2-b47-scaled ... 1.29 (ct.grad)           fv0-stem-b4 / fv1-stem-b4 ....... 0.98 / 0.98 (conv_down.1.bias)
    fv0-hat3-b3 ........... 0.56 (norm2.weight)      fv0-tail-b37 .................... 0.16 (x.grad)
    fv0-hat3-b37-scaled ... 0.67 (norm2.weight)
    fv0-hat3-b68-scaled ... 0.56 (norm2.weight)

No tensor needs a factor above 2, no tensor is bounded on its own, and the engine needed no fix.  The largest yardstick is 0.076
(conv_down.1.bias of the fv0 stem; the CPU twin caps it at 0.10); the hat blocks' largest are the cpb_mlp gradients at 0.04 ..
0.06, everything else is 0.2 .. 2 %.  The k third of qkv.bias measures 0.7e-4 .. 1.6e-4 of the k third of the weight (the bound
allows about 4e-2); conv1.bias and conv2.bias are exactly zero.

The same cases in f32 (test_the_same_cases_in_f32: every scaled case and every case with B >= 33, under test_fastervit_gpu.py's
2e-4 / 1e-3 / 2e-3 for the convolutional stages and 3e-4 / 2e-3 / 3e-3 for the hat blocks, in relative L2): the largest error of
any tensor is 1.4e-6 (norm1.bias of fv3-conv1-b3-scaled), 1.0e-6 in the hat blocks (attn.qkv.weight[q] of fv3 at B 47 / 48); the
outputs and the input gradients <= 8.4e-7.

Bit for bit: every case twice; the fused linear layers against the pair they replace (gemm_bias_act switched off) at fv0 B 97 and
at fv3 B 48 (LayerScale and want_raw in the epilogue); the window round trip of _PermuteRows, values and gradients.

The whole module: 104 tests in 15 s on an MI355X, the references included; the slowest test 1.9 s (fv0-hat2-b3 in bf16, which
builds the two networks), the largest blocks (B 97, B 48) 0.9 .. 1.1 s each with their float64 reference.

Mutations of fastervit_functions.py / fastervit.py (not committed), each run against the bf16, the f32 and the fused-pair test:
  1. `K.add(dx0, gb)` instead of `g` in ConvBlockFunction.backward: x.grad of all seven scaled ConvBlock cases and nothing else;
     ratio 188 .. 204 at B 3, 85 at B 19, 88 at B 33; f32 x.grad error 0.62 .. 0.64 at B 3, 0.34 at B 19 / 33.
  2. row_scale not passed to lin_bwd for proj in attn_sub_bwd: all nine scaled hat cases, bf16 and f32; 28 .. 30 tensors over the
     bound at level 2 (15 .. 16 at level 3), led by hat_attn.proj.bias (169 .. 479), hat_norm1.bias (164 .. 439) and
     attn.proj.bias (162 .. 262); at level 3 attn.proj.bias 163 .. 180, attn.proj.weight 37 .. 41; f32 x.grad error 0.7e-2 .. 1.9e-2, ct.grad 1.3e-2 .. 2.6e-2, the
     largest parameter error 0.45 .. 1.9.
  3. `K.sum_rows(dS_buf.view(-1), min(n, 32), ...)` in window_attention_bwd: the attention-bias MLPs alone, wherever the bgemm path
     sums more than 32 rows.  bf16: fv1-hat2-b33 attn.pos_emb_funct.cpb_mlp.2.weight 48, .0.weight 27, .0.bias 22; fv3 B 48 and
     B 47 likewise (47 .. 77), there also hat_attn.pos_emb_funct.cpb_mlp.* (14 .. 36: 48 / 47 carrier rows); fv0 in bf16 passes,
     it does not run this code.  f32 (every head dim on bgemm): all eight hat cases with more than 32 windows, error 0.34 (37
     windows) .. 1.05.
  4. stream id `4 * self.index` for the carrier stream in HipHAT.forward: FakeRng's assertion ("window stream (id 4 * index): 3
     rows, not the 12 windows") in all seven scaled level-2 cases, bf16 and f32, and in both fused-pair cases.
  5. `xn` instead of `x` as the residual of fc2 in mlp_sub_fwd: `out` of all thirteen hat cases, fused and unfused alike: out.ct
     ratio 213 .. 313, out.x 178 .. 214 at level 2 (and 14 .. 16 more tensors each), out 147 .. 162 at level 3; f32 out.x error
     0.29 .. 0.31, out.ct 0.39 .. 0.43.  The fused-pair test passes, as it should: both forms take the same wrong residual.
"""

from __future__ import annotations

import pytest
import torch

from tests import _fastervit_bwd_ref as E
from tests.test_efformer_bf16_gpu import _same_bits, _Spy

pytestmark = pytest.mark.gpu

FACTOR = 2.0
# test_fastervit_gpu's tolerances (there relative to the largest entry), here in relative L2
F32_TOL_HAT = {"out": 3e-4, "out.x": 3e-4, "out.ct": 3e-4, "x.grad": 2e-3, "ct.grad": 2e-3}
F32_TOL = {"out": 2e-4, "x.grad": 1e-3}
F32_PARAM_TOL_HAT, F32_PARAM_TOL = 3e-3, 2e-3

HAT = E.HAT2 + E.HAT3
F32_CASES = [c for c in E.CASES if c.scaled or c.n >= 33]
FUSED = [c for c in E.HAT2 if (c.variant, c.n, c.scaled) in (("0", 97, True), ("3", 48, True))]

# dfd_gemm_plan of (qkv, proj, fc1, fc2) on the window stream; every hat case not named here: (0, 0, 0, 0)
PLAN = {"fv0-hat2-b33-scaled": (128, 0, 128, 0), "fv0-hat2-b97-scaled": (256, 128, 256, 128), "fv0-hat2-b97": (256, 128, 256, 128),
        "fv1-hat2-b33-scaled": (128, 0, 128, 0), "fv3-hat2-b48-scaled": (256, 128, 256, 128), "fv3-hat2-b47-scaled": (256, 0, 256, 0),
        "fv0-hat3-b68-scaled": (128, 0, 128, 0)}
PROJ_TILES = {"fv0-hat2-b97-scaled": 161, "fv0-hat2-b97": 161, "fv3-hat2-b48-scaled": 160, "fv3-hat2-b47-scaled": 156}
CONV_DIRECT = {("0", 0), ("0", 1)}                               # (variant, level) of the ConvBlocks on dfd_conv3_direct


def _ids(cases):
    return [c.id for c in cases]


def _rows(case: E.Case) -> int:
    return case.windows * (53 if case.level == 2 else 49)


def _plans(case: E.Case, rows: int) -> tuple:
    """dfd_gemm_plan of qkv, proj, fc1 and fc2 at `rows` rows of the case's width."""
    from deepfakedetection_amd import kernels as K

    c = E.dim(case)
    return tuple(int(K._L().dfd_gemm_plan(rows, k, n)) for k, n in ((c, 3 * c), (c, c), (c, 4 * c), (4 * c, c)))


def _check_hat_paths(case, inp, dtype, fused_fwd, fused_bwd, fwd, bwd):
    """The paths a hat case names: fused linear layers by the planner's count, the attention kernels by head dim."""
    from deepfakedetection_amd import kernels as K

    n_attn = 2 if inp.carrier else 1
    hd = E.dim(case) // inp.mod.attn.heads
    assert hd == {"0": 32, "1": 40, "2": 48, "3": 64}[case.variant]
    if dtype == E.BF:
        plans = _plans(case, _rows(case))
        assert plans == PLAN.get(case.id, (0, 0, 0, 0)), plans
        assert not inp.carrier or _plans(case, 16 * case.n) == (0, 0, 0, 0)
        if case.id in PROJ_TILES:                                # 128-row tiles x 256-column tiles of proj (and fc2) against the 160 threshold
            assert ((_rows(case) + 127) // 128) * ((E.dim(case) + 255) // 256) == PROJ_TILES[case.id]
        assert fused_fwd == sum(p > 0 for p in plans), (fused_fwd, plans)
    else:
        assert fused_fwd == 0
    assert fused_bwd == 0
    if K.wattn_supported(dtype, 53 if inp.carrier else 49, hd):
        assert case.variant == "0" and dtype == E.BF
        assert (fwd["wattn_fwd"], bwd["wattn_bwd"], fwd["bgemm"], bwd["bgemm"]) == (n_attn, n_attn, 0, 0), (fwd, bwd)
    else:
        assert case.variant != "0" or dtype != E.BF
        assert (fwd["wattn_fwd"], bwd["wattn_bwd"], fwd["bgemm"], bwd["bgemm"]) == (0, 0, 2 * n_attn, 4 * n_attn), (fwd, bwd)
    if case.id == "fv0-hat2-b33-scaled":                         # 33 partial rows: one full group of 32 and a group of one
        assert int(K._L().dfd_wattn_parts(case.windows)) == 33
    if case.id == "fv1-hat2-b33-scaled":                         # sum_rows over 132 rows: four groups of 32 and one of 4
        assert case.windows == 4 * 32 + 4
    print(f"{case.id}: {_rows(case)} rows; rowtable_grad_plan {K.rowtable_grad_plan(dtype, case.windows * 49, 49, E.dim(case))}; "
          f"dfd_pw_ntd_plan of proj {int(K._L().dfd_pw_ntd_plan(_rows(case), E.dim(case), E.dim(case)))}")


def _run(monkeypatch, case, dtype):
    """One engine run under the spies -> (tensors, gemm_bias_act served forward / backward, path calls forward / backward,
    partial rows of the convolutions with statistics)."""
    from deepfakedetection_amd import kernels as K
    from tests.test_vit_ops_gpu import _PathSpy

    fused, paths = _Spy(monkeypatch, "gemm_bias_act"), _PathSpy(monkeypatch, K)
    conv_fwd, conv_parts = K.conv_fwd, []

    def conv_spy(*args, **kwargs):
        res = conv_fwd(*args, **kwargs)
        if kwargs.get("stats"):
            conv_parts.append(res[2])
        return res

    monkeypatch.setattr(K, "conv_fwd", conv_spy)
    mark = {}

    def after_forward():
        mark["fused"], mark["paths"] = fused.served, dict(paths.calls)

    got = E.engine(E.hip_module(case), E.inputs(case), dtype, after_forward)
    bwd = {k: paths.calls[k] - mark["paths"][k] for k in paths.calls}
    return got, mark["fused"], fused.served - mark["fused"], mark["paths"], bwd, conv_parts


def _check_conv_path(case, dtype, conv_parts):
    """Which 3x3 kernel ran, from the partial rows the two training-forward convolutions report: the direct kernel has one per
    workgroup of its persistent grid, the implicit GEMM one per row tile."""
    if not case.train:
        assert conv_parts == []                                  # eval statistics: no partial rows to tell the kernels by
        return
    c, res = E.dim(case), E.RES[case.level]
    direct, implicit = E.conv3_direct_grid(case.n, res, c), E.conv_implicit_parts(case.n, res, c)
    if dtype == E.BF and (case.variant, case.level) in CONV_DIRECT:
        assert direct is not None and min(direct) != implicit
        assert conv_parts == [min(direct)] * 2, (conv_parts, direct)
        if case.n == E.B_PAST_GRID[case.level]:
            assert direct[1] < direct[0] < 2 * direct[1]          # a second, partial round
    else:
        assert dtype != E.BF or direct is None
        assert conv_parts == [implicit] * 2, (conv_parts, implicit)


def _exactly_zero(case, ref, got):
    names = [n for n in ref if n not in E.OUTPUTS]
    nonzero = [n for n in E.exact_zeros(case, names) if int(torch.count_nonzero(got[n]))]
    assert not nonzero, f"not exactly zero: {nonzero}"


@pytest.mark.parametrize("case", E.CASES, ids=_ids(E.CASES))
def test_every_tensor_against_float64(monkeypatch, case):
    inp = E.inputs(case)
    ref, yard, zeros = E.reference(case)
    got, fused_fwd, fused_bwd, fwd, bwd, conv_parts = _run(monkeypatch, case, E.BF)
    if case.kind == "hat":
        _check_hat_paths(case, inp, E.BF, fused_fwd, fused_bwd, fwd, bwd)
    else:
        assert fused_fwd == fused_bwd == 0 and not any(fwd.values()) and not any(bwd.values())
    if case.kind == "conv":
        _check_conv_path(case, E.BF, conv_parts)
    for name in inp.g:
        assert got[name].dtype == (torch.float32 if case.kind == "tail" else E.BF), name
    assert E.exact_zeros(case, list(ref)) <= zeros
    _exactly_zero(case, ref, got)
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
    got, fused_fwd, fused_bwd, fwd, bwd, conv_parts = _run(monkeypatch, case, torch.float32)
    if case.kind == "hat":
        _check_hat_paths(case, inp, torch.float32, fused_fwd, fused_bwd, fwd, bwd)
    if case.kind == "conv":
        _check_conv_path(case, torch.float32, conv_parts)
    assert all(got[name].dtype == torch.float32 for name in inp.g)
    _exactly_zero(case, ref, got)
    errs = E.errors(got, ref, zeros)
    worst = max(errs, key=errs.get)
    print(f"{case.id}: largest f32 error {errs[worst]:.3e} ({worst}); " + ", ".join(f"{n} {errs[n]:.3e}" for n in E.OUTPUTS if n in errs))
    tol, ptol = (F32_TOL_HAT, F32_PARAM_TOL_HAT) if case.kind == "hat" else (F32_TOL, F32_PARAM_TOL)
    bad = [(n, errs[n]) for n in errs if errs[n] > tol.get(n, ptol)]
    assert not bad, bad


@pytest.mark.parametrize("case", E.CASES, ids=_ids(E.CASES))
def test_the_same_call_twice_gives_the_same_bits(case):
    inp, hmod = E.inputs(case), E.hip_module(case)
    first = E.engine(hmod, inp)
    bad = _same_bits("second call", E.engine(hmod, inp), first)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("case", FUSED, ids=_ids(FUSED))
def test_fused_linear_gives_the_bits_of_the_pair(monkeypatch, case):
    """kernels.gemm_bias_act promises the bits of pwconv + bn_act_apply: with it switched off attn_sub_fwd (through pwbn_fwd) and
    mlp_sub_fwd (through _lin_apply) run the pair, and every tensor of the block must come out the same."""
    from deepfakedetection_amd import kernels as K

    inp, hmod = E.inputs(case), E.hip_module(case)
    spy = _Spy(monkeypatch, "gemm_bias_act")
    base = E.engine(hmod, inp)
    assert spy.served == 4
    monkeypatch.setattr(K, "gemm_bias_act", lambda *args, **kwargs: None)
    pair = E.engine(hmod, inp)
    assert spy.served == 4
    bad = _same_bits("the pair", pair, base)
    assert not bad, "\n".join(bad)


def test_window_round_trip_is_exact_for_values_and_gradients():
    """_PermuteRows with _window_maps — HipFasterViTLayer's window_partition / window_reverse — at B 3 in bf16: the partition has
    the bits of the oracle's window_partition, partition then reverse is the identity, and so are the two backward passes
    (test_vit_ops_gpu.test_copy_rows_partition_and_inverse pins kernels.copy_rows on these maps, not the autograd Function)."""
    from deepfakedetection_amd.fastervit import _PermuteRows, _window_maps
    from oracle.fastervit_ref import window_partition

    B, res, C = 3, 14, 256
    gen = torch.Generator().manual_seed(11)
    x = torch.randn((B, res, res, C), generator=gen).to(E.BF)
    g = torch.randn((B * res * res, C), generator=gen).to(E.BF)
    part = _window_maps(B, res, torch.device("cuda"))[0]
    xd = x.cuda().view(-1, C).requires_grad_()
    xw = _PermuteRows.apply(xd, part, True)
    want = window_partition(x.permute(0, 3, 1, 2), 7)
    assert torch.equal(xw.detach().cpu().view(B * 4, 49, C), want)
    back = _PermuteRows.apply(xw, part, False)
    assert torch.equal(back.detach(), xd.detach())
    back.backward(g.cuda())
    assert torch.equal(xd.grad.cpu(), g)
    xd.grad = None
    xw2 = _PermuteRows.apply(xd, part, True)                     # the partition's backward alone is the reverse of the gradient
    xw2.backward(g.cuda())
    gw = window_partition(xd.grad.cpu().view(B, res, res, C).permute(0, 3, 1, 2), 7)
    assert torch.equal(gw.reshape(-1, C), g)
