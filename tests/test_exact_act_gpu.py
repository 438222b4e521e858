"""Exact tests of the SiLU / GELU instantiations of the reducing kernels, with saturating data: tolerance 0.

tests/test_exact_gpu.py holds the kernels to a float64 reference bit for bit, with the activation code "none".  The activation is a
template parameter of almost every hot kernel, so the instantiations the networks run are other compiled code - and some variants
exist with an activation only: the LDS-DMA ring kernel's BN + gate prologue (SiLU, statistics, the per-tile gate table), the
wave-autonomous weight gradient's BN + act (+ gate) prologues, the matrix-core depthwise forward's LDS geometry behind an
activating prologue, the eval epilogues of pwconv_eval / dwconv_eval (SiLU) and the GELU epilogue of the 256-tile GEMM.

The technique (tests/_exact.py, act64): the pre-activations come from {-128, -96, 32, 64}, where the kernels' own formulas return
exactly 0 and exactly z, derivative exactly 0 and 1 - SiLU and GELU act as a ReLU computed through the real SiLU / GELU code.  Every
product, sum and store stays exact, so `check_exact`'s argument carries over: an activation skipped on a ragged tail row (a negative
pre-activation then comes through), a gate applied before the activation (2**-5 * 32 = 1 is not saturated), a gate row of the
neighbouring image, an act' missing from one lane all change the result by whole quanta.  (An activation applied TWICE is the one
mistake saturating data cannot see: max(max(z, 0), 0) is max(z, 0).)  The first test measures the saturation on the device; tests/test_exact_act_cpu.py proves on any machine that
max(z, 0) is also the true function's correctly rounded value at these points, runs the conditions of every case here and asserts
that at least 40 % of the operands behind an activation are non-zero.

Every dfd_tune change sits in `tuned()` and restores the defaults the rest of the suite runs with.
"""

from __future__ import annotations

import ctypes

import pytest

from tests import _exact as E
from tests._exact import ACT_GELU, ACT_SILU, ACTS, BF16, same
from tests.test_exact_gpu import DT, _dw_all, _k, _pw_fwd, _wgrad, dev, part_sums, tuned

pytestmark = pytest.mark.gpu

ACT_IDS = {ACT_SILU: "silu", ACT_GELU: "gelu"}
act_param = pytest.mark.parametrize("act", ACTS, ids=[ACT_IDS[a] for a in ACTS])


# ================================================================================================================== the probe
@pytest.mark.parametrize("rd", DT)
@act_param
def test_saturated_activations_probe(act, rd):
    """Runs first.  The thresholds of tests/_exact.py come from an f32 emulation of the formulas; here the device's own v_exp / v_rcp
    say whether they hold: every probe point through bn_act_apply (forward) and act_bn_bwd mode 0 with D = 1 (derivative) has to come
    back as max(z, 0) and (z > 0).  (`same` compares values: the -0 the formulas give below the thresholds equals 0.)  Every other
    test of this file rests on this one: if it fails, the saturation claim is wrong, not the kernels."""
    K = _k()
    c = E.act_probe(act)
    y, st = dev(c.y, rd), dev(c.st)
    fwd = K.bn_act_apply(y, st, act)
    dz, _, _ = K.act_bn_bwd(dev(c.ones, rd), y, None, None, st, act)
    print(f"probe act {act} {rd}: z {c.z[0, :, 0, 0].tolist()} -> fwd {fwd[0, :, 0, 0].tolist()} grad {dz[0, :, 0, 0].tolist()}")
    same(fwd, c.fwd, f"act {act} {rd}: act(z) at the probe points")
    same(dz, c.grad, f"act {act} {rd}: act'(z) at the probe points")


# ================================================================================================================ 1x1 forward
@pytest.mark.parametrize("rd", DT)
@pytest.mark.parametrize("ci", range(len(E.PW_ACT_CASES)), ids=[f"{c[0]}-{'x'.join(map(str, c[1]))}" for c in E.PW_ACT_CASES])
def test_pwconv_forward_with_saturated_activations_is_exact(ci, rd):
    """BN + act and BN + act + gate with SiLU and GELU on every tier that takes a prologue, with statistics and without.  The ring
    kernel has one such instantiation, <BN + gate, SiLU, statistics> (bf16): its plan function is asserted, and the same case runs once
    more through dfd_tune(4, 0) on the register-staged kernel.  The ring shapes put 4 (HW = 25), 1 (64), 2 (103, 197) images into the
    gate table of a 64-row tile."""
    K = _k()
    lib = K._L()
    tier, (N, HW, Kd, No), _, _ = E.PW_ACT_CASES[ci]
    for act in ACTS:
        for mode in E.PW_ACT_MODES:
            c = E.pw_fwd_act(ci, mode, act)
            ring = rd == BF16 and tier == "ring" and mode == 2 and act == ACT_SILU
            if ring:
                assert lib.dfd_pw_ntd_plan(N * HW, Kd, No) > 0, "the ring kernel no longer serves this shape"
            _pw_fwd(K, c, rd)
            if ring:
                with tuned({4: 0}):
                    assert lib.dfd_pw_ntd_plan(N * HW, Kd, No) == 0
                    _pw_fwd(K, c, rd)


@pytest.mark.parametrize("rd", DT)
@pytest.mark.parametrize("ci", E.PW_EVAL_CASES, ids=[f"{E.PW_FWD_CASES[i][0]}-{'x'.join(map(str, E.PW_FWD_CASES[i][1]))}" for i in E.PW_EVAL_CASES])
def test_pwconv_eval_is_exact(ci, rd):
    """The SiLU epilogue of the eval form, panel-resident and tile kernel: z = scale (y +- 1/2) is saturated whatever integer y is."""
    K = _k()
    e = E.pw_eval(ci)
    w_nk, _ = K.prep_weights(dev(e.c.w), rd, True, False)
    same(K.pwconv_eval(dev(e.c.a, rd), w_nk, dev(e.st), ACT_SILU), e.out, f"{e.what} {rd}")


# ========================================================================================================= 1x1 weight gradient
@pytest.mark.parametrize("rd", DT)
@pytest.mark.parametrize("case", E.WGRAD_TILED_CASES)
def test_pwconv_wgrad_tiled_kernel_with_saturated_activations_is_exact(case, rd):
    K = _k()
    for act in ACTS:
        for pmode, qmode in E.WGRAD_TILED_ACT_MODES:
            _wgrad(K, E.pw_wgrad(case, pmode, qmode, False, act), pmode, qmode, rd, accumulate=(pmode, qmode, act) == (3, 2, ACT_SILU))


@pytest.mark.parametrize("modes", E.WGRAD_LARGE_ACT_MODES, ids=[f"narrow{n}-wide{w}-{ACT_IDS[a]}" for n, w, a in E.WGRAD_LARGE_ACT_MODES])
@pytest.mark.parametrize("case", E.WGRAD_LARGE_CASES)
def test_pwconv_wgrad_large_m_with_saturated_activations_is_exact(case, modes):
    """The wave-autonomous kernel (bf16, M >= 196,608) takes an activating prologue on its wide operand only: BN + act + gate with SiLU
    (narrow operand raw or affine2) and BN + act with SiLU or GELU behind affine2.  The wide operand is q at 24 x 144 and p at 32 x 8
    and 144 x 24, so both operand orders run.  The kernel has no plan function; E.tnw_serves restates its conditions."""
    K = _k()
    narrow_mode, wide_mode, act = modes
    assert E.tnw_serves(case, narrow_mode, wide_mode, act), "the wave-autonomous kernel does not take this case"
    pmode, qmode = (narrow_mode, wide_mode) if case[2] <= case[3] else (wide_mode, narrow_mode)
    _wgrad(K, E.pw_wgrad(case, pmode, qmode, True, act), pmode, qmode, BF16, accumulate=modes == (3, 2, ACT_SILU))


# =================================================================================================================== depthwise
@pytest.mark.parametrize("rd", DT)
@act_param
@pytest.mark.parametrize("case", E.DW_CASES)
def test_depthwise_vector_unit_kernels_with_saturated_activations_are_exact(case, act, rd):
    """Forward with the BN + act prologue, data gradient with the act' epilogue and its sums, weight gradient with the prologue."""
    with tuned({0: 0}):
        _dw_all(_k(), E.dw(case, act), rd, f"depthwise {case} act {act} {rd}")


@act_param
@pytest.mark.parametrize("case", [c for c in E.DW_CASES if c[3] % 16 == 0] + [E.DW_MM_ACT_CASE])
def test_depthwise_matrix_core_forward_with_saturated_activations_is_exact(case, act):
    """The matrix-core forward plans its tiles with another cost behind an activating prologue: the plan is asked with the prologue
    flag, and at DW_MM_ACT_CASE it has to differ from the plan without (two images per tile instead of one)."""
    from deepfakedetection_amd._lib import DwShape

    K = _k()
    c = E.dw(case, act)
    N, H, W, C, k, s, pt, pl = case
    plan, plain = (ctypes.c_int * 12)(), (ctypes.c_int * 12)()
    shape = DwShape(N, H, W, C, c.Ho, c.Wo, k, s, pt, pl)
    assert K._L().dfd_dw_mm_plan(ctypes.byref(shape), 1, plan) == 0, "the matrix-core planner declined the shape"
    if case == E.DW_MM_ACT_CASE:
        assert K._L().dfd_dw_mm_plan(ctypes.byref(shape), 0, plain) == 0 and list(plan) != list(plain), "the two plans no longer differ here"
    with tuned({0: 9}):
        _dw_all(K, c, BF16, f"depthwise {case} act {act} matrix-core form")


def test_depthwise_with_saturated_silu_is_exact_with_several_items_per_workgroup():
    K = _k()
    c = E.dw(E.DW_SQUEEZED_CASE, ACT_SILU)
    with tuned({0: 0, 8: 16, 9: 16, 10: 16, 11: 3}):
        for rd in DT:
            _dw_all(K, c, rd, f"depthwise {c.shape} SiLU {rd}, squeezed grid")


@pytest.mark.parametrize("rd", DT)
@pytest.mark.parametrize("case", E.DW_CASES)
def test_dwconv_eval_is_exact(case, rd):
    """conv -> BN -> SiLU stored activated, and the channel sums of the stored tensor per (tile, image)."""
    K = _k()
    e = E.dw_eval(case)
    N, H, W, C, k, s, pt, pl = case
    out, parts, tiles = K.dwconv_eval(dev(e.c.xt, rd), dev(e.c.w), dev(e.st), ACT_SILU, k, s, pt, pl, e.c.Ho, e.c.Wo)
    same(out, e.out, f"{e.what} {rd}")
    assert parts.shape == (tiles, N, C)
    same(parts.double().sum(0), e.img_sums, f"{e.what} {rd}: channel sums of the stored tensor")


# ================================================================================================================== row passes
@pytest.mark.parametrize("rd", DT)
@act_param
@pytest.mark.parametrize("case", E.ROW_CASES)
def test_row_passes_with_saturated_activations_are_exact(case, act, rd):
    """bn_act_apply, act_bn_bwd in its three modes, pool_act, pool_bwd_reduce; the one-ulp allowances are those of
    test_row_passes_are_exact (the quotient dpool / (H*W) where H*W is no power of two), nothing else."""
    K = _k()
    c = E.rows(case, act)
    N, H, W, C = case
    tag = f"{c.what} {rd}"
    y, g, st, gate, dpool = dev(c.y, rd), dev(c.g, rd), dev(c.st), dev(c.gate), dev(c.dpool)
    same(K.bn_act_apply(y, st, act), c.at, f"{tag}: bn_act_apply")
    for mode, (D, gt, dp) in enumerate([(g, None, None), (g, gate, dpool), (None, None, dpool)]):
        dz, parts, n = K.act_bn_bwd(D, y, gt, dp, st, act)
        if mode == 0 or c.pow2_hw or rd == BF16:
            same(dz, c.dz[mode], f"{tag}: act_bn_bwd mode {mode}")
            same(part_sums(parts, n, C), c.dz_sums[mode], f"{tag}: act_bn_bwd sums mode {mode}")
        else:
            if mode == 2:
                E.within_one_ulp(dz, c.dz[mode], f"{tag}: act_bn_bwd mode {mode} (dpool / (H*W), H*W no power of two)")
            else:
                E.within_quotient_ulp(dz, c.dz[mode], c.quot, f"{tag}: act_bn_bwd mode {mode} (D * gate + dpool / (H*W), H*W no power of two)")
            E.sums_within(part_sums(parts, n, C), c.dz_sums[mode], c.dz_sum_tol[mode], f"{tag}: act_bn_bwd sums mode {mode} (inexact quotient)")
    pooled = K.pool_act(y, st, act)
    if c.pow2_hw:
        same(pooled, c.pooled, f"{tag}: pool_act")
    else:
        E.within_one_ulp(pooled, c.pooled, f"{tag}: pool_act (H*W no power of two)")
    same(K.pool_bwd_reduce(g, y, st, act), c.pool_bwd, f"{tag}: pool_bwd_reduce")


@pytest.mark.parametrize("rd", DT)
@act_param
def test_bn_add_act_with_saturated_activations_is_exact(act, rd):
    K = _k()
    c = E.bn_add(act)
    C = E.ADD_ACT_CASE[3]
    y, other, g, st = dev(c.y, rd), dev(c.other, rd), dev(c.g, rd), dev(c.st)
    same(K.bn_add_act(y, st, other, act), c.out, f"{c.what} {rd}: forward")
    d, parts, n = K.bn_add_act_bwd(g, y, st, other, act)
    same(d, c.d, f"{c.what} {rd}: backward")
    same(part_sums(parts, n, C), c.d_sums, f"{c.what} {rd}: sums (d, d * xhat)")


# ============================================================================================================ dense convolution
@pytest.mark.parametrize("rd", DT)
@pytest.mark.parametrize("case", E.CONV_CASES)
def test_dense_convolution_with_saturated_gelu_is_exact(case, rd):
    """conv_fwd (direct 3x3 kernel / implicit GEMM) with statistics and without, conv_wgrad with and without the BN-backward map, and
    im2col, all behind BN + GELU."""
    K = _k()
    act = ACT_GELU
    c = E.conv(case, act)
    k, s, p, C, Co, H, N = case
    tag = f"{c.what} {rd}"
    x, st = dev(c.x, rd), dev(c.st)
    w_nk, _ = K.prep_weights(K.conv_weight_to_gemm(dev(c.w)), rd, True, False)
    y, parts, n = K.conv_fwd(x, st, act, w_nk, k, s, p, c.Ho, c.Ho, stats=True)
    same(y, c.y, f"{tag}: conv_fwd")
    same(part_sums(parts, n, Co), c.y_sums, f"{tag}: conv_fwd statistics")
    y2, _, _ = K.conv_fwd(x, st, act, w_nk, k, s, p, c.Ho, c.Ho, stats=False)
    same(y2, c.y, f"{tag}: conv_fwd, no statistics")
    pt, praw, p2, coef = dev(c.pt, rd), dev(c.p, rd), dev(c.p2, rd), dev(c.coef)
    for pin, pro in ((pt, None), (praw, K.pro_affine2(p2, coef))):
        same(K.conv_wgrad(pin, pro, x, st, act, k, s, p), c.dw, f"{tag}: conv_wgrad {'with' if pro is not None else 'without'} map")
    same(K.im2col(x, st, act, k, s, p, c.Ho, c.Ho), E.im2col64(c.xa, k, s, p, c.Ho), f"{tag}: im2col")


def test_gemm_bias_act_with_saturated_gelu_is_exact():
    """The fused epilogue of the 256-tile GEMM with GELU: y + bias in 64 Z + 32, saturated either side."""
    K = _k()
    c = E.gemm_bias_act(ACT_GELU)
    M, Kd, N = E.GEMM_BIAS_ACT_CASE
    assert K._L().dfd_gemm_plan(M, Kd, N) == 256, "the 256-tile GEMM no longer serves this shape"
    w_nk, _ = K.prep_weights(dev(c.w), BF16, True, False)
    for res, want in ((dev(c.res, BF16), c.out), (None, c.out - c.res.double())):
        fused = K.gemm_bias_act(dev(c.a, BF16), w_nk, dev(c.st), ACT_GELU, res, dev(c.rs), want_raw=True)
        assert fused is not None, "shape expected to be served by the fused kernel"
        same(fused[0], want, f"gemm_bias_act: gelu(scale * y + shift) * row scale {'+ residual' if res is not None else ''}")
        same(fused[1], c.y, "gemm_bias_act: raw product")
