"""Exact integer-data tests of the reducing kernels, at every dispatch tier: tolerance 0.

The tolerance tests (tests/test_ops_gpu.py, tests/test_vit_ops_gpu.py) draw Gaussian inputs and accept rounding noise: 1.6e-2 for bf16
tensors, 3e-3 .. 5e-3 for weight gradients, 1e-3 .. 2e-3 for statistics.  That noise floor is wide enough to hide the mistakes these
kernels actually make - a weight gradient that drops its last 32-row step, a forward that drops the last K element, a statistics
partial row counted twice, a bf16 store that truncates.  Here there is no noise floor.

The technique (tests/_exact.py; tests/test_mx_gpu.py does the same for the block-scaled GEMM): the operands are small nonzero
integers and the BN states, BN-backward coefficients, gates and row scales are powers of two times small integers, so every
product, every partial sum in ANY order and every stored value is exactly representable, and the kernel has to equal a float64
reference bit for bit.  The conditions under which that holds are asserted on the CPU before anything is launched (`check_exact`):
  * every operand, after its prologue, is exactly representable in the storage dtype;
  * every reduction has sum |term| <= 2**24 quanta, so every f32 summation order is exact;
  * every bf16-stored result is an integer with |v| <= 256, every f32 result has |v| <= 2**24;
  * statistics: the bound holds for the total over all rows, so device-side and host-side partial sums are both exact.
A case that violates one is an error of the test, never a skip; no element is masked or left out of a comparison.  This file uses
the activation code "none" wherever an entry point takes one; an entry point that declines it for some prologue is covered with
the prologues it does accept.  The SiLU / GELU instantiations are exact too where the activation SATURATES: with pre-activations
from {-128, -96, 32, 64} the kernels' own formulas return exactly 0 and exactly z (derivative 0 and 1), so SiLU and GELU act as a
ReLU computed through the real SiLU / GELU code and the argument above carries over.  Those cases - the variants that cannot be
reached with "none" at all among them - are in tests/test_exact_act_gpu.py (sets, thresholds and the probe that measures them:
tests/_exact.py, act64).  tests/test_exact_cpu.py and tests/test_exact_act_cpu.py check the same cases (conditions, and the f32 oracle
on the same data) on any machine.

Two quantities are not bit-exact by nature, because a multiplication by the rounded reciprocal and a division differ by up to one
f32 ulp: the pooled mean and the dpool / (H*W) term of act_bn_bwd.  Where H*W is a power of two they are exact as well; elsewhere
(5 x 3, 56 x 56) the f32 result is allowed ONE f32 ulp against the correctly rounded quotient - where the quotient is one term of
D * gate + dpool / (H*W), one ulp of that term plus the half ulp of the sum's own rounding - and the bf16 result is still exact (the
quotient is an integer within one f32 ulp, which the bf16 store rounds away).  The kernel's statistics are sums of the STORED dz, so
they are compared at tolerance 0 in every mode and at every shape in bf16, and in f32 wherever dz is exact: mode 0 everywhere, all
modes at 8 x 8 and at 64 x 64 (12,288 rows, many partial rows).  Only the f32 sums of modes 1 and 2 at 5 x 3 and 56 x 56 add inexact
terms; they are held to the worst-case bound of an f32 sum of such terms in any order (tests/_exact.py, rows()), which is tight at
60 rows and loose at 9,408 - the exact checks at that size are the bf16 run and the 64 x 64 shape.

The last section checks the ROUNDING of the bf16 stores: every output is a single product of two random bf16 numbers, the
reference is the exact f32 product rounded to nearest-even by torch, and the data is asserted to contain enough outputs that
truncation would get wrong (>= 40 %) and enough exact ties of both kinds (>= 16).

Every dfd_tune change sits in try / finally and restores the defaults the rest of the suite runs with.
"""

from __future__ import annotations

import contextlib
import ctypes

import pytest
import torch

from tests import _exact as E
from tests._exact import BF16, F32, same

pytestmark = pytest.mark.gpu

DT = [F32, BF16]
ACT_NONE = 0
TUNE_DEFAULTS = {0: 1, 4: 1, 8: 1024, 9: 1024, 10: 1024, 11: 32}


def _k():
    from deepfakedetection_amd import kernels

    return kernels


def dev(t, rd=None):
    if t is None:
        return None
    return (t if rd is None else t.to(rd)).cuda()


@contextlib.contextmanager
def tuned(settings: dict):
    """dfd_tune keys for the block; the defaults used elsewhere in the suite come back whatever happens inside."""
    lib = _k()._L()
    try:
        for key, value in settings.items():
            assert lib.dfd_tune(key, value) == 0
        yield
    finally:
        for key in settings:
            lib.dfd_tune(key, TUNE_DEFAULTS[key])


def part_sums(parts, n, C):
    """The partial rows [n][2][C] a kernel left, added on the host in float64 (exact: every row is an exact f32)."""
    assert n >= 1
    return parts[: n * 2 * C].view(n, 2, C).double().sum(0).cpu()


def make_pro(K, i, mode, HW, rd, act=ACT_NONE):
    """Prologue struct of `mode` (0 none, 1 BN, 2 BN + gate, 3 affine2) over the inputs of a builder; the tensors stay alive with it."""
    if mode == 0:
        return None
    if mode == 3:
        return K.pro_affine2(dev(i.a2, rd), dev(i.coef))
    if mode == 1:
        return K.pro_bn_act(dev(i.coef), act)
    return K.pro_bn_act_gate(dev(i.coef), act, dev(i.gate), HW)


# ======================================================================================================== 1x1 forward
def _pw_fwd(K, c, rd):
    N, HW, Kd, No = c.shape
    a = dev(c.a, rd)
    pro = make_pro(K, c, c.mode, HW, rd, getattr(c, "act", ACT_NONE))
    w_nk, _ = K.prep_weights(dev(c.w), rd, True, False)
    out, parts, n = K.pwconv(a, pro, w_nk, None, stats=c.has_stats)
    same(out, c.out, f"{c.what} {rd}: out")
    if c.has_stats:
        same(part_sums(parts, n, No), c.sums, f"{c.what} {rd}: statistics (sum y, sum y*y)")
        out1, _, _ = K.pwconv(a, pro, w_nk, None, stats=False)
        same(out1, c.out, f"{c.what} {rd}: out without statistics")
    if c.has_res:
        out2, _, _ = K.pwconv(a, pro, w_nk, dev(c.res, rd), stats=False)
        same(out2, c.out_res, f"{c.what} {rd}: out + residual")


@pytest.mark.parametrize("rd", DT)
@pytest.mark.parametrize("ci", range(len(E.PW_FWD_CASES)), ids=[f"{c[0]}-{'x'.join(map(str, c[1]))}" for c in E.PW_FWD_CASES])
def test_pwconv_forward_is_exact_at_every_tier(ci, rd):
    """Tile kernel (64-row instances with column tiles 32 / 64 / 128; the 128-row instance serves BN and BN + gate at 50 x 197 rows),
    panel-resident wave-autonomous kernel, LDS-DMA ring kernel (and, through dfd_tune(4, 0), the register-staged kernel on the ring
    kernel's shapes), 256-tile LDS-DMA GEMM.  Prologues none, BN, BN + gate, affine2; statistics where the entry point takes them;
    the residual for none and affine2.  The ring kernel and the 256-tile GEMM are bf16 kernels: their plan functions are asserted so
    that a silent fallback cannot pass for them (f32 runs the same shapes on the tile kernel)."""
    K = _k()
    lib = K._L()
    tier, (N, HW, Kd, No), _, _ = E.PW_FWD_CASES[ci]
    if rd == BF16 and tier == "ring":
        assert lib.dfd_pw_ntd_plan(N * HW, Kd, No) > 0, "the ring kernel no longer serves this shape"
    if rd == BF16 and tier == "gemm":
        assert lib.dfd_gemm_plan(N * HW, Kd, No) == 256, "the 256-tile GEMM no longer serves this shape"
    for mode in E.pw_modes(tier):
        c = E.pw_fwd(ci, mode)
        _pw_fwd(K, c, rd)
        if rd == BF16 and tier == "ring":
            with tuned({4: 0}):
                assert lib.dfd_pw_ntd_plan(N * HW, Kd, No) == 0
                _pw_fwd(K, c, rd)


# ==================================================================================================== 1x1 weight gradient
def _wgrad_into(K, p, pro_p, q, pro_q, dw, accumulate):
    """kernels.pwconv_wgrad with the accumulate flag of the C entry point."""
    Ni, Nj = p.shape[-1], q.shape[-1]
    M = p.numel() // Ni
    lib = K._L()
    ws = K.scratch(p.device, "wgrad_ws", lib.dfd_pwconv_wgrad_ws(M, Ni, Nj))
    K.check(lib.dfd_pwconv_wgrad(K._dt(p), K._p(p), ctypes.byref(pro_p) if pro_p is not None else None, Ni, K._p(q),
                                 ctypes.byref(pro_q) if pro_q is not None else None, Nj, M, K._p(dw), int(accumulate), K._p(ws),
                                 ws.numel() * 4, K._stream()), "dfd_pwconv_wgrad", f"M={M} Ni={Ni} Nj={Nj}")
    return dw


def _wgrad(K, c, pmode, qmode, rd, accumulate):
    N, HW, Ni, Nj = c.shape
    p, q = dev(c.p.a, rd), dev(c.q.a, rd)
    pro_p, pro_q = make_pro(K, c.p, pmode, HW, rd, c.act), make_pro(K, c.q, qmode, HW, rd, c.act)
    same(K.pwconv_wgrad(p, pro_p, q, pro_q), c.dw, f"{c.what} {rd}: dw")
    if accumulate:
        slot = dev(c.pre).clone()
        same(_wgrad_into(K, p, pro_p, q, pro_q, slot, True), c.dw_acc, f"{c.what} {rd}: dw accumulated onto integers")
        same(_wgrad_into(K, p, pro_p, q, pro_q, slot, False), c.dw, f"{c.what} {rd}: dw over a used destination")


@pytest.mark.parametrize("rd", DT)
@pytest.mark.parametrize("case", E.WGRAD_TILED_CASES)
def test_pwconv_wgrad_tiled_kernel_is_exact(case, rd):
    """Split-K tiled kernel: p plain and affine2, q plain, BN and BN + gate; row counts of 64 * 40 + 1 and 64 * 40 - 1 among them, so the
    last reduction step of the last split holds one row / misses one row; accumulate onto a destination preloaded with integers."""
    K = _k()
    for pmode, qmode in E.WGRAD_TILED_MODES:
        _wgrad(K, E.pw_wgrad(case, pmode, qmode), pmode, qmode, rd, accumulate=(pmode, qmode) in ((0, 0), (3, 2)))


@pytest.mark.parametrize("rd", DT)
@pytest.mark.parametrize("case", E.WGRAD_LARGE_CASES)
def test_pwconv_wgrad_large_m_is_exact(case, rd):
    """M >= 196,608 rows: bf16 runs the wave-autonomous kernel (raw x raw, affine2 x raw, raw x affine2, both operand orders), f32 the
    tiled kernel over many splits (it has no affine2 prologue on q).  Values from {-1, 1}: sum |term| = M."""
    K = _k()
    for pmode, qmode in E.WGRAD_LARGE_MODES:
        if rd == F32 and qmode == 3:
            continue
        _wgrad(K, E.pw_wgrad(case, pmode, qmode, True), pmode, qmode, rd, accumulate=(pmode, qmode) == (3, 0))


# ================================================================================================== fused expand backward
@pytest.mark.parametrize("case", E.FUSED_CASES)
def test_fused_expand_backward_is_exact(case):
    K = _k()
    c = E.pw_fused(case)
    dz, y, x, coef = dev(c.dz, BF16), dev(c.y, BF16), dev(c.x, BF16), dev(c.coef)
    _, w_kn = K.prep_weights(dev(c.w), BF16, True, True)
    for res, want_dx in ((None, c.dx), (dev(c.res, BF16), c.dx_res)):
        both = K.pwconv_bwd_fused(dz, y, coef, x, w_kn, res)
        assert both is not None, "shape expected to be served by the fused kernel"
        tag = f"{c.what} {'with' if res is not None else 'without'} residual"
        same(both[0], want_dx, f"{tag}: dx")
        same(both[1], c.dw, f"{tag}: dw")


# ================================================================================================================ depthwise
def _dw_all(K, c, rd, tag):
    """Forward, data gradient and weight gradient of one shape, with and without the BN prologue / epilogue and the BN-backward map.
    c.act is the activation of the prologue / epilogue (E.dw(case, act)); the variants without a BN state take none."""
    N, H, W, C, k, s, pt, pl = c.shape
    act = c.act
    x, xt, w, st = dev(c.x, rd), dev(c.xt, rd), dev(c.w), dev(c.st)
    dz, dyt, yraw, coef = dev(c.dz, rd), dev(c.dyt, rd), dev(c.yraw, rd), dev(c.coef)
    y, parts, n = K.dwconv_fwd(x, st, act, w, k, s, pt, pl, c.Ho, c.Wo, stats=True)
    same(y, c.y, f"{tag}: forward with the BN prologue")
    same(part_sums(parts, n, C), c.y_sums, f"{tag}: forward statistics")
    if act != ACT_NONE:
        y1, _, _ = K.dwconv_fwd(x, st, act, w, k, s, pt, pl, c.Ho, c.Wo, stats=False)
        same(y1, c.y, f"{tag}: forward with the BN prologue, without statistics")
    y2, parts, n = K.dwconv_fwd(xt, None, ACT_NONE, w, k, s, pt, pl, c.Ho, c.Wo, stats=True)
    same(y2, c.y, f"{tag}: forward")
    same(part_sums(parts, n, C), c.y_sums, f"{tag}: forward statistics, no prologue")
    y3, _, _ = K.dwconv_fwd(xt, None, ACT_NONE, w, k, s, pt, pl, c.Ho, c.Wo, stats=False)
    same(y3, c.y, f"{tag}: forward without statistics")
    for (d, yr, cf), (xin, sti) in [((dz, yraw, coef), (x, st)), ((dyt, None, None), (x, st)), ((dz, yraw, coef), (None, None)),
                                    ((dyt, None, None), (None, None))]:
        v = f"{'map' if cf is not None else 'plain'}, {'epilogue' if xin is not None else 'no epilogue'}"
        dzin, parts, n = K.dwconv_bwd_data(d, yr, cf, w, xin, sti, act if sti is not None else ACT_NONE, (N, H, W, C), k, s, pt, pl)
        same(dzin, c.dzin if xin is not None else c.da, f"{tag}: data gradient ({v})")
        if xin is not None:
            same(part_sums(parts, n, C), c.dzin_sums, f"{tag}: data-gradient sums (dzin, dzin * xhat) ({v})")
    for (d, yr, cf), (xin, sti) in [((dz, yraw, coef), (x, st)), ((dyt, None, None), (xt, None)), ((dz, yraw, coef), (xt, None)),
                                    ((dyt, None, None), (x, st))]:
        v = f"{'map' if cf is not None else 'plain'}, {'prologue' if sti is not None else 'no prologue'}"
        same(K.dwconv_bwd_weight(d, yr, cf, xin, sti, act if sti is not None else ACT_NONE, k, s, pt, pl), c.dw, f"{tag}: weight gradient ({v})")


@pytest.mark.parametrize("rd", DT)
@pytest.mark.parametrize("case", E.DW_CASES)
def test_depthwise_vector_unit_kernels_are_exact(case, rd):
    with tuned({0: 0}):                                      # the vector-unit forward for every shape
        _dw_all(_k(), E.dw(case), rd, f"depthwise {case} {rd}")


@pytest.mark.parametrize("case", [c for c in E.DW_CASES if c[3] % 16 == 0])
def test_depthwise_matrix_core_forward_is_exact(case):
    from deepfakedetection_amd._lib import DwShape

    K = _k()
    c = E.dw(case)
    N, H, W, C, k, s, pt, pl = case
    plan = (ctypes.c_int * 12)()
    assert K._L().dfd_dw_mm_plan(ctypes.byref(DwShape(N, H, W, C, c.Ho, c.Wo, k, s, pt, pl)), 1, plan) == 0, "the matrix-core planner declined the shape"
    with tuned({0: 9}):
        _dw_all(K, c, BF16, f"depthwise {case} matrix-core form")


def test_depthwise_sums_are_exact_with_several_items_per_workgroup():
    """dfd_tune keys 8-11 squeeze the grids of the vector-unit kernels as in test_dwconv_grid_knobs_change_the_partial_rows_not_the_tensors:
    every workgroup then walks several work items and adds their statistics up itself."""
    K = _k()
    c = E.dw(E.DW_SQUEEZED_CASE)
    N, H, W, C, k, s, pt, pl = c.shape
    with tuned({0: 0}):
        _, _, n_default = K.dwconv_fwd(dev(c.xt, BF16), None, ACT_NONE, dev(c.w), k, s, pt, pl, c.Ho, c.Wo, stats=True)
    with tuned({0: 0, 8: 16, 9: 16, 10: 16, 11: 3}):
        _, _, n_squeezed = K.dwconv_fwd(dev(c.xt, BF16), None, ACT_NONE, dev(c.w), k, s, pt, pl, c.Ho, c.Wo, stats=True)
        assert n_squeezed < n_default, f"the squeezed grid has as many partial rows as the default one: {n_squeezed} / {n_default}"
        for rd in DT:
            _dw_all(K, c, rd, f"depthwise {c.shape} {rd}, squeezed grid")


# ===================================================================================================================== stem
@pytest.mark.parametrize("rd", DT)
@pytest.mark.parametrize("pad", E.STEM_PADS)
@pytest.mark.parametrize("case", E.STEM_CASES)
def test_stem_is_exact(case, pad, rd):
    """32 x 32 inputs with 32 / 48 channels run the matrix-core kernels in bf16, 33 x 35 with 40 channels the f32-FMA kernels."""
    K = _k()
    c = E.stem(case, pad)
    Co = case[3]
    x, w = dev(c.x), dev(c.w)
    y, parts, n = K.stem_conv_fwd(x, w, rd, 2, pad[0], pad[1], c.Ho, c.Wo)
    same(y, c.y, f"{c.what} {rd}: forward")
    same(part_sums(parts, n, Co), c.y_sums, f"{c.what} {rd}: statistics")
    same(K.stem_conv_wgrad(x, dev(c.dz, rd), dev(c.yraw, rd), dev(c.coef), 3, 2, pad[0], pad[1]), c.dw, f"{c.what} {rd}: weight gradient")
    same(K.stem_conv_wgrad(x, dev(c.dyt, rd), None, None, 3, 2, pad[0], pad[1]), c.dw, f"{c.what} {rd}: weight gradient, no map")


# =============================================================================================================== row passes
@pytest.mark.parametrize("rd", DT)
@pytest.mark.parametrize("case", E.ROW_CASES)
def test_row_passes_are_exact(case, rd):
    K = _k()
    c = E.rows(case)
    N, H, W, C = case
    tag = f"{c.what} {rd}"
    if case == (3, 56, 56, 96):
        assert int(K._L().dfd_pool_ws(K._dt(dev(c.y, rd)), N, H * W, C)) > 0, "shape was meant to split H*W over workgroups"
    y, g, st, rs, gate, dpool = dev(c.y, rd), dev(c.g, rd), dev(c.st), dev(c.rs), dev(c.gate), dev(c.dpool)
    for scale, want, want_bias in ((None, c.red, c.bias), (rs, c.red_rs, c.bias_rs)):
        v = "with" if scale is not None else "without"
        parts, n = K.bn_bwd_reduce(g, y, st, scale)
        same(part_sums(parts, n, C), want, f"{tag}: bn_bwd_reduce {v} row scale (sum g, sum g * xhat)")
        same(K.bias_grad(g, scale), want_bias, f"{tag}: bias_grad {v} row scale")
        slot = torch.full((C,), 7.0, device="cuda")
        assert K.bias_grad(g, scale, out=slot) is slot
        same(slot, want_bias, f"{tag}: bias_grad into a destination")
    for mode, (D, gt, dp) in enumerate([(g, None, None), (g, gate, dpool), (None, None, dpool)]):
        dz, parts, n = K.act_bn_bwd(D, y, gt, dp, st, ACT_NONE)
        if mode == 0 or c.pow2_hw or rd == BF16:
            # (bf16, H*W no power of two: dpool / (H*W) is an integer within one f32 ulp, which the bf16 store rounds away)
            same(dz, c.dz[mode], f"{tag}: act_bn_bwd mode {mode}")
        elif mode == 2:
            E.within_one_ulp(dz, c.dz[mode], f"{tag}: act_bn_bwd mode {mode} (dpool / (H*W), H*W no power of two)")
        else:
            E.within_quotient_ulp(dz, c.dz[mode], c.quot, f"{tag}: act_bn_bwd mode {mode} (D * gate + dpool / (H*W), H*W no power of two)")
        if mode == 0 or c.pow2_hw or rd == BF16:
            # (the kernel adds up the stored dz, which is exact here: sums of exact terms)
            same(part_sums(parts, n, C), c.dz_sums[mode], f"{tag}: act_bn_bwd sums mode {mode}")
        else:
            E.sums_within(part_sums(parts, n, C), c.dz_sums[mode], c.dz_sum_tol[mode], f"{tag}: act_bn_bwd sums mode {mode} (inexact quotient)")
    pooled = K.pool_act(y, st, ACT_NONE)
    if c.pow2_hw:
        same(pooled, c.pooled, f"{tag}: pool_act")
    else:
        E.within_one_ulp(pooled, c.pooled, f"{tag}: pool_act (H*W no power of two)")
    same(K.pool_bwd_reduce(g, y, st, ACT_NONE), c.pool_bwd, f"{tag}: pool_bwd_reduce")
    same(K.pool_bwd_reduce(g, y, st, ACT_NONE), c.pool_bwd, f"{tag}: pool_bwd_reduce again (arrival counters re-armed)")
    parts, n = K.channel_stats(g)
    same(part_sums(parts, n, C), c.g_stats, f"{tag}: channel_stats")
    both = torch.empty((2, C), device="cuda")
    K.sum_rows(parts, n, 2 * C, both.view(-1))
    same(both, c.g_stats, f"{tag}: channel_stats through sum_rows")


@pytest.mark.parametrize("P", E.SUM_ROWS_P)
def test_sum_rows_is_exact(P):
    K = _k()
    c = E.sum_rows(P)
    out = torch.full((c.L,), 5.0, device="cuda")
    K.sum_rows(dev(c.parts).view(-1), P, c.L, out)
    same(out, c.want, f"sum_rows of {P} rows")
    acc = dev(c.pre).clone()
    K.sum_rows(dev(c.parts).view(-1), P, c.L, acc, accumulate=True)
    same(acc, c.want_acc, f"accumulating sum_rows of {P} rows")


def test_grad_sumsq_is_exact():
    K = _k()
    c = E.grad_sumsq()
    keep, table = [], []
    for g in c.gs:
        d = dev(g)
        keep.append(d)
        for off in range(0, g.numel(), c.chunk):
            cnt = min(c.chunk, g.numel() - off)
            table.append([0, d.data_ptr() + 4 * off, 0, 0, cnt])
    partials = torch.full((len(table),), -1.0, dtype=torch.float64, device="cuda")
    K.grad_sumsq(torch.tensor(table, dtype=torch.int64, device="cuda"), partials)
    same(partials, c.want, "grad_sumsq")


# ========================================================================================================== dense convolution
@pytest.mark.parametrize("rd", DT)
@pytest.mark.parametrize("case", E.CONV_CASES)
def test_dense_convolution_is_exact(case, rd):
    """conv_fwd (the direct 3x3 kernel for bf16 stride-1 layers with 64 / 96 / 128 input channels, the implicit GEMM otherwise) with
    and without the producer's BN, with statistics; conv_wgrad with and without the BN-backward map and the BN; col2im."""
    K = _k()
    c = E.conv(case)
    k, s, p, C, Co, H, N = case
    tag = f"{c.what} {rd}"
    x, xt, st = dev(c.x, rd), dev(c.xt, rd), dev(c.st)
    w_nk, _ = K.prep_weights(K.conv_weight_to_gemm(dev(c.w)), rd, True, False)
    for xin, state in ((xt, None), (x, st)):
        v = "with" if state is not None else "without"
        y, parts, n = K.conv_fwd(xin, state, ACT_NONE, w_nk, k, s, p, c.Ho, c.Ho, stats=True)
        same(y, c.y, f"{tag}: conv_fwd {v} BN")
        same(part_sums(parts, n, Co), c.y_sums, f"{tag}: conv_fwd statistics {v} BN")
        y2, _, _ = K.conv_fwd(xin, state, ACT_NONE, w_nk, k, s, p, c.Ho, c.Ho, stats=False)
        same(y2, c.y, f"{tag}: conv_fwd {v} BN, no statistics")
    pt, praw, p2, coef = dev(c.pt, rd), dev(c.p, rd), dev(c.p2, rd), dev(c.coef)
    for pin, pro in ((pt, None), (praw, K.pro_affine2(p2, coef))):
        for xin, state in ((xt, None), (x, st)):
            same(K.conv_wgrad(pin, pro, xin, state, ACT_NONE, k, s, p), c.dw,
                 f"{tag}: conv_wgrad {'with' if pro is not None else 'without'} map, {'with' if state is not None else 'without'} BN")
    same(K.col2im(dev(c.dcol, rd), (N, H, H, C), k, s, p), c.dx, f"{tag}: col2im")


# =========================================================================================== matrix products of the ViT path
def test_bgemm_is_exact():
    K = _k()
    c = E.bgemm()
    B, H, Nq, Nk, dk, dv = E.BGEMM_CASE
    S = torch.empty((B, H, Nq, Nk), device="cuda")
    K.bgemm(dev(c.q), (H * Nq * dk, Nq * dk, dk, 1), dev(c.k), (H * Nk * dk, Nk * dk, 1, dk), S, (H * Nq * Nk, Nq * Nk, Nk, 1), B, H, Nq, Nk, dk)
    same(S, c.S, "bgemm 49 x 196")
    O = torch.empty((B, H, Nq, dv), device="cuda")
    K.bgemm(S, (H * Nq * Nk, Nq * Nk, Nk, 1), dev(c.v), (H * Nk * dv, Nk * dv, dv, 1), O, (H * Nq * dv, Nq * dv, dv, 1), B, H, Nq, dv, Nk)
    same(O, c.O, "bgemm K = 196")


@pytest.mark.parametrize("case", E.ATTN_APPLY_CASES)
def test_attn_apply_is_exact(case):
    K = _k()
    c = E.attn_apply(case)
    B, H, To, Tc, D = case
    assert K.attn_mfma_supported(BF16, To, Tc, D, D)
    f = dev(c.f)
    same(K.attn_apply(f, dev(c.x, BF16), (B, To, 1, H * D), H, alpha=0.5), c.out, f"attn_apply {case}")
    same(K.attn_apply(f, dev(c.g, BF16), (B, Tc, 1, H * D), H, alpha=0.5, transpose=True), c.out_t, f"attn_apply {case} transposed")


@pytest.mark.parametrize("case", E.LINEAR_CASES)
def test_linear_is_exact(case):
    K = _k()
    c = E.linear(case)
    x, w, b, dout = dev(c.x), dev(c.w), dev(c.b), dev(c.dout)
    same(K.linear_fwd(x, w, b), c.out, f"linear_fwd {case}")
    dx, dw, db = K.linear_bwd(dout, x, w, True, True, True)
    same(dx, c.dx, f"linear_bwd dx {case}")
    same(dw, c.dw, f"linear_bwd dw {case}")
    same(db, c.db, f"linear_bwd db {case}")


def test_gemm_bias_act_is_exact():
    K = _k()
    c = E.gemm_bias_act()
    M, Kd, N = E.GEMM_BIAS_ACT_CASE
    w_nk, _ = K.prep_weights(dev(c.w), BF16, True, False)
    fused = K.gemm_bias_act(dev(c.a, BF16), w_nk, dev(c.st), ACT_NONE, dev(c.res, BF16), dev(c.rs), want_raw=True)
    assert fused is not None, "shape expected to be served by the fused kernel"
    same(fused[0], c.out, "gemm_bias_act: (scale * y + shift) * row scale + residual")
    same(fused[1], c.y, "gemm_bias_act: raw product")


def test_vit_scatter_and_gather_sums_are_exact():
    K = _k()
    c = E.vit_small()
    for rd in DT:
        same(K.avgpool_fwd(dev(c.x, rd), 2, 2), c.pooled, f"avgpool_fwd k = 2 {rd}")
        same(K.avgpool_bwd(dev(c.gp, rd), (2, 14, 14, 32), 2, 2), c.dpool, f"avgpool_bwd k = 2 {rd}")
        same(K.rowtable_grad(dev(c.gt, rd), 49), c.rowtable, f"rowtable_grad {rd}")
        same(K.subsample_add_bwd(dev(c.gs, rd), dev(c.dx0, rd).clone(), 2), c.dx1, f"subsample_add_bwd {rd}")
    same(K.bias_scatter(dev(c.dfull), dev(c.idx), c.n), c.scat, "bias_scatter")
    table = torch.zeros((c.T, c.H), device="cuda")
    same(K.relpos_bias_bwd(dev(c.dbias), table, dev(c.ridx), c.nl, c.ng), c.dtable, "relpos_bias_bwd at table = 0 (16 * sigmoid' = 4)")


# ================================================================================================ rounding of the bf16 stores
@pytest.mark.parametrize("ci", range(len(E.ROUND_PW_CASES)), ids=[f"{c[0]}-{c[1]}x{c[2]}x{c[3]}" for c in E.ROUND_PW_CASES])
def test_pwconv_forward_rounds_its_bf16_store_to_nearest_even(ci):
    K = _k()
    lib = K._L()
    c = E.round_pw(ci)
    M, Kd, No = c.shape
    if c.tier == "ring":
        assert lib.dfd_pw_ntd_plan(M, Kd, No) > 0
    if c.tier == "gemm":
        assert lib.dfd_gemm_plan(M, Kd, No) == 256
    a = dev(c.a, BF16)
    w_nk, _ = K.prep_weights(dev(c.w), BF16, True, False)
    out, _, _ = K.pwconv(a, None, w_nk, None, stats=False)
    E.same_bits(out, c.want, f"1x1 forward, {c.tier} tier")
    if c.tier == "ring":
        with tuned({4: 0}):
            out, _, _ = K.pwconv(a, None, w_nk, None, stats=False)
        E.same_bits(out, c.want, "1x1 forward, register-staged kernel on the ring kernel's shape")


def test_row_kernels_round_their_bf16_stores_to_nearest_even():
    """dwconv_fwd with a centre-tap-only weight (both forms), bn_act_apply, act_bn_bwd, scale_rows, affine2_apply: one product of two
    bf16 numbers per output.  axpby has f32 tensors only: its single product is exact and must come back unrounded."""
    K = _k()
    c = E.round_rows()
    N, H, W, C = c.shape
    x = dev(c.x, BF16)
    w = torch.zeros((C, 1, 3, 3))
    w[:, 0, 1, 1] = c.chan
    from deepfakedetection_amd._lib import DwShape

    plan = (ctypes.c_int * 12)()
    assert K._L().dfd_dw_mm_plan(ctypes.byref(DwShape(N, H, W, C, H, W, 3, 1, 1, 1)), 1, plan) == 0, "the matrix-core planner declined the shape"
    for form, key0 in (("vector-unit", 0), ("matrix-core", 9)):
        with tuned({0: key0}):
            y, _, _ = K.dwconv_fwd(x, None, ACT_NONE, dev(w), 3, 1, 1, 1, H, W, stats=False)
        E.same_bits(y, c.by_chan, f"dwconv_fwd, centre tap only, {form}")
    st = torch.zeros((4, C))
    st[0], st[3] = c.chan, 1.0
    E.same_bits(K.bn_act_apply(x, dev(st), ACT_NONE), c.by_chan, "bn_act_apply")
    dz, _, _ = K.act_bn_bwd(x, x, dev(c.img_chan), torch.zeros((N, C), device="cuda"), dev(st), ACT_NONE)
    E.same_bits(dz, c.by_img_chan, "act_bn_bwd (D * gate)")
    E.same_bits(K.scale_rows(x, dev(c.img)), c.by_img, "scale_rows")
    coef = torch.zeros((3, C))
    coef[0] = c.chan
    E.same_bits(K.affine2_apply(x, x, dev(coef)), c.by_chan, "affine2_apply")
    xf = dev(c.x)
    same(K.axpby(xf, None, a=E.TIE_FACTOR, b=0.0), c.x.double() * E.TIE_FACTOR, "axpby (f32: the product of two bf16 numbers is exact)")
    same(K.axpby(xf, xf, a=E.TIE_FACTOR, b=0.0), c.x.double() * E.TIE_FACTOR, "axpby with a zero-weighted addend")
