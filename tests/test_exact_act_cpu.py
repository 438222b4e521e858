"""The saturated-activation cases of tests/test_exact_act_gpu.py, checked without a GPU.

Three things per case:
  * the builder runs: the exactness conditions of tests/_exact.py hold, every pre-activation lies in a saturated range, and at least
    40 % of the operands behind the activation are non-zero (about half are exact zeros now; the share is asserted so detection does
    not quietly thin out);
  * the saturation claim, for every point set used: the f32 emulation of the kernels' own formula gives max(z, 0) and (z > 0)
    exactly, and the true float64 activation and derivative differ from those by less than 2**-30 of the smallest quantum any case
    works in - so the float64 reference max(z, 0) is the operation's correctly rounded result and not a convention;
  * the f32 oracle (oracle/ops_ref.py) on the same data equals the float64 reference.  torch's f32 sigmoid / gelu return a denormal
    (silu(-96) ~ -2e-40) where the kernels' formula returns -0, so the oracle's activation is compared after flushing |v| < 2**-126
    to zero (E.flush_denormals).
"""

from __future__ import annotations

import pytest
import torch
import torch.nn.functional as F

from oracle import ops_ref as R
from tests import _exact as E
from tests._exact import ACTS, BF16, same

MIN_SHARE = 0.40


def oracle_act(z, act, rd):
    return R.rnd(E.flush_denormals(R.act_fwd(z, act)), rd)


def oracle_grad(z, act):
    return E.flush_denormals(R.act_grad(z, act))


# ------------------------------------------------------------------------------------------------------- the saturation claim
def _points(act):
    """Every pre-activation the cases use: the sets themselves, the probe points, and the lattices of the epilogue tests (the eval
    forms are SiLU's, scale (y +- 1/2) with scale 256 or 512; gemm_bias_act is GELU's, 64 Z + 32)."""
    pts = set(E.SAT + E.SAT_LEAN + E.probe_points(act))
    if act == E.ACT_SILU:
        pts |= {sc / 2 * (2 * y + s) for sc in (256.0, 512.0) for y in (-127, -1, 0, 1, 127) for s in (-1, 1)}
    else:
        pts |= {32.0 * (y + s) for y in (-96, -2, 0, 2, 96) for s in (-3, -1, 1, 3)}
    return torch.tensor(sorted(pts), dtype=torch.float64)


@pytest.mark.parametrize("act", ACTS)
def test_the_kernel_formulas_saturate_exactly_and_the_true_function_agrees(act):
    z = _points(act)
    want, want_grad = E.act64(z, act), E.act_grad64(z, act)
    fwd, grad = E.emulate_act_f32(z, act)
    same(fwd, want, f"act {act}: f32 emulation of act_fwd")
    same(grad, want_grad, f"act {act}: f32 emulation of act_grad")
    tol = 2.0 ** -30 * E.SAT_QUANTUM
    true_fwd, true_grad = E.true_act64(z, act)
    assert float((true_fwd - want).abs().max()) < tol, f"act {act}: the true activation is {float((true_fwd - want).abs().max()):.3g} away"
    assert float((true_grad - want_grad).abs().max()) < tol, f"act {act}: the true derivative is {float((true_grad - want_grad).abs().max()):.3g} away"
    same(E.flush_denormals(R.act_fwd(z.float(), act)), want, f"act {act}: oracle activation, denormals flushed")
    same(oracle_grad(z.float(), act), want_grad, f"act {act}: oracle derivative, denormals flushed")


def test_the_points_that_are_not_yet_saturated_are_rejected():
    """The emulation is sharp: one step inside the thresholds it no longer returns 0 / z, and act64 refuses such data."""
    silu, _ = E.emulate_act_f32(torch.tensor([-88.0, 16.0]), E.ACT_SILU)
    assert float(silu[0]) != 0.0 and float(silu[1]) != 16.0
    gelu, _ = E.emulate_act_f32(torch.tensor([5.0]), E.ACT_GELU)
    assert float(gelu[0]) != 5.0
    for bad, act in ((-88.0, E.ACT_SILU), (-32.0, E.ACT_SILU), (16.0, E.ACT_SILU), (0.0, E.ACT_SILU), (-14.0, E.ACT_GELU), (5.0, E.ACT_GELU)):
        with pytest.raises(E.ConditionViolated, match="saturated"):
            E.act64(torch.tensor([bad], dtype=torch.float64), act)
    with pytest.raises(E.ConditionViolated, match="non-zero"):
        E.nonzero_share("x", torch.tensor([0.0, 0.0, 1.0]))


def test_probe_data():
    for act in ACTS:
        c = E.act_probe(act)
        assert sorted(set(c.z.flatten().tolist())) == sorted(float(v) for v in E.probe_points(act))
        assert set(E.SAT) <= set(E.probe_points(act))
        for rd in E.DTYPES:
            z = c.st[0] * R.rnd(c.y, rd) + c.st[1]
            same(oracle_act(z, act, rd), c.fwd, f"probe act {act} {rd}: forward")
            same(R.rnd(c.ones * oracle_grad(z, act), rd), c.grad, f"probe act {act} {rd}: derivative")


# --------------------------------------------------------------------------------------------------------------- 1x1 forward
def _pro(i, mode, rd, act, N, HW, K):
    """R.prologue with the activation flushed: BN, act, round, gate, round."""
    a = R.rnd(i.a.view(N, HW, K), rd)
    if mode in (0, 3):
        return R.prologue(a, mode, rd, R.ACT_NONE, i.coef, None if i.a2 is None else i.a2.view(N, HW, K), i.gate)
    v = oracle_act(i.coef[0] * a + i.coef[1], act, rd)
    return R.rnd(v * i.gate[:, None, :], rd) if mode == 2 else v


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("rd", E.DTYPES)
@pytest.mark.parametrize("ci", range(len(E.PW_ACT_CASES)))
def test_pwconv_forward(ci, rd, act):
    for mode in E.PW_ACT_MODES:
        c = E.pw_fwd_act(ci, mode, act)
        assert c.share >= MIN_SHARE
        N, HW, K, No = c.shape
        A = _pro(c, mode, rd, act, N, HW, K)
        same(A, c.A, f"{c.what}: oracle prologue")
        out = R.rnd(A.reshape(N, HW, 1, K) @ R.rnd(c.w, rd).t(), rd)
        same(out, c.out, f"{c.what}: oracle product")
        same(R.stats_sums(out), c.sums, f"{c.what}: oracle statistics")


def test_the_ring_cases_vary_the_images_per_tile():
    """Images a 64-row tile of the ring kernel can touch (its gate table): 4 at HW = 25, 1 at 64 (aligned), 2 at 103 and 197."""
    ring = {c[1][1]: c[1] for c in E.PW_ACT_CASES if c[0] == "ring"}
    assert sorted(ring) == [25, 64, 103, 197]
    spans = {}
    for HW, (N, _, _, _) in ring.items():
        M = N * HW
        assert M >= 16 * 64 - 63, "fewer than the ring kernel's 16 row tiles"
        spans[HW] = max((min(m0 + 63, M - 1) // HW) - m0 // HW + 1 for m0 in range(0, M, 64))
    assert spans == {25: 4, 64: 1, 103: 2, 197: 2}


def test_the_data_shows_the_mistakes_it_is_meant_to_show():
    """On the HW = 25 ring case (BN + SiLU + gate), with the kernels' SiLU emulated in f32: each mistake of an activation-bearing
    prologue changes the product; the right order of operations reproduces the reference."""
    ci = len(E.PW_ACT_CASES) - 1
    c = E.pw_fwd_act(ci, 2, E.ACT_SILU)
    N, HW, K, No = c.shape
    z = (c.coef[0] * c.a.view(N, HW, K) + c.coef[1]).double()
    silu = lambda t: E.emulate_act_f32(t, E.ACT_SILU)[0].double()
    gate = c.gate.double()[:, None, :]
    product = lambda A: A @ c.w.double().t()
    same(product(silu(z) * gate).view(c.out.shape), c.out, "the prologue as specified")
    skipped = silu(z)
    skipped[-1, -1] = z[-1, -1]                                        # no activation on the last row
    mistakes = {"gate before the activation": silu(z * gate), "gate row of the neighbouring image": silu(z) * gate.roll(1, 0),
                "activation skipped on the last row": skipped * gate, "no gate": silu(z)}
    for name, A in mistakes.items():
        assert not torch.equal(product(A).view(c.out.shape), c.out), f"{name}: the product does not change"


@pytest.mark.parametrize("rd", E.DTYPES)
@pytest.mark.parametrize("ci", E.PW_EVAL_CASES)
def test_pwconv_eval(ci, rd):
    e = E.pw_eval(ci)
    y = R.rnd(e.c.a.view(-1, e.c.shape[2]) @ R.rnd(e.c.w, rd).t(), rd)
    same(oracle_act(y * e.st[0] + e.st[1], R.ACT_SILU, rd).view(e.out.shape), e.out, f"{e.what}: oracle")


# ---------------------------------------------------------------------------------------------------------- 1x1 weight gradient
def _wgrad(c, pmode, qmode, rd, act):
    N, HW, Ni, Nj = c.shape
    assert c.share >= MIN_SHARE
    P, Q = _pro(c.p, pmode, rd, act, N, HW, Ni), _pro(c.q, qmode, rd, act, N, HW, Nj)
    same(P, c.P, f"{c.what}: oracle prologue of p")
    same(Q, c.Q, f"{c.what}: oracle prologue of q")
    same(P.reshape(-1, Ni).t() @ Q.reshape(-1, Nj), c.dw, f"{c.what}: f32 product")


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("rd", E.DTYPES)
@pytest.mark.parametrize("case", E.WGRAD_TILED_CASES)
def test_pwconv_wgrad_tiled(case, rd, act):
    for pmode, qmode in E.WGRAD_TILED_ACT_MODES:
        _wgrad(E.pw_wgrad(case, pmode, qmode, False, act), pmode, qmode, rd, act)


def large_modes(case, narrow_mode, wide_mode):
    """(pmode, qmode) with the wide operand of the case carrying the wide mode."""
    return (narrow_mode, wide_mode) if case[2] <= case[3] else (wide_mode, narrow_mode)


@pytest.mark.parametrize("case", E.WGRAD_LARGE_CASES)
def test_pwconv_wgrad_large_m(case):
    for narrow_mode, wide_mode, act in E.WGRAD_LARGE_ACT_MODES:
        assert E.tnw_serves(case, narrow_mode, wide_mode, act)
        pmode, qmode = large_modes(case, narrow_mode, wide_mode)
        _wgrad(E.pw_wgrad(case, pmode, qmode, True, act), pmode, qmode, BF16, act)


# -------------------------------------------------------------------------------------------------------------------- depthwise
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("rd", E.DTYPES)
@pytest.mark.parametrize("case", E.DW_CASES + [E.DW_SQUEEZED_CASE, E.DW_MM_ACT_CASE])
def test_depthwise(case, rd, act):
    c = E.dw(case, act)
    assert c.share >= MIN_SHARE
    N, H, W, C, k, s, pt, pl = case
    z = c.st[0] * c.x + c.st[1]
    xa = oracle_act(z, act, rd)
    same(xa, c.xt, f"{c.what}: oracle prologue")
    y = R.dwconv_fwd(xa, None, R.ACT_NONE, c.w, k, s, pt, pl, c.Ho, c.Wo, rd)
    same(y, c.y, f"{c.what}: oracle forward")
    same(R.stats_sums(y), c.y_sums, f"{c.what}: oracle statistics")
    dy = R.rnd(c.coef[0] * c.dz + c.coef[1] * c.yraw + c.coef[2], rd)
    same(dy, c.dyt, f"{c.what}: BN-backward map")
    da, dw = R.dwconv_bwd(dy, xa, c.w, k, s, pt, pl, rd)
    same(da, c.da, f"{c.what}: oracle data gradient")
    dzin = R.rnd(da * oracle_grad(z, act), rd)
    same(dzin, c.dzin, f"{c.what}: oracle data gradient behind act'")
    same(dw, c.dw, f"{c.what}: oracle weight gradient")
    xhat = (c.x - c.st[2]) * c.st[3]
    same(torch.stack([dzin.reshape(-1, C).sum(0), (dzin * xhat).reshape(-1, C).sum(0)]), c.dzin_sums, f"{c.what}: f32 sums of the data gradient")


@pytest.mark.parametrize("rd", E.DTYPES)
@pytest.mark.parametrize("case", E.DW_CASES)
def test_dwconv_eval(case, rd):
    e = E.dw_eval(case)
    N, H, W, C, k, s, pt, pl = case
    raw = R.dwconv_fwd(e.c.xt, None, R.ACT_NONE, e.c.w, k, s, pt, pl, e.c.Ho, e.c.Wo, rd)
    out = oracle_act(raw * e.st[0] + e.st[1], R.ACT_SILU, rd)
    same(out, e.out, f"{e.what}: oracle")
    same(out.sum((1, 2)), e.img_sums, f"{e.what}: f32 sums per image")


# ------------------------------------------------------------------------------------------------------------------- row passes
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("rd", E.DTYPES)
@pytest.mark.parametrize("case", E.ROW_CASES)
def test_row_passes(case, rd, act):
    c = E.rows(case, act)
    assert c.share >= MIN_SHARE
    N, H, W, C = case
    z = c.st[0] * c.y + c.st[1]
    a = oracle_act(z, act, rd)
    same(a, c.at, f"{c.what}: oracle activation")
    same((a * c.g).sum((1, 2)), c.pool_bwd, f"{c.what}: pool backward")
    E.within_one_ulp(a.mean((1, 2)), c.pooled, f"{c.what}: pooled mean")
    for mode, da in enumerate([c.g, c.g * c.gate[:, None, None, :] + c.dpool[:, None, None, :] / (H * W),
                               (c.dpool[:, None, None, :] / (H * W)).expand(N, H, W, C)]):
        same(R.rnd(da * oracle_grad(z, act), rd), c.dz[mode], f"{c.what}: act_bn_bwd mode {mode}")


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("rd", E.DTYPES)
def test_bn_add_act(rd, act):
    c = E.bn_add(act)
    C = E.ADD_ACT_CASE[3]
    pre = c.st[0] * R.rnd(c.y, rd) + c.st[1] + c.other
    same(oracle_act(pre, act, rd), c.out, f"{c.what}: oracle forward")
    d = R.rnd(c.g * oracle_grad(pre, act), rd)
    same(d, c.d, f"{c.what}: oracle backward")
    xhat = (c.y - c.st[2]) * c.st[3]
    same(torch.stack([d.reshape(-1, C).sum(0), (d * xhat).reshape(-1, C).sum(0)]), c.d_sums, f"{c.what}: f32 sums")


# ------------------------------------------------------------------------------------------------------------ dense convolution
@pytest.mark.parametrize("rd", E.DTYPES)
@pytest.mark.parametrize("case", E.CONV_CASES)
def test_dense_convolution(case, rd):
    act = E.ACT_GELU
    c = E.conv(case, act)
    assert c.share >= MIN_SHARE
    k, s, p, C, Co, H, N = case
    a = oracle_act(c.st[0] * c.x + c.st[1], act, rd)
    same(a, c.xt, f"{c.what}: oracle prologue")
    y = R.rnd(F.conv2d(a.permute(0, 3, 1, 2), R.rnd(c.w, rd), stride=s, padding=p).permute(0, 2, 3, 1), rd)
    same(y, c.y, f"{c.what}: conv2d")
    same(R.stats_sums(y), c.y_sums, f"{c.what}: oracle statistics")
    col = E.im2col64(a.double(), k, s, p, c.Ho).float()
    same(c.pt.view(-1, Co).t() @ col.reshape(-1, k * k * C), c.dw, f"{c.what}: f32 weight gradient")


def test_gemm_bias_act_with_gelu():
    g = E.gemm_bias_act(E.ACT_GELU)
    y = R.rnd(g.a @ g.w.t(), BF16)
    same(y, g.y, "gemm_bias_act product")
    M = y.shape[0]
    z = g.st[0] * y + g.st[1]
    same(R.rnd(E.flush_denormals(R.act_fwd(z, R.ACT_GELU)) * g.rs.view(M, 1, 1, 1) + g.res, BF16), g.out, "gemm_bias_act GELU epilogue")
    assert float(g.z.abs().min()) >= 32.0


@pytest.mark.parametrize("act", ACTS)
def test_mx_quant_rows_data(act):
    """The saturated values survive the MX fp8 quantiser of the oracle exactly; the first block of row 0 is all zero."""
    c = E.mx_rows(act)
    for rd in E.DTYPES:
        want = oracle_act(c.st[0] * R.rnd(c.a, rd) + c.st[1], act, rd)
        same(want, c.want, f"mx_quant_rows act {act} {rd}: oracle prologue")
        q, s = R.mx_quant(want)
        same(R.mx_dequant(q, s), c.want, f"mx_quant_rows act {act} {rd}: quantised and dequantised")
        assert int(s[0, 0]) == 0 and int(q[0, :32].max()) == 0
