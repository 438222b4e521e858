"""The exact-arithmetic cases of tests/test_exact_gpu.py and tests/test_coord_gpu.py, checked without a GPU.

For every case of the GPU file: build the inputs and the float64 reference (the builder runs the exactness conditions of
tests/_exact.py and raises if one is violated - so "the reference stays within the limits" is verified on any machine), then
evaluate the f32 oracle the tolerance tests use (oracle/ops_ref.py) on the same data.  Where the oracle has no function for the
operation - the plain products, sum_rows, grad_sumsq, the scatter / gather sums of the ViT path, col2im - the f32 side is the plain
torch op the tolerance tests compare with (a matmul, a sum, index_add_, autograd of F.unfold): another precision and another code
path than the float64 builder, not an oracle of the project.  On this data the oracle has to agree with float64 EXACTLY as well, in both storage dtypes, which
tests the oracle too.
"""

from __future__ import annotations

import pytest
import torch
import torch.nn.functional as F

from oracle import ops_ref as R
from tests import _exact as E
from tests._exact import BF16, F32, same

FAMILIES = {
    "1x1 forward": E.PW_FWD_CASES, "1x1 weight gradient, tiled": E.WGRAD_TILED_CASES, "1x1 weight gradient, large M": E.WGRAD_LARGE_CASES,
    "fused expand backward": E.FUSED_CASES, "depthwise": E.DW_CASES + [E.DW_SQUEEZED_CASE], "stem": E.STEM_CASES, "row passes": E.ROW_CASES,
    "sum_rows": E.SUM_ROWS_P, "grad_sumsq": E.GRAD_SUMSQ_SIZES, "dense convolution": E.CONV_CASES, "attn_apply": E.ATTN_APPLY_CASES,
    "rounding, 1x1 forward": E.ROUND_PW_CASES, "coordinate MLPs": E.COORD_SHAPES, "relative-position bias chain": E.CPB_GEOMS,
}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_every_family_has_cases(family):
    assert len(FAMILIES[family]) > 0


def test_the_conditions_reject_what_they_should():
    """check_exact itself: an operand bf16 cannot hold, a reduction above 2**24, a bf16 result that is no small integer."""
    ok = torch.tensor([1.0, -2.0, 0.5])
    E.check_exact("fine", operands=[("a", ok, E.DTYPES)], reductions=[("r", torch.tensor([2.0 ** 24]), 1.0)], results=[("y", ok.round(), E.DTYPES)])
    with pytest.raises(E.ConditionViolated, match="operand"):
        E.check_exact("x", operands=[("a", torch.tensor([1.0 + 2.0 ** -9]), (BF16,))])
    with pytest.raises(E.ConditionViolated, match="reduction"):
        E.check_exact("x", reductions=[("r", torch.tensor([2.0 ** 24 + 2], dtype=torch.float64), 1.0)])
    with pytest.raises(E.ConditionViolated, match="reduction"):
        E.check_exact("x", stats=[("r", torch.tensor([2.0 ** 23 + 1]), 0.5)])
    with pytest.raises(E.ConditionViolated, match="bf16 result"):
        E.check_exact("x", results=[("y", torch.tensor([0.5]), (BF16,))])
    with pytest.raises(E.ConditionViolated, match="bf16 result"):
        E.check_exact("x", results=[("y", torch.tensor([257.0]), (BF16,))])
    with pytest.raises(E.ConditionViolated, match="f32 result"):
        E.check_exact("x", results=[("y", torch.tensor([2.0 ** 24 + 1], dtype=torch.float64), (F32,))])
    with pytest.raises(AssertionError, match="1 of 3 elements differ; first at \\(1,\\): got 5.0, want -2.0"):
        same(torch.tensor([1.0, 5.0, 0.5]), ok, "x")
    same(ok.to(BF16), ok.double(), "x")
    E.within_one_ulp(torch.tensor([1.0 / 3.0]) * (1 + 2.0 ** -23), torch.tensor([1.0], dtype=torch.float64) / 3, "x")
    third = torch.tensor([1.0], dtype=torch.float64) / 3
    E.within_quotient_ulp(torch.tensor([-1.0 + 1.0 / 3.0 + 2.0 ** -25]), third - 1, third, "x")
    with pytest.raises(AssertionError, match="one f32 ulp of the quotient term"):
        E.within_quotient_ulp(torch.tensor([-1.0 + 1.0 / 3.0 + 2.0 ** -22]), third - 1, third, "x")
    with pytest.raises(AssertionError, match="more than one f32 ulp"):
        E.within_one_ulp(torch.tensor([1.0 / 3.0]) * (1 + 2.0 ** -21), torch.tensor([1.0], dtype=torch.float64) / 3, "x")


def _pro(i, mode, rd, N, HW, K):
    a = i.a.view(N, HW, K)
    a2 = None if i.a2 is None else i.a2.view(N, HW, K)
    return R.prologue(a, mode, rd, R.ACT_NONE, i.coef, a2, i.gate)


@pytest.mark.parametrize("rd", E.DTYPES)
@pytest.mark.parametrize("ci", range(len(E.PW_FWD_CASES)))
def test_pwconv_forward(ci, rd):
    for mode in E.pw_modes(E.PW_FWD_CASES[ci][0]):
        c = E.pw_fwd(ci, mode)
        N, HW, K, No = c.shape
        A = _pro(c, mode, rd, N, HW, K)
        same(A, c.A, f"{c.what}: oracle prologue")
        out = R.rnd(A.reshape(N, HW, 1, K) @ R.rnd(c.w, rd).t(), rd)
        same(out, c.out, f"{c.what}: oracle product")
        same(R.stats_sums(out), c.sums, f"{c.what}: oracle statistics")
        same(R.rnd(out + c.res, rd), c.out_res, f"{c.what}: oracle residual")


def _wgrad(c, pmode, qmode, rd):
    N, HW, Ni, Nj = c.shape
    P, Q = _pro(c.p, pmode, rd, N, HW, Ni), _pro(c.q, qmode, rd, N, HW, Nj)
    same(P, c.P, f"{c.what}: oracle prologue of p")
    same(Q, c.Q, f"{c.what}: oracle prologue of q")
    same(P.reshape(-1, Ni).t() @ Q.reshape(-1, Nj), c.dw, f"{c.what}: f32 product")


@pytest.mark.parametrize("rd", E.DTYPES)
@pytest.mark.parametrize("case", E.WGRAD_TILED_CASES)
def test_pwconv_wgrad_tiled(case, rd):
    for pmode, qmode in E.WGRAD_TILED_MODES:
        _wgrad(E.pw_wgrad(case, pmode, qmode), pmode, qmode, rd)


@pytest.mark.parametrize("case", E.WGRAD_LARGE_CASES)
def test_pwconv_wgrad_large_m(case):
    for pmode, qmode in E.WGRAD_LARGE_MODES:
        _wgrad(E.pw_wgrad(case, pmode, qmode, True), pmode, qmode, BF16)


@pytest.mark.parametrize("case", E.FUSED_CASES)
def test_fused_expand_backward(case):
    c = E.pw_fused(case)
    M, Cm, Cin = case
    d = R.prologue(c.dz.view(1, M, Cm), 3, BF16, coef=c.coef, a2=c.y.view(1, M, Cm))[0]
    same(d, c.d, f"{c.what}: oracle BN-backward map")
    dx = R.rnd(d @ R.rnd(c.w, BF16), BF16)
    same(dx, c.dx.view(M, Cin), f"{c.what}: dx")
    same(R.rnd(dx + c.res.view(M, Cin), BF16), c.dx_res.view(M, Cin), f"{c.what}: dx + residual")
    same(d.t() @ c.x.view(M, Cin), c.dw, f"{c.what}: dw")


@pytest.mark.parametrize("rd", E.DTYPES)
@pytest.mark.parametrize("case", E.DW_CASES + [E.DW_SQUEEZED_CASE])
def test_depthwise(case, rd):
    c = E.dw(case)
    N, H, W, C, k, s, pt, pl = case
    y = R.dwconv_fwd(c.x, c.st, R.ACT_NONE, c.w, k, s, pt, pl, c.Ho, c.Wo, rd)
    same(y, c.y, f"{c.what}: oracle forward with the BN prologue")
    same(R.dwconv_fwd(c.xt, None, R.ACT_NONE, c.w, k, s, pt, pl, c.Ho, c.Wo, rd), c.y, f"{c.what}: oracle forward")
    same(R.stats_sums(y), c.y_sums, f"{c.what}: oracle statistics")
    dy = R.rnd(c.coef[0] * c.dz + c.coef[1] * c.yraw + c.coef[2], rd)
    same(dy, c.dyt, f"{c.what}: BN-backward map")
    da, dw = R.dwconv_bwd(dy, R.rnd(c.st[0] * c.x + c.st[1], rd), c.w, k, s, pt, pl, rd)
    same(R.rnd(da * R.act_grad(c.x, R.ACT_NONE), rd), c.dzin, f"{c.what}: oracle data gradient")
    same(dw, c.dw, f"{c.what}: oracle weight gradient")
    xhat = (c.x - c.st[2]) * c.st[3]
    got = torch.stack([da.reshape(-1, C).sum(0), (da * xhat).reshape(-1, C).sum(0)])
    same(got, c.dzin_sums, f"{c.what}: f32 sums of the data gradient")


@pytest.mark.parametrize("rd", E.DTYPES)
@pytest.mark.parametrize("pad", E.STEM_PADS)
@pytest.mark.parametrize("case", E.STEM_CASES)
def test_stem(case, pad, rd):
    c = E.stem(case, pad)
    y = R.stem_conv_fwd(c.x, c.w, 2, pad[0], pad[1], c.Ho, c.Wo, rd)
    same(y, c.y, f"{c.what}: oracle forward")
    same(R.stats_sums(y), c.y_sums, f"{c.what}: oracle statistics")
    dy = R.rnd(c.coef[0] * c.dz + c.coef[1] * c.yraw + c.coef[2], rd)
    same(dy, c.dyt, f"{c.what}: BN-backward map")
    same(R.stem_conv_wgrad(c.x, dy, 3, 2, pad[0], pad[1], rd), c.dw, f"{c.what}: oracle weight gradient")


@pytest.mark.parametrize("rd", E.DTYPES)
@pytest.mark.parametrize("case", E.ROW_CASES)
def test_row_passes(case, rd):
    c = E.rows(case)
    N, H, W, C = case
    M = N * H * W
    ones = torch.ones(C)
    # R.bn_bwd_coef returns (coef, sum g*xhat, sum g): the two sums bn_bwd_reduce leaves in its partial rows
    for g, want in ((c.g, c.red), (c.g * c.rs[:, None, None, None], c.red_rs)):
        _, s2, s1 = R.bn_bwd_coef(R.rnd(g, rd), R.rnd(c.y, rd), ones, c.st)
        same(torch.stack([s1, s2]), want, f"{c.what}: oracle BN-backward sums")
    same(c.g.sum((0, 1, 2)), c.bias, f"{c.what}: bias gradient")
    z = c.st[0] * c.y + c.st[1]
    a = R.rnd(R.act_fwd(z, R.ACT_NONE), rd)
    same(a, c.at, f"{c.what}: oracle activation")
    same((a * c.g).sum((1, 2)), c.pool_bwd, f"{c.what}: pool backward")
    E.within_one_ulp(a.mean((1, 2)), c.pooled, f"{c.what}: pooled mean")
    for mode, da in enumerate([c.g, c.g * c.gate[:, None, None, :] + c.dpool[:, None, None, :] / (H * W),
                               (c.dpool[:, None, None, :] / (H * W)).expand(N, H, W, C)]):
        same(R.rnd(da * R.act_grad(z, R.ACT_NONE), rd), c.dz[mode], f"{c.what}: act_bn_bwd mode {mode}")
    same(R.stats_sums(c.g), c.g_stats, f"{c.what}: channel statistics")
    assert M == c.g.numel() // C


@pytest.mark.parametrize("P", E.SUM_ROWS_P)
def test_sum_rows_and_grad_sumsq(P):
    c = E.sum_rows(P)
    same(c.parts[:P].sum(0), c.want, "sum_rows")
    same(c.pre + c.parts[:P].sum(0), c.want_acc, "sum_rows accumulate")
    g = E.grad_sumsq()
    assert [t.numel() for t in g.gs] == list(E.GRAD_SUMSQ_SIZES)
    got = [(t[off:off + g.chunk] * t[off:off + g.chunk]).sum() for t in g.gs for off in range(0, t.numel(), g.chunk)]
    same(torch.stack(got), g.want, "grad_sumsq: f32 sums of squares per table row")


@pytest.mark.parametrize("rd", E.DTYPES)
@pytest.mark.parametrize("case", E.CONV_CASES)
def test_dense_convolution(case, rd):
    c = E.conv(case)
    k, s, p, C, Co, H, N = case
    a = R.rnd(c.st[0] * c.x + c.st[1], rd)
    same(a, c.xt, f"{c.what}: oracle prologue")
    y = R.rnd(F.conv2d(a.permute(0, 3, 1, 2), R.rnd(c.w, rd), stride=s, padding=p).permute(0, 2, 3, 1), rd)
    same(y, c.y, f"{c.what}: conv2d")
    same(R.stats_sums(y), c.y_sums, f"{c.what}: oracle statistics")
    P = R.prologue(c.p.view(1, -1, Co), 3, rd, coef=c.coef, a2=c.p2.view(1, -1, Co))[0]
    same(P, c.pt.view(-1, Co), f"{c.what}: oracle BN-backward map")
    col = E.im2col64(a.double(), k, s, p, c.Ho).float()
    same(P.t() @ col.reshape(-1, k * k * C), c.dw, f"{c.what}: f32 weight gradient")
    xz = torch.zeros((N, H, H, C), requires_grad=True)               # col2im is the adjoint of im2col: autograd of F.unfold in f32
    (E.im2col64(xz, k, s, p, c.Ho) * c.dcol).sum().backward()
    same(xz.grad, c.dx, f"{c.what}: col2im as the gradient of im2col")


def test_vit_matrix_products():
    b = E.bgemm()
    S = b.q @ b.k.transpose(-1, -2)
    same(S, b.S, "bgemm q k^T")
    same(S @ b.v, b.O, "bgemm S v")
    for case in E.ATTN_APPLY_CASES:
        c = E.attn_apply(case)
        B, H, To, Tc, D = case
        heads = lambda t, T: t.view(B, T, H, D).permute(0, 2, 1, 3)
        back = lambda t, T: t.permute(0, 2, 1, 3).reshape(B, T, 1, H * D)
        same(R.rnd(back(0.5 * (R.rnd(c.f, BF16) @ heads(c.x, Tc)), To), BF16), c.out, f"attn_apply {case}")
        same(R.rnd(back(0.5 * (R.rnd(c.f, BF16).transpose(-1, -2) @ heads(c.g, To)), Tc), BF16), c.out_t, f"attn_apply^T {case}")
    g = E.gemm_bias_act()
    y = R.rnd(g.a @ g.w.t(), BF16)
    same(y, g.y, "gemm_bias_act product")
    M = y.shape[0]
    same(R.rnd((g.st[0] * y + g.st[1]) * g.rs.view(M, 1, 1, 1) + g.res, BF16), g.out, "gemm_bias_act epilogue")
    v = E.vit_small()
    same(F.avg_pool2d(v.x.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1), v.pooled, "avgpool forward")
    xr = v.x.permute(0, 3, 1, 2).clone().requires_grad_()
    F.avg_pool2d(xr, 2, 2).backward(v.gp.permute(0, 3, 1, 2))
    same(xr.grad.permute(0, 2, 3, 1), v.dpool, "avgpool backward")
    same(v.gt.sum(0).view(49, 64), v.rowtable, "rowtable_grad")
    same(torch.zeros(v.H, v.n).index_add_(1, v.idx.long(), v.dfull), v.scat, "bias_scatter")
    t = torch.zeros(v.T, v.H, requires_grad=True)
    (16 * torch.sigmoid(t[v.ridx.long()].view(v.nl, v.nl, v.H).permute(2, 0, 1))).backward(v.dbias[:, v.ng:, v.ng:])
    same(t.grad, v.dtable, "relpos_bias_bwd at table = 0")


@pytest.mark.parametrize("case", E.LINEAR_CASES)
def test_linear_head(case):
    """test_linear_is_exact of tests/test_exact_gpu.py: the builder has checked that every sum stays exact in f32; plain f32 torch agrees."""
    l = E.linear(case)
    same(F.linear(l.x, l.w, l.b), l.out, f"linear_fwd {case}")
    same(l.dout @ l.w, l.dx, f"linear dx {case}")
    same(l.dout.t() @ l.x, l.dw, f"linear dw {case}")
    same(l.dout.sum(0), l.db, f"linear db {case}")


def _mlp32(c):
    """Plain f32 torch on the data of one coordinate-MLP job: (table, dw0, db0, dw2)."""
    w0, b0, w2 = (t.clone().requires_grad_(True) for t in (c.w0, c.b0, c.w2))
    table = torch.relu(c.coords @ w0.t() + b0) @ w2.t()
    return table, w0, b0, w2


@pytest.mark.parametrize("ci", E.COORD_CASES)
def test_coord_mlp(ci):
    """tests/test_coord_gpu.py: the f32 evaluation of the same data reproduces float64, ReLU boundary included."""
    c = E.coord_mlp(ci)
    table, w0, b0, w2 = _mlp32(c)
    table.backward(c.dtable)
    same(table, c.table, f"{c.what}: f32 table")
    same(w0.grad, c.dw0, f"{c.what}: f32 dw0")
    same(b0.grad, c.db0, f"{c.what}: f32 db0")
    same(w2.grad, c.dw2, f"{c.what}: f32 dw2")
    T, D, Hd = c.shape
    assert c.zeros > 0 or T * Hd < 1000
    assert (c.coords.shape, c.w0.shape, c.b0.shape, c.w2.shape, c.dtable.shape) == ((T, 2), (Hd, 2), (Hd,), (D, Hd), (T, D))


def test_coord_mlp_on_the_carrier_grid_through_the_oracle():
    """The 4 x 4 grid's coordinates are multiples of 1/2, so the oracle's own PosEmb1D (which builds them itself) is exact there."""
    from oracle.fastervit_ref import PosEmb1D

    c = E.coord_mlp(E.COORD_GRID16)
    T, D, _ = c.shape
    pe = PosEmb1D(D, T)
    with torch.no_grad():
        pe.cpb_mlp[0].weight.copy_(c.w0), pe.cpb_mlp[0].bias.copy_(c.b0), pe.cpb_mlp[2].weight.copy_(c.w2)
    x = torch.zeros(1, T, D)
    out = pe(x)[0]
    out.backward(c.dtable)
    same(out, c.table, "PosEmb1D table on the 4 x 4 grid")
    same(pe.cpb_mlp[0].weight.grad, c.dw0, "PosEmb1D dw0")
    same(pe.cpb_mlp[0].bias.grad, c.db0, "PosEmb1D db0")
    same(pe.cpb_mlp[2].weight.grad, c.dw2, "PosEmb1D dw2")
    from deepfakedetection_amd.fastervit import PosEmbMLPSwinv1D

    same(PosEmbMLPSwinv1D(D, T)._coords, c.coords, "the project's coordinate buffer of the 4 x 4 grid")


@pytest.mark.parametrize("gi", range(len(E.CPB_GEOMS)))
def test_coord_cpb_chain(gi):
    """The whole chain in plain f32 torch: table exactly 0, bias 8 / 0, dtable = 4 scatter(dbias) and zero in rows the index never
    names, and the MLP gradients from there; the saturated table gives 0 / 16 by the gathered row."""
    c = E.coord_cpb(gi)
    nl, ng, T, H = c.geom
    table, w0, b0, w2 = _mlp32(c)
    table.retain_grad()
    local = 16 * torch.sigmoid(table[c.idx.long()].view(nl, nl, H).permute(2, 0, 1))
    bias = F.pad(local, (ng, 0, ng, 0))
    bias.backward(c.dbias)
    same(table, c.table, f"{c.what}: f32 table")
    assert float(table.detach().abs().max()) == 0.0
    same(bias, c.bias, f"{c.what}: f32 bias")
    same(table.grad, c.dtable, f"{c.what}: f32 dtable")
    assert float(table.grad[~c.used].abs().max() if bool((~c.used).any()) else 0.0) == 0.0
    same(w0.grad, c.dw0, f"{c.what}: f32 dw0")
    same(b0.grad, c.db0, f"{c.what}: f32 db0")
    same(w2.grad, c.dw2, f"{c.what}: f32 dw2")
    sat = F.pad(16 * torch.sigmoid(c.sat_table[c.idx.long()].view(nl, nl, H).permute(2, 0, 1)), (ng, 0, ng, 0))
    same(sat, c.sat_bias, f"{c.what}: f32 bias of the saturated table")
    if c.geom[:2] == (49, 4) and bool(c.used.all()):
        from deepfakedetection_amd.fastervit import PosEmbMLPSwinv2D

        assert torch.equal(PosEmbMLPSwinv2D(7, H, nl + ng)._idx32, c.idx), "the project's index buffer of the 7 x 7 window"


def test_coord_shipped_geometry_is_well_conditioned():
    """The condition of the tolerance test at the shipped geometries (tests/test_coord_gpu.py): at the recorded seed no ReLU unit of
    the six modules sits within f32 rounding of 0 - and the check does raise where one does."""
    jobs = E.coord_shipped()
    assert [j.spec for j in jobs] == E.SHIPPED_POS + E.SHIPPED_CPB
    assert all(j.margin > 1.0 for j in jobs)
    j = jobs[0]
    w0, b0 = j.w0.clone(), j.b0.clone()
    b0[5] = -(j.coords[3].double() @ w0[5].double()).float()                # unit 5 at row 3: the pre-activation is rounding only
    with pytest.raises(E.ConditionViolated, match="within f32 rounding of 0"):
        E.relu_margin("planted", j.coords, w0, b0)


@pytest.mark.parametrize("ci", range(len(E.ROUND_PW_CASES)))
def test_rounding_data_of_the_1x1_forward(ci):
    """The builder asserts the conditions (40 % of the outputs would differ under truncation, 16 ties or more of both kinds); here
    the f32 product of the same operands, rounded by torch, is the reference bit for bit."""
    c = E.round_pw(ci)
    M, K, No = c.shape
    out = (c.a.view(M, K) @ c.w.t()).to(BF16)                   # one nonzero term per sum: the f32 product is exact
    E.same_bits(out.view(1, M, 1, No), c.want, f"rounding data {c.tier}")


def test_rounding_data_of_the_row_kernels():
    c = E.round_rows()
    E.same_bits((c.x * c.chan).to(BF16), c.by_chan, "per-channel")
    E.same_bits((c.x * c.img[:, None, None, None]).to(BF16), c.by_img, "per-image")
    E.same_bits((c.x * c.img_chan[:, None, None, :]).to(BF16), c.by_img_chan, "per-(image, channel)")
    trunc = E.truncate_bf16(c.x * c.chan).to(BF16)
    with pytest.raises(AssertionError, match="differ from round-to-nearest-even"):
        E.same_bits(trunc, c.by_chan, "a truncating store")
