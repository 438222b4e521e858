"""The CPU twin of tests/test_vit_edges_gpu.py: needs no GPU.

Runs every builder of tests/_vit_cases.py (so every check_exact declaration is evaluated here), holds each hand-written reference
against torch's own operator at the case shapes (the up2 tap table against nn.Upsample, the avgpool coverage mask against autograd,
im2col / col2im against F.unfold / F.fold and against each other through autograd), and checks the case tables: every declared launch
shape follows from the restated rules AND from the library's host-side query dfd_rowtable_grad_plan, every cap case really passes
16384 * 256 vectors with its last image behind the first pass, and no case but the stated one needs more than about 300 MB.
"""

from __future__ import annotations

import ctypes

import pytest
import torch
import torch.nn.functional as F

from deepfakedetection_amd import _lib
from oracle import ops_ref as R
from tests import _vit_cases as V
from tests._exact import BF16, DTYPES, F32, same

DT_CODE = {F32: _lib.F32, BF16: _lib.BF16}
EINVAL = -1


def plan(rd, rows, T, C):
    s, w, r = ctypes.c_int(-1), ctypes.c_long(-1), ctypes.c_int(-1)
    code = _lib.load().dfd_rowtable_grad_plan(DT_CODE[rd], rows, T, C, ctypes.byref(s), ctypes.byref(w), ctypes.byref(r))
    return code, (s.value, w.value, r.value)


# --------------------------------------------------------------------------------------------------------------- rowtable plan
def test_abi_149_exports():
    lib = _lib.load()
    assert lib.dfd_version() >= 149
    assert lib.dfd_rowtable_grad_plan(_lib.F32, 49, 49, 64, None, None, None) == 0           # null outputs are allowed
    for what, args in {"rows = 0": (_lib.F32, 0, 1, 8), "T = 0": (_lib.F32, 8, 0, 8), "rows % T": (_lib.F32, 50, 49, 8),
                       "C = 0": (_lib.F32, 49, 49, 0), "C = 6 in f32": (_lib.F32, 49, 49, 6), "C = 4 in bf16": (_lib.BF16, 49, 49, 4),
                       "dtype 2": (2, 49, 49, 8)}.items():
        assert lib.dfd_rowtable_grad_plan(*args, None, None, None) == EINVAL, what


@pytest.mark.parametrize("i", range(len(V.ROWTABLE_CASES)))
def test_rowtable_case_has_its_plan(i):
    c = V.ROWTABLE_CASES[i]
    assert plan(c.rd, c.nw * c.T, c.T, c.C) == (0, c.plan), c.note
    assert V.rowtable_rule(c.nw, c.T, c.C, V.VEC[c.rd]) == c.plan + (c.limiter,), c.note
    assert V.rowtable(i).dtable.shape == (c.T, c.C)


def test_rowtable_plan_is_the_restated_rule():
    for rd in DTYPES:
        for C in (4, 8, 24, 64, 264, 520, 536, 1024):
            if C % V.VEC[rd]:
                continue
            for T in (1, 3, 16, 49, 50, 700, 2049):
                for nw in (1, 6, 27, 28, 127, 128, 255, 256, 259, 588, 4096, 4229, 70000):
                    assert plan(rd, nw * T, T, C) == (0, V.rowtable_rule(nw, T, C, V.VEC[rd])[:3]), (rd, nw, T, C)


def test_rowtable_table_reaches_every_tier():
    by = {(c.nw, c.T, c.C, c.rd): c for c in V.ROWTABLE_CASES}
    lanes = lambda c: V.rowtable_lanes(c.nw, *c.plan)
    assert lanes(by[6, 49, 64, BF16]) == [(6, 0, 6)]                                          # tail loop only, 26 row lanes without a window
    assert lanes(by[127, 3, 64, BF16]) == [(127, 31, 1)]                                      # lane 31 alone skips the unrolled loop
    assert lanes(by[256, 3, 64, BF16]) == [(128, 32, 0)] * 2
    assert lanes(by[259, 3, 64, BF16]) == [(130, 32, 0), (129, 32, 0)]                        # w_end clipped to nw
    last = lanes(by[4101, 16, 64, BF16])
    assert len(last) == 32 and last[0] == (129, 32, 0) and last[-1] == (102, 6, 26)
    assert 4229 // 128 == 33 and lanes(by[4229, 16, 64, BF16])[-1][0] == 4229 - 31 * 133
    assert V.chanmap(264, 4) == (33, 7, 2) and 33 * 7 == 231                                  # 25 idle threads, blockIdx.y in {0, 1}
    assert lanes(by[60, 50, 264, F32]) == [(30, 7, 0)] * 2
    grid = lanes(by[588, 50, 264, F32])
    assert 2048 // (50 * 2) == 20 < 588 // 28 and len(grid) == 20 and grid[-1][0] == 18
    assert V.chanmap(4, 4) == (1, 256, 1) and V.chanmap(8, 8) == (1, 256, 1)
    assert {c.limiter for c in V.ROWTABLE_CASES} == {"one", "windows", "cap", "grid"}
    assert 60 * 50 * 264 * 4 < V.BUDGET_BYTES and 588 * 50 * 264 * 4 < V.BUDGET_BYTES


# ------------------------------------------------------------------------------------------------------------ reducing kernels
def test_reduce_widths_follow_make_chanmap():
    for C, maps in V.REDUCE_WIDTHS.items():
        for rd in DTYPES:
            assert V.chanmap(C, V.VEC[rd]) == maps[rd], (C, rd)
    assert V.REDUCE_WIDTHS[224][BF16][0] * V.REDUCE_WIDTHS[224][BF16][1] == 252               # 4 idle lanes
    assert {r for C, rd, r in V.REDUCE_CASES if (C, rd) == (224, BF16)} == {1, 8, 37, 600}
    assert {r for C, rd, r in V.REDUCE_CASES if (C, rd) == (1024, F32)} == {1, 3, 17, 600}
    assert V.nparts_rule(600, 4) == 38 and V.nparts_rule(600, 256) == 1 and V.nparts_rule(37, 9) == 2 and V.nparts_rule(8, 9) == 1
    assert V.nparts_rule(10 ** 7, 4) == 1024


@pytest.mark.parametrize("C,rows", sorted({(C, rows) for C, _, rows in V.REDUCE_CASES}))
def test_reduce_exact_data_in_f32(C, rows):
    c = V.reduce_exact(C, rows)
    y, g = c.y.view(rows, C), c.g.view(rows, C)
    same(torch.stack([y.sum(0), (y * y).sum(0)]), c.stats, c.what + " stats")
    xhat = (y - c.st[2]) * c.st[3]
    same(torch.stack([g.sum(0), (g * xhat).sum(0)]), c.sums, c.what + " sums")
    same(R.rnd(c.g, BF16), c.d, c.what + " d in bf16")


# ------------------------------------------------------------------------------------------------------------------------- up2
@pytest.mark.parametrize("h", sorted({s[1] for s in V.UP2_SHAPES} | {s[2] for s in V.UP2_SHAPES}))
def test_up2_tap_table_is_nn_upsample(h):
    eye = torch.eye(h, dtype=torch.float64).view(h, 1, h, 1)                                  # h one-hot columns as images [h, 1, h, 1]
    up = torch.nn.Upsample(scale_factor=(2, 1), mode="bilinear")(eye)                         # [h, 1, 2h, 1]
    same(V.up2_matrix(h), up[:, 0, :, 0].t(), f"up2 taps, h = {h}")
    assert bool((V.up2_matrix(h).sum(1) == 1).all())
    if h == 1:
        assert V.up2_taps(0, 1)[:2] == (0, 0) and V.up2_taps(1, 1)[:2] == (0, 0)              # both taps clamp to the same row


@pytest.mark.parametrize("shape", V.UP2_SHAPES)
def test_up2_references(shape):
    c = V.up2_exact(shape)
    sn = c.s.double().permute(0, 3, 1, 2).clone().requires_grad_()
    up = torch.nn.Upsample(scale_factor=2, mode="bilinear")(sn)
    up.backward(c.g.double().permute(0, 3, 1, 2))
    same(up.detach().permute(0, 2, 3, 1), c.out, c.what + " forward")
    same(sn.grad.permute(0, 2, 3, 1), c.ds, c.what + " backward")
    for act in (V.ACT_GELU, V.ACT_SILU):
        gc = V.up2_gauss(shape, F32, act)
        sn = gc.s.double().permute(0, 3, 1, 2).clone().requires_grad_()
        ref = R.act_fwd(torch.nn.Upsample(scale_factor=2, mode="bilinear")(sn), act)
        ref.backward(gc.g.double().permute(0, 3, 1, 2))
        assert torch.allclose(ref.detach().permute(0, 2, 3, 1), gc.out, rtol=0, atol=1e-12)
        assert torch.allclose(sn.grad.permute(0, 2, 3, 1), gc.ds, rtol=0, atol=1e-12)


# ----------------------------------------------------------------------------------------------------- subsample and avgpool
@pytest.mark.parametrize("case", V.SUBSAMPLE_CASES)
def test_subsample_references(case):
    N, H, W, s, C = case
    c = V.subsample(case)
    xn = c.x.double().permute(0, 3, 1, 2)
    same(c.a.double() + c.bias.double() + F.avg_pool2d(xn, 1, s).permute(0, 2, 3, 1), c.out_b, c.what)           # nn.AvgPool2d(1, s, 0)
    assert torch.equal(c.dx1[:, ~c.lattice], c.dx0.double()[:, ~c.lattice]), c.what + ": the reference changes a pixel off the lattice"
    assert not torch.equal(c.dx1[:, c.lattice], c.dx0.double()[:, c.lattice])
    assert bool(c.lattice[H - 1].any()) == ((H - 1) % s == 0)                                  # H = m s + 1: the last row is sampled


@pytest.mark.parametrize("case", V.AVGPOOL_CASES)
def test_avgpool_references(case):
    N, H, W, k, s, C = case
    c = V.avgpool(case)
    ones = torch.ones(1, c.Ho, c.Wo, 1, dtype=torch.float64)
    hit = V.avgpool64(torch.zeros(1, H, W, 1), ones, k, s)[1][0, :, :, 0] != 0                 # autograd: pixels that receive a gradient
    assert torch.equal(hit, c.covered), c.what
    assert bool((c.dx[:, ~c.covered] == 0).all())
    if c.exact:
        same(F.avg_pool2d(c.x.permute(0, 3, 1, 2), k, s).permute(0, 2, 3, 1), c.out, c.what + " in f32")


def test_avgpool_table_reaches_its_edges():
    cov = {case: V.avgpool(case).covered for case in V.AVGPOOL_CASES}
    full = lambda m: bool(m.all())
    assert full(cov[2, 14, 14, 5, 3, 32]) and full(cov[1, 8, 8, 2, 2, 16]) and full(cov[1, 6, 6, 1, 1, 8]) and full(cov[2, 5, 5, 5, 3, 8])
    m = cov[1, 15, 16, 5, 3, 8]
    assert full(m[:14, :14]) and not bool(m[14].any()) and not bool(m[:, 14:].any())
    m = cov[1, 9, 9, 4, 2, 8]
    assert full(m[:8, :8]) and not bool(m[8].any()) and not bool(m[:, 8].any())
    assert V.avgpool((1, 7, 7, 3, 1, 8)).Ho == 5


# ------------------------------------------------------------------------------------------------------------ bookkeeping data
@pytest.mark.parametrize("C", V.COPY_C)
@pytest.mark.parametrize("n", V.COPY_N)
def test_copy_rows_cases(C, n):
    for mode in V.COPY_MODES:
        c = V.copy_rows(C, n, mode)
        written = (c.want != V.COPY_FILL).all(1)
        assert int(written.sum()) == n and c.rdst - n == c.untouched and (c.untouched > 0) == (mode in ("didx", "both", "fewer"))
        for idx in (c.sidx, c.didx):
            assert idx is None or (idx.dtype == torch.int32 and len(set(idx.tolist())) == n)


@pytest.mark.parametrize("case", V.ADD_ROWTABLE_CASES)
def test_add_rowtable_cases(case):
    T, nw, C = case
    c = V.add_rowtable(case)
    rows = c.x.view(nw * T, C)
    same(rows + c.tab[torch.arange(nw * T) % T], c.out.view(nw * T, C), f"add_rowtable {case}: row r takes table row r mod T")


@pytest.mark.parametrize("case", V.BIAS_CASES)
def test_bias_cases(case):
    H, T, L = case
    c = V.bias(case)
    t = c.table.clone().requires_grad_()
    t[:, c.idx.long()].backward(c.dfull)
    same(t.grad, c.dtable, c.what)
    assert (T == 1) == bool(c.used.all())


@pytest.mark.parametrize("case", V.RELPOS_CASES)
def test_relpos_cases(case):
    H, nl, ng, T = case
    c = V.relpos(case)
    t0 = torch.zeros(T, H, dtype=torch.float64, requires_grad=True)
    b = 16 * torch.sigmoid(t0[c.idx.long()].view(nl, nl, H).permute(2, 0, 1))
    b.backward(c.dfull.double()[:, ng:, ng:])
    same(t0.grad, c.dtable, c.what + ": the derivative at table = 0 is 4")
    assert bool((c.dtable[~c.used] == 0).all()) and (T == 1) == bool(c.used.all())
    assert bool((c.full[:, :ng] == 0).all()) and bool((c.full[:, :, :ng] == 0).all())
    assert ((T * H) % 4 != 0) == (case != V.RELPOS_CASES[0])


# ------------------------------------------------------------------------------------------------------------- im2col / col2im
@pytest.mark.parametrize("i", range(len(V.IM2COL_CASES)))
def test_im2col_references(i):
    k, s, pt, pl, C, H, N, (Ho, Wo) = V.IM2COL_CASES[i]
    c = V.im2col(i)
    xn = c.x.double().clone().requires_grad_()
    V.im2col64(xn, k, s, pt, pl, Ho, Wo).backward(c.dcol.double())
    same(xn.grad, c.dx, c.what + ": col2im is the transpose of im2col")
    full = ((H + 2 * pt - k) // s + 1, (H + 2 * pl - k) // s + 1)
    if pt == pl and (Ho, Wo) == full:
        unf = F.unfold(c.x.double().permute(0, 3, 1, 2), k, padding=pt, stride=s)
        same(unf.view(N, C, k * k, Ho, Wo).permute(0, 3, 4, 2, 1).reshape(N, Ho, Wo, k * k * C), c.col, c.what + " against F.unfold")
        back = c.dcol.double().view(N, Ho * Wo, k * k, C).permute(0, 3, 2, 1).reshape(N, C * k * k, Ho * Wo)
        same(F.fold(back, (H, H), k, padding=pt, stride=s).permute(0, 2, 3, 1), c.dx, c.what + " against F.fold")
    else:
        assert (Ho, Wo) == full or (Ho + 1, Wo + 1) == full


def test_im2col_table_has_the_listed_geometries():
    keys = {(k, s, pt, pl) for k, s, pt, pl, *_ in V.IM2COL_CASES}
    assert {(5, 1, 2, 2), (7, 2, 3, 3), (3, 3, 0, 0), (3, 4, 1, 1), (3, 2, 0, 1), (3, 2, 1, 1), (3, 1, 1, 1)} <= keys
    assert not V.conv_shape_ok(8, 1, 1, 1, 8, 9, 9, 1, 4, 4) and not V.conv_shape_ok(3, 5, 1, 1, 8, 9, 9, 1, 2, 2)
    assert not V.conv_shape_ok(3, 2, 1, 1, 8, 12, 12, 1, 8, 6) and V.conv_shape_ok(3, 2, 1, 1, 8, 12, 12, 1, 7, 6)


@pytest.mark.parametrize("case", V.PERM_CASES)
def test_weight_perm_references(case):
    O, I, k = case
    c = V.weight_perm(case)
    for o in range(O):
        for i in range(I):
            for kh in range(k):
                for kw in range(k):
                    assert c.to_gemm[o, (kh * k + kw) * I + i] == c.w[o, i, kh, kw]
                    assert c.dgrad[i, ((k - 1 - kh) * k + (k - 1 - kw)) * O + o] == c.w[o, i, kh, kw]


# ------------------------------------------------------------------------------------------------------------------ cap cases
@pytest.mark.parametrize("name", list(V.CAP_CASES))
def test_cap_case_passes_the_first_grid_pass(name):
    c = V.CAP_CASES[name]
    total = V.cap_total(name)
    assert total > V.FIRST_PASS == 4194304 and V.grid_rule(total) == V.GRID_CAP
    assert (c.N - 1) * c.per_image >= V.FIRST_PASS > (c.N - 2) * c.per_image                  # the smallest N with the last image behind it
    assert (c.bytes <= V.BUDGET_BYTES) == (name not in V.CAP_OVER_BUDGET) and c.bytes <= 6 * 2 ** 26 + 192
