"""The small spatial and token-bookkeeping kernels of csrc/dfd_vit.hip at their edges and launch tiers.  Data, launch shapes and
float64 references: tests/_vit_cases.py; the CPU twin that checks the data's own conditions, the references and the tables on any
machine: tests/test_vit_edges_cpu.py.

Integer data are compared at tolerance 0 (tests/_exact.py, `same`).  Everything with GELU or SiLU, pooling with k = 3 or 5,
relpos_bias_fwd and the BN prologue of im2col are held to the bounds tests/test_vit_ops_gpu.py states for this family, relative to the
reference's largest magnitude: 2e-4 in f32, 1.6e-2 in bf16, 5e-4 / 5e-3 for per-channel sums.  Every rowtable case first asserts the
launch shape it is listed under through dfd_rowtable_grad_plan, every reducing case the number of partial rows the kernel reports,
every cap case that its grid is at the cap: a changed dispatch fails here instead of silently moving a case to another branch.
"""

from __future__ import annotations

import ctypes

import pytest
import torch

from tests import _vit_cases as V
from tests._exact import BF16, DTYPES, F32, same

pytestmark = pytest.mark.gpu

EINVAL, EWORKSPACE = -1, -4
RD = pytest.mark.parametrize("rd", DTYPES, ids=["f32", "bf16"])


def _k():
    from deepfakedetection_amd import kernels

    return kernels


def dev(t, rd=None):
    if t is None:
        return None
    return (t if rd is None else t.to(rd)).cuda().contiguous()


def close(got, want64, rel, what):
    g, w = got.detach().double().cpu(), want64.double()
    assert g.shape == w.shape, f"{what}: shape {tuple(g.shape)} vs {tuple(w.shape)}"
    scale = max(float(w.abs().max()), 1e-6)
    err = float((g - w).abs().max()) / scale
    assert err <= rel, f"{what}: max err {err:.3e} of max |ref| {scale:.3e} > {rel:.1e}"


def _guarded(values, fill, guard=V.GUARD):
    """(view of `values` inside a larger buffer, the buffer): `guard` elements of `fill` in front of and behind the tensor.  What a
    launch reads past an end is then a known value that spoils its result, and what it writes there is found by _guard_intact."""
    n = values.numel()
    buf = torch.full((n + 2 * guard,), fill, dtype=values.dtype, device="cuda")
    view = buf[guard:guard + n].view(values.shape)
    view.copy_(values)
    return view, buf


def _guard_intact(buf, fill, what, guard=V.GUARD):
    assert bool((buf[:guard] == fill).all()) and bool((buf[-guard:] == fill).all()), f"{what}: written outside the tensor"


# ----------------------------------------------------------------------------------------------------------------- rowtable_grad
@pytest.mark.parametrize("i", range(len(V.ROWTABLE_CASES)), ids=lambda i: "{0.nw}-{0.T}-{0.C}-{1}".format(V.ROWTABLE_CASES[i], str(V.ROWTABLE_CASES[i].rd)[6:]))
def test_rowtable_grad_at_its_tier(i):
    K = _k()
    c = V.rowtable(i)
    nw, T, C, rd = c.case.nw, c.case.T, c.case.C, c.case.rd
    assert K.rowtable_grad_plan(rd, nw * T, T, C) == c.case.plan, f"{c.what}: another launch shape serves this case now ({c.case.note})"
    # g sits in front of as many windows of ones as the splits' common length reaches past the last window: a split that is not
    # clipped to nw reads them
    splits, w_per, _ = c.case.plan
    g, _ = _guarded(dev(c.g, rd), 1.0, guard=(splits * w_per - nw) * T * C + V.GUARD)
    same(K.rowtable_grad(g, T), c.dtable, c.what)
    # the raw call on a workspace of its own that starts as garbage: accumulate = 0 twice (same bits), then accumulate = 1
    L, st = K._L(), K._stream()
    nbytes = int(L.dfd_rowtable_grad_ws(T, C))
    ws = torch.full((nbytes // 4,), float("nan"), device="cuda")
    run = lambda out, acc: L.dfd_rowtable_grad(K._dt(rd), K._p(g), K._p(out), nw * T, T, C, acc, K._p(ws), nbytes, st)
    first, second, acc = (torch.full((T, C), 77.0, device="cuda") for _ in range(3))
    assert run(first, 0) == 0 and run(second, 0) == 0
    same(first, c.dtable, c.what + ", raw call")
    assert torch.equal(first, second), f"{c.what}: a second call on the same workspace gives other bits"
    acc.copy_(dev(c.pre))
    assert run(acc, 1) == 0
    same(acc, c.pre.double() + c.dtable, c.what + ", accumulate = 1")


# -------------------------------------------------------------------------------------------------------------- reducing kernels
def _partial_sums(parts, n, C):
    return parts[: n * 2 * C].view(n, 2, C).double().sum(0)


@pytest.mark.parametrize("C,rd,rows", V.REDUCE_CASES, ids=lambda v: str(v)[6:] if isinstance(v, torch.dtype) else str(v))
def test_reducing_kernels_on_every_chanmap(C, rd, rows):
    K = _k()
    c = V.reduce_exact(C, rows)
    cvb, rpb, nvc = V.REDUCE_WIDTHS[C][rd]
    want_n = V.nparts_rule(rows, rpb)
    y, g, other, st = dev(c.y, rd), dev(c.g, rd), dev(c.other, rd), dev(c.st)
    K.partials_buf(y.device, C).fill_(float("nan"))
    parts, n = K.channel_stats(y)
    assert n == want_n, f"{c.what} {rd}: channel_stats reports {n} partial rows, the case is listed under {want_n}"
    same(_partial_sums(parts, n, C), c.stats, f"{c.what} {rd}: channel_stats")
    K.partials_buf(y.device, C).fill_(float("nan"))
    d, parts, n = K.bn_add_act_bwd(g, y, st, other, V.ACT_NONE)
    assert n == want_n, f"{c.what} {rd}: bn_add_act_bwd reports {n} partial rows, the case is listed under {want_n}"
    same(d, c.d, f"{c.what} {rd}: d")
    same(_partial_sums(parts, n, C), c.sums, f"{c.what} {rd}: sums of d and d * xhat")
    d2, _, _ = K.bn_add_act_bwd(g, y, None, None, V.ACT_NONE, stats=False)
    same(d2, c.d, f"{c.what} {rd}: d without state, addend and partial rows")


@RD
@pytest.mark.parametrize("act", V.ACTS3)
@pytest.mark.parametrize("C", list(V.REDUCE_WIDTHS))
def test_bn_add_act_bwd_activations_on_every_chanmap(C, act, rd):
    K = _k()
    c = V.reduce_act(C, rd, act)
    d, parts, n = K.bn_add_act_bwd(dev(c.g), dev(c.y), dev(c.st), dev(c.other), act)
    assert n == V.nparts_rule(V.REDUCE_ROWS_BIG, V.REDUCE_WIDTHS[C][rd][1])
    close(d, c.d, V.TOL[rd], f"bn_add_act_bwd C {C} act {act} {rd}: d")
    got = _partial_sums(parts, n, C)
    close(got[0], c.sums[0], V.TOL_SUMS[rd], "sum d")
    close(got[1], c.sums[1], V.TOL_SUMS[rd], "sum d * xhat")


# ------------------------------------------------------------------------------------------------------------------------- up2
def up2_bwd_raw(K, g, s, act, ws):
    N, h, w, C = s.shape
    ds = torch.full_like(s, 77.0)
    assert K._L().dfd_up2_act_bwd(K._dt(s), K._p(g), K._p(s), act, K._p(ds), N, h, w, C, K._p(ws), K._stream()) == 0
    return ds


@RD
@pytest.mark.parametrize("shape", V.UP2_SHAPES)
def test_up2_clamped_taps_are_exact(shape, rd):
    K = _k()
    c = V.up2_exact(shape)
    s, g = dev(c.s, rd), dev(c.g, rd)
    same(K.up2_act_fwd(s, V.ACT_NONE), c.out, f"{c.what} {rd}: forward")
    same(K.up2_act_bwd(g, s, V.ACT_NONE), c.ds, f"{c.what} {rd}: backward")
    same(up2_bwd_raw(K, g, s, V.ACT_NONE, torch.empty_like(g)), c.ds, f"{c.what} {rd}: backward, a workspace it does not need")


@RD
@pytest.mark.parametrize("act", [V.ACT_GELU, V.ACT_SILU])
@pytest.mark.parametrize("shape", V.UP2_SHAPES)
def test_up2_with_activation_both_backward_paths(shape, act, rd):
    K = _k()
    c = V.up2_gauss(shape, rd, act)
    s, g = dev(c.s), dev(c.g)
    close(K.up2_act_fwd(s, act), c.out, V.TOL[rd], f"up2 {shape} act {act} {rd}: forward")
    two = K.up2_act_bwd(g, s, act)                                             # gq = g act'(up) into a workspace, then the NONE kernel
    one = up2_bwd_raw(K, g, s, act, None)                                      # k_up2_act_bwd<T, ACT>: act' per tap
    close(two, c.ds, V.TOL[rd], f"up2 {shape} act {act} {rd}: two-pass backward")
    close(one, c.ds, V.TOL[rd], f"up2 {shape} act {act} {rd}: single-pass backward")
    if rd == F32:
        close(one, two.double().cpu(), V.TOL[rd], f"up2 {shape} act {act}: the two backward paths against each other")


# ------------------------------------------------------------------------------------------------------------------- subsample
@RD
@pytest.mark.parametrize("case", V.SUBSAMPLE_CASES)
def test_subsample_edges_are_exact(case, rd):
    K = _k()
    N, H, W, s, C = case
    c = V.subsample(case)
    a, (x, _) = dev(c.a, rd), _guarded(dev(c.x, rd), 100.0)
    same(K.subsample_add(a, dev(c.bias), x, s), c.out_b, f"{c.what} {rd}")
    same(K.subsample_add(a, None, x, s), c.out_0, f"{c.what} {rd}: bias = None")
    before = dev(c.dx0, rd)
    dx, buf = _guarded(before, 100.0)
    K.subsample_add_bwd(a, dx, s)
    same(dx, c.dx1, f"{c.what} {rd}: backward")
    _guard_intact(buf, 100.0, f"{c.what} {rd}: backward")
    off = ~c.lattice.cuda()
    assert torch.equal(dx[:, off], before[:, off]), f"{c.what} {rd}: a pixel off the stride lattice changed"


# --------------------------------------------------------------------------------------------------------------------- avgpool
@RD
@pytest.mark.parametrize("case", V.AVGPOOL_CASES)
def test_avgpool_uncovered_and_overlapping_maps(case, rd):
    K = _k()
    N, H, W, k, s, C = case
    c = V.avgpool(case, rd)
    x, g = dev(c.x, rd), dev(c.g, rd)
    out = K.avgpool_fwd(x, k, s)
    dx = torch.full((N, H, W, C), 77.0, dtype=rd, device="cuda")
    assert K._L().dfd_avgpool_bwd(K._dt(rd), K._p(g), K._p(dx), N, H, W, k, s, C, K._stream()) == 0
    if c.exact:
        same(out, c.out, f"{c.what} {rd}: forward")
        same(dx, c.dx, f"{c.what} {rd}: backward")
    else:
        close(out, c.out, V.TOL[rd], f"{c.what} {rd}: forward")
        close(dx, c.dx, V.TOL[rd], f"{c.what} {rd}: backward")
    lost = dx[:, ~c.covered.cuda()]
    assert bool((lost == 0.0).all()), f"{c.what} {rd}: a pixel no window reads has a gradient of {float(lost.abs().max())}"


# ------------------------------------------------------------------------------------------------ copy_rows and add_rowtable
@RD
@pytest.mark.parametrize("n", V.COPY_N)
@pytest.mark.parametrize("C", V.COPY_C)
def test_copy_rows_index_forms(C, n, rd):
    K = _k()
    for mode in V.COPY_MODES:
        c = V.copy_rows(C, n, mode)
        dst = torch.full((c.rdst, C), V.COPY_FILL, dtype=rd, device="cuda")
        K.copy_rows(dev(c.src, rd), dev(c.sidx), dst, dev(c.didx), n)
        same(dst, c.want, f"copy_rows C {C} n {n} {mode} {rd} (rows that are not written keep {V.COPY_FILL})")


@RD
@pytest.mark.parametrize("case", V.ADD_ROWTABLE_CASES)
def test_add_rowtable_is_exact(case, rd):
    K = _k()
    c = V.add_rowtable(case)
    same(K.add_rowtable(dev(c.x, rd), dev(c.tab)), c.out, f"add_rowtable {case} {rd}")


# ----------------------------------------------------------------------------------------------- bias gather / scatter, relpos
@pytest.mark.parametrize("case", V.BIAS_CASES)
def test_bias_gather_scatter_are_exact(case):
    K = _k()
    H, T, L = case
    c = V.bias(case)
    idx, dfull = dev(c.idx), dev(c.dfull)
    same(K.bias_gather(dev(c.table), idx), c.full, c.what + ": gather")
    got = K.bias_scatter(dfull, idx, T, out=torch.full((H, T), 77.0, device="cuda"))
    same(got, c.dtable, c.what + ": scatter")
    assert bool((got[:, ~c.used.cuda()] == 0.0).all()), c.what + ": a table entry no index names is not exactly 0"
    acc = dev(c.pre)
    assert K._L().dfd_bias_scatter(K._p(dfull), K._p(idx), K._p(acc), H, T, L, 1, K._stream()) == 0
    same(acc, c.pre.double() + c.dtable, c.what + ": scatter, accumulate = 1")


@pytest.mark.parametrize("case", V.RELPOS_CASES)
def test_relpos_bias_edges(case):
    K = _k()
    H, nl, ng, T = case
    c = V.relpos(case)
    idx = dev(c.idx)
    full = K.relpos_bias_fwd(dev(c.table), idx, nl, ng)
    close(full, c.full, V.TOL[F32], c.what + ": forward")
    assert bool((full[:, :ng] == 0.0).all()) and bool((full[:, :, :ng] == 0.0).all()), c.what + ": carrier rows / columns are not exactly 0"
    # backward at table = 0 (derivative exactly 4), table and dtable inside guarded buffers: T * H is no multiple of the four waves
    # of a workgroup in three of the four cases, and the idle waves must neither read nor write
    table, _ = _guarded(torch.zeros(T, H), 0.0)
    dtable, dbuf = _guarded(torch.full((T, H), 77.0), 55.0)
    assert K._L().dfd_relpos_bias_bwd(K._p(dev(c.dfull)), K._p(table), K._p(idx), K._p(dtable), H, T, nl, ng, K._stream()) == 0
    same(dtable, c.dtable, c.what + ": backward at table = 0")
    assert bool((dtable[~c.used.cuda()] == 0.0).all()), c.what + ": a table row no index names is not exactly 0"
    _guard_intact(dbuf, 55.0, c.what + ": dtable")


# ------------------------------------------------------------------------------------------------------------- im2col / col2im
def _shape(K, c):
    from deepfakedetection_amd._lib import DwShape

    return DwShape(c.N, c.H, c.H, c.C, c.Ho, c.Wo, c.k, c.s, c.pt, c.pl)


@RD
@pytest.mark.parametrize("i", range(len(V.IM2COL_CASES)), ids=lambda i: "k{0}s{1}p{2}{3}-{5}".format(*V.IM2COL_CASES[i]))
def test_im2col_col2im_geometries(i, rd):
    K = _k()
    c = V.im2col(i)
    L, st, shp = K._L(), K._stream(), _shape(K, c)
    x, dcol = dev(c.x, rd), dev(c.dcol, rd)
    col = torch.full((c.N, c.Ho, c.Wo, c.k * c.k * c.C), 77.0, dtype=rd, device="cuda")
    assert L.dfd_im2col(K._dt(rd), K._p(x), None, V.ACT_NONE, K._p(col), ctypes.byref(shp), st) == 0
    same(col, c.col, f"{c.what} {rd}: im2col")
    dx = torch.full((c.N, c.H, c.H, c.C), 77.0, dtype=rd, device="cuda")
    assert L.dfd_col2im(K._dt(rd), K._p(dcol), K._p(dx), ctypes.byref(shp), st) == 0
    same(dx, c.dx, f"{c.what} {rd}: col2im")
    if c.pt == c.pl:                                                           # the front end takes one padding
        same(K.im2col(x, None, V.ACT_NONE, c.k, c.s, c.pt, c.Ho, c.Wo), c.col, f"{c.what} {rd}: im2col through the front end")
        same(K.col2im(dcol, (c.N, c.H, c.H, c.C), c.k, c.s, c.pt), c.dx, f"{c.what} {rd}: col2im through the front end")
    p = V.im2col_prologue(i, rd)
    col.fill_(77.0)
    assert L.dfd_im2col(K._dt(rd), K._p(dev(p.x)), K._p(dev(p.st)), V.ACT_GELU, K._p(col), ctypes.byref(shp), st) == 0
    close(col, p.col, V.TOL[rd], f"{c.what} {rd}: im2col behind BN + GELU")
    pad = (c.col == 0).cuda() & (p.col == 0).cuda()                            # taps outside the map: zero AFTER the prologue
    assert bool((col[pad] == 0.0).all()), f"{c.what} {rd}: a tap outside the map is not exactly 0 behind the prologue"


@pytest.mark.parametrize("case", V.PERM_CASES)
def test_conv_weight_perm_modes(case):
    K = _k()
    O, I, k = case
    c = V.weight_perm(case)
    w = dev(c.w)
    wg = K.conv_weight_to_gemm(w)
    same(wg, c.to_gemm, f"conv_weight_perm {case}: mode 1")
    same(K.conv_weight_to_dgrad_gemm(w), c.dgrad, f"conv_weight_perm {case}: mode 2")
    same(K.conv_wgrad_from_gemm(wg, (O, I, k, k), out=torch.full((O, I, k, k), 77.0, device="cuda")), c.w, f"conv_weight_perm {case}: mode 0")
    acc = dev(c.pre)
    assert K._L().dfd_conv_weight_perm(K._p(wg), K._p(acc), O, I, k, 0, 1, K._stream()) == 0
    same(acc, c.pre.double() + c.w.double(), f"conv_weight_perm {case}: mode 0, accumulate = 1")


# --------------------------------------------------------------------------------------------------------- past the grid cap
# See CAP_CASES (tests/_vit_cases.py) for the count each launcher forms.  Image 0 and the last image hold data of their own, every
# image between them a third pattern; the last image lies wholly in the second trip of the grid-stride loop.
def _at_cap(name, total):
    assert total == V.cap_total(name) and total > V.FIRST_PASS and V.grid_rule(total) == V.GRID_CAP, f"{name}: the grid is not at its cap"
    return V.CAP_CASES[name].N


def _ends(N, tail, seed, scale=1.0, vals=None):
    """(device f32 [N, *tail], f64 [2, *tail] = its first and last image)."""
    from tests._exact import S3, pick

    draw = (lambda s: scale * pick(tail, s, vals or S3)) if vals != "gauss" else (lambda s: V.randn(tail, s).double())
    first, last, mid = draw(seed), draw(seed + 1), draw(seed + 2)
    t = torch.empty((N,) + tuple(tail), device="cuda")
    t[:] = mid.float().cuda()
    t[0], t[-1] = first.float().cuda(), last.float().cuda()
    return t, torch.stack([first, last])


def _two(t):
    return torch.stack([t[0], t[-1]])


def test_cap_copy_rows():
    K = _k()
    N = _at_cap("copy_rows", 8193 * 256 * (8 // 4))                            # n * (C / 4)
    n = N * 256
    src, ends = _ends(N, (256, 8), 11000)
    dst = torch.full((n, 8), V.COPY_FILL, device="cuda")
    sidx = torch.arange(n - 1, -1, -1, dtype=torch.int32, device="cuda")        # dst[r] = src[n - 1 - r]
    K.copy_rows(src.view(n, 8), sidx, dst, None, n)
    same(_two(dst.view(N, 256, 8)), ends.flip(0).flip(1), "copy_rows past the grid cap: first and last 256 rows")


def test_cap_add_rowtable():
    K = _k()
    N = _at_cap("add_rowtable", 42801 * 49 * (8 // 4))                         # rows * (C / 4)
    x, ends = _ends(N, (49, 8), 11010)
    tab = V.add_rowtable((49, 3, 64)).tab[:, :8].contiguous()
    same(_two(K.add_rowtable(x, tab.cuda())), ends + tab.double(), "add_rowtable past the grid cap: first and last window")


def test_cap_subsample_add():
    K = _k()
    N = _at_cap("subsample_add", 524289 * 2 * 2 * (8 // 4))                    # N * h * w * (C / 4), h = (3 - 1) / 2 + 1
    x, xe = _ends(N, (3, 3, 8), 11020)
    a, ae = _ends(N, (2, 2, 8), 11023)
    bias = V.subsample((2, 7, 7, 2, 8)).bias
    same(_two(K.subsample_add(a, bias.cuda(), x, 2)), ae + bias.double() + xe[:, ::2, ::2], "subsample_add past the grid cap")


def test_cap_subsample_add_bwd():
    K = _k()
    N = _at_cap("subsample_bwd", 524289 * 2 * 2 * (8 // 4))                    # the same count: g's pixels
    dx, de = _ends(N, (3, 3, 8), 11030)
    g, ge = _ends(N, (2, 2, 8), 11033)
    de[:, ::2, ::2] += ge
    same(_two(K.subsample_add_bwd(g, dx, 2)), de, "subsample_add_bwd past the grid cap")


def test_cap_avgpool_fwd():
    K = _k()
    N = _at_cap("avgpool_fwd", 524289 * 2 * 2 * (8 // 4))                      # N * Ho * Wo * (C / 4), Ho = (3 - 2) / 1 + 1
    x, xe = _ends(N, (3, 3, 8), 11040, scale=4.0)
    want, _ = V.avgpool64(xe, torch.zeros(2, 2, 2, 8), 2, 1)
    same(_two(K.avgpool_fwd(x, 2, 1)), want, "avgpool_fwd past the grid cap")


def test_cap_avgpool_bwd():
    K = _k()
    N = _at_cap("avgpool_bwd", 83888 * 5 * 5 * (8 // 4))                       # N * H * W * (C / 4): the INPUT's pixels
    g, ge = _ends(N, (2, 2, 8), 11050, scale=4.0)
    _, want = V.avgpool64(torch.zeros(2, 5, 5, 8), ge, 2, 2)
    dx = K.avgpool_bwd(g, (N, 5, 5, 8), 2, 2)
    same(_two(dx), want, "avgpool_bwd past the grid cap")
    assert bool((_two(dx)[:, 4] == 0.0).all()) and bool((_two(dx)[:, :, 4] == 0.0).all())


def test_cap_up2_fwd():
    K = _k()
    N = _at_cap("up2_fwd", 131073 * 2 * 2 * (8 // 4) * 4)                      # N * h * w * (C / 4) * 4: the OUTPUT's vectors
    s, se = _ends(N, (2, 2, 8), 11060, scale=16.0)
    same(_two(K.up2_act_fwd(s, V.ACT_NONE)), V.up2_fwd64(se, V.ACT_NONE)[1], "up2_act_fwd past the grid cap")


def test_cap_up2_gradient_pass():
    K = _k()
    N = _at_cap("up2_grad", 131073 * 2 * 2 * (8 // 4) * 4)                     # pass 1 of the two-pass backward: tot * 4, as the forward
    s, se = _ends(N, (2, 2, 8), 11070, vals="gauss")
    g, ge = _ends(N, (4, 4, 8), 11073, vals="gauss")
    close(_two(K.up2_act_bwd(g, s, V.ACT_GELU)), V.up2_bwd64(ge, se, V.ACT_GELU), V.TOL[F32], "up2 gradient pass past the grid cap")


def test_cap_up2_bwd():
    K = _k()
    N = _at_cap("up2_bwd", 2097153 * 1 * 1 * (8 // 4))                         # N * h * w * (C / 4): the INPUT's pixels
    s, se = _ends(N, (1, 1, 8), 11080, scale=16.0)
    g, ge = _ends(N, (2, 2, 8), 11083, scale=16.0)
    same(_two(K.up2_act_bwd(g, s, V.ACT_NONE)), V.up2_bwd64(ge, se, V.ACT_NONE), "up2_act_bwd past the grid cap")


# ---------------------------------------------------------------------------------------------------------- argument rejection
def test_arguments_are_rejected_before_any_launch():
    """Every call below must return DFD_EINVAL (DFD_EWORKSPACE for the short workspace) from the entry point's own checks; every
    pointer is a 4 MiB buffer of a known pattern, which must still hold it afterwards."""
    from deepfakedetection_amd._lib import DwShape

    K = _k()
    L, st = K._L(), K._stream()
    bufs = [torch.full((1 << 20,), 3.0, device="cuda") for _ in range(5)]
    a, b, c, d, e = (t.data_ptr() for t in bufs)
    ibuf = torch.zeros(1 << 16, dtype=torch.int32, device="cuda")
    ix = ibuf.data_ptr()
    n = ctypes.c_int(-5)
    np_ = ctypes.byref(n)
    f32, bf16 = 0, 1
    shp = lambda **kw: ctypes.byref(DwShape(**{**dict(N=1, H=12, W=12, C=8, Ho=6, Wo=6, k=3, stride=2, pad_top=1, pad_left=1), **kw}))
    bad = {
        "up2 fwd C = 12": lambda: L.dfd_up2_act_fwd(f32, a, 0, b, 1, 2, 2, 12, st),
        "up2 fwd h = 0": lambda: L.dfd_up2_act_fwd(f32, a, 0, b, 1, 0, 2, 8, st),
        "up2 fwd no s": lambda: L.dfd_up2_act_fwd(f32, None, 0, b, 1, 2, 2, 8, st),
        "up2 fwd dtype": lambda: L.dfd_up2_act_fwd(2, a, 0, b, 1, 2, 2, 8, st),
        "up2 bwd C = 12": lambda: L.dfd_up2_act_bwd(bf16, a, b, 0, c, 1, 2, 2, 12, None, st),
        "up2 bwd w = 0": lambda: L.dfd_up2_act_bwd(f32, a, b, 3, c, 1, 2, 0, 8, d, st),
        "up2 bwd no ds": lambda: L.dfd_up2_act_bwd(f32, a, b, 0, None, 1, 2, 2, 8, None, st),
        "subsample stride 0": lambda: L.dfd_subsample_add(f32, a, b, c, d, 1, 4, 4, 0, 8, st),
        "subsample C = 12": lambda: L.dfd_subsample_add(f32, a, b, c, d, 1, 4, 4, 2, 12, st),
        "subsample no x": lambda: L.dfd_subsample_add(f32, a, b, None, d, 1, 4, 4, 2, 8, st),
        "subsample H = 0": lambda: L.dfd_subsample_add(bf16, a, b, c, d, 1, 0, 4, 2, 8, st),
        "subsample bwd stride 0": lambda: L.dfd_subsample_add_bwd(f32, a, b, 1, 4, 4, 0, 8, st),
        "subsample bwd no dx": lambda: L.dfd_subsample_add_bwd(f32, a, None, 1, 4, 4, 2, 8, st),
        "avgpool fwd H < k": lambda: L.dfd_avgpool_fwd(f32, a, b, 1, 4, 8, 5, 3, 8, st),
        "avgpool fwd W < k": lambda: L.dfd_avgpool_fwd(f32, a, b, 1, 8, 4, 5, 3, 8, st),
        "avgpool fwd stride 0": lambda: L.dfd_avgpool_fwd(f32, a, b, 1, 8, 8, 2, 0, 8, st),
        "avgpool fwd k = 0": lambda: L.dfd_avgpool_fwd(f32, a, b, 1, 8, 8, 0, 1, 8, st),
        "avgpool fwd C = 12": lambda: L.dfd_avgpool_fwd(bf16, a, b, 1, 8, 8, 2, 2, 12, st),
        "avgpool bwd H < k": lambda: L.dfd_avgpool_bwd(f32, a, b, 1, 4, 8, 5, 3, 8, st),
        "avgpool bwd stride 0": lambda: L.dfd_avgpool_bwd(f32, a, b, 1, 8, 8, 2, 0, 8, st),
        "avgpool bwd no g": lambda: L.dfd_avgpool_bwd(f32, None, b, 1, 8, 8, 2, 2, 8, st),
        "copy_rows C = 12": lambda: L.dfd_copy_rows(f32, a, None, b, None, 4, 12, st),
        "copy_rows n = 0": lambda: L.dfd_copy_rows(f32, a, None, b, None, 0, 8, st),
        "copy_rows no dst": lambda: L.dfd_copy_rows(bf16, a, ix, None, None, 4, 8, st),
        "add_rowtable C = 12": lambda: L.dfd_add_rowtable(f32, a, b, c, 49, 49, 12, st),
        "add_rowtable T = 0": lambda: L.dfd_add_rowtable(f32, a, b, c, 49, 0, 8, st),
        "add_rowtable no table": lambda: L.dfd_add_rowtable(f32, a, None, c, 49, 49, 8, st),
        "rowtable_grad rows % T": lambda: L.dfd_rowtable_grad(f32, a, b, 50, 49, 8, 0, c, 1 << 22, st),
        "rowtable_grad C = 6": lambda: L.dfd_rowtable_grad(f32, a, b, 49, 49, 6, 0, c, 1 << 22, st),
        "rowtable_grad C = 12 in bf16": lambda: L.dfd_rowtable_grad(bf16, a, b, 49, 49, 12, 0, c, 1 << 22, st),
        "rowtable_grad no workspace": lambda: L.dfd_rowtable_grad(f32, a, b, 49, 49, 8, 0, None, 1 << 22, st),
        "rowtable_grad no dtable": lambda: L.dfd_rowtable_grad(f32, a, None, 49, 49, 8, 0, c, 1 << 22, st),
        "bias_gather T = 0": lambda: L.dfd_bias_gather(a, ix, b, 2, 0, 9, st),
        "bias_gather no idx": lambda: L.dfd_bias_gather(a, None, b, 2, 3, 9, st),
        "bias_scatter L = 0": lambda: L.dfd_bias_scatter(a, ix, b, 2, 3, 0, 0, st),
        "bias_scatter H = 0": lambda: L.dfd_bias_scatter(a, ix, b, 0, 3, 9, 1, st),
        "bias_scatter no dtable": lambda: L.dfd_bias_scatter(a, ix, None, 2, 3, 9, 0, st),
        "relpos fwd n_local = 0": lambda: L.dfd_relpos_bias_fwd(a, ix, b, 2, 0, 4, st),
        "relpos fwd n_global = -1": lambda: L.dfd_relpos_bias_fwd(a, ix, b, 2, 4, -1, st),
        "relpos fwd no table": lambda: L.dfd_relpos_bias_fwd(None, ix, b, 2, 4, 0, st),
        "relpos bwd T = 0": lambda: L.dfd_relpos_bias_bwd(a, b, ix, c, 2, 0, 4, 0, st),
        "relpos bwd H = 0": lambda: L.dfd_relpos_bias_bwd(a, b, ix, c, 0, 1, 4, 0, st),
        "relpos bwd no dtable": lambda: L.dfd_relpos_bias_bwd(a, b, ix, None, 2, 1, 4, 0, st),
        "im2col k = 8": lambda: L.dfd_im2col(f32, a, None, 0, b, shp(k=8, Ho=3, Wo=3), st),
        "im2col stride 5": lambda: L.dfd_im2col(f32, a, None, 0, b, shp(stride=5, Ho=2, Wo=2), st),
        "im2col stride 0": lambda: L.dfd_im2col(f32, a, None, 0, b, shp(stride=0), st),
        "im2col Ho too large": lambda: L.dfd_im2col(f32, a, None, 0, b, shp(Ho=8), st),
        "im2col Wo too large": lambda: L.dfd_im2col(bf16, a, None, 0, b, shp(Wo=8), st),
        "im2col C = 12": lambda: L.dfd_im2col(f32, a, None, 0, b, shp(C=12), st),
        "im2col negative padding": lambda: L.dfd_im2col(f32, a, None, 0, b, shp(pad_left=-1), st),
        "im2col no shape": lambda: L.dfd_im2col(f32, a, None, 0, b, None, st),
        "im2col no col": lambda: L.dfd_im2col(f32, a, None, 0, None, shp(), st),
        "col2im k = 8": lambda: L.dfd_col2im(f32, a, b, shp(k=8, Ho=3, Wo=3), st),
        "col2im stride 5": lambda: L.dfd_col2im(f32, a, b, shp(stride=5, Ho=2, Wo=2), st),
        "col2im Ho too large": lambda: L.dfd_col2im(f32, a, b, shp(Ho=8), st),
        "col2im no dx": lambda: L.dfd_col2im(bf16, a, None, shp(), st),
        "conv_weight_perm O = 0": lambda: L.dfd_conv_weight_perm(a, b, 0, 3, 3, 1, 0, st),
        "conv_weight_perm k = 0": lambda: L.dfd_conv_weight_perm(a, b, 3, 3, 0, 0, 1, st),
        "conv_weight_perm no src": lambda: L.dfd_conv_weight_perm(None, b, 3, 3, 3, 2, 0, st),
        "channel_stats C = 12": lambda: L.dfd_channel_stats(f32, a, 16, 12, b, 1024, np_, st),
        "channel_stats rows = 0": lambda: L.dfd_channel_stats(f32, a, 0, 8, b, 1024, np_, st),
        "channel_stats no nparts": lambda: L.dfd_channel_stats(f32, a, 16, 8, b, 1024, None, st),
        "channel_stats pcap = 0": lambda: L.dfd_channel_stats(bf16, a, 16, 8, b, 0, np_, st),
        "channel_stats no partials": lambda: L.dfd_channel_stats(f32, a, 16, 8, None, 1024, np_, st),
        "bn_add_act_bwd partials without nparts": lambda: L.dfd_bn_add_act_bwd(f32, a, b, c, None, 0, d, 16, 8, e, 1024, None, st),
        "bn_add_act_bwd partials without state": lambda: L.dfd_bn_add_act_bwd(f32, a, b, None, None, 0, d, 16, 8, e, 1024, np_, st),
        "bn_add_act_bwd pcap = 0": lambda: L.dfd_bn_add_act_bwd(f32, a, b, c, None, 0, d, 16, 8, e, 0, np_, st),
        "bn_add_act_bwd C = 12": lambda: L.dfd_bn_add_act_bwd(bf16, a, b, c, None, 0, d, 16, 12, None, 0, None, st),
        "bn_add_act_bwd no d": lambda: L.dfd_bn_add_act_bwd(f32, a, b, c, None, 0, None, 16, 8, None, 0, None, st),
    }
    for what, call in bad.items():
        assert call() == EINVAL, what
    need = int(L.dfd_rowtable_grad_ws(49, 8))
    assert need <= 1 << 22
    assert L.dfd_rowtable_grad(f32, a, b, 49, 49, 8, 0, c, need - 1, st) == EWORKSPACE, "rowtable_grad: a workspace one byte short"
    torch.cuda.synchronize()
    assert n.value == -5
    for t in bufs:
        assert bool((t == 3.0).all()), "a rejected call wrote to one of its buffers"
    assert bool((ibuf == 0).all())
