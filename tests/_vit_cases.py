"""TEST INFRASTRUCTURE - case tables and float64 references for the small spatial and token-bookkeeping kernels of csrc/dfd_vit.hip
(pure CPU; nothing here touches the GPU).

up2_act, subsample_add, avgpool, copy_rows, add_rowtable / rowtable_grad, bias_gather / bias_scatter, relpos_bias, im2col / col2im,
conv_weight_perm, and the ChanMap shapes of channel_stats / bn_add_act_bwd.  One case per branch of each kernel and per boundary
between two branches, with the launch shape each case is MEANT to reach written next to it.  The rules the launchers follow are
restated below (chanmap, rowtable_rule, nparts_rule, grid_rule); tests/test_vit_edges_cpu.py holds the tables against these rules and
against the library's own host-side query (dfd_rowtable_grad_plan), tests/test_vit_edges_gpu.py runs the kernels.

Wherever the arithmetic allows, the data are small integers (tests/_exact.py: pick, check_exact) and the comparison is at tolerance 0.
Values that pass through sixteenths (the bilinear weights) or through 1 / k**2 (the pooling mean) are drawn from 16 * {-3..3} or
k**2 * {-3..3}, so that every stored result is an integer: the same lattice as operands in {-3..3} with results in sixteenths, in the
units check_exact asks of a bf16 result.
"""

from __future__ import annotations

import functools
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

from oracle import ops_ref as R
from tests._exact import BF16, DTYPES, F32, S2, S3, ConditionViolated, bn_state, check_exact, f32, pick

ACT_NONE, ACT_SILU, ACT_GELU = R.ACT_NONE, R.ACT_SILU, R.ACT_GELU
ACTS3 = (ACT_NONE, ACT_GELU, ACT_SILU)
THREADS = 256
GRID_CAP = 16384                                       # workgroups of the grid-stride kernels below (k_col2im and k_im2col: 32768)
FIRST_PASS = GRID_CAP * THREADS                        # 4,194,304 vectors: what one pass of a capped grid covers
MAX_PARTIALS = 1024
ROWTAB_MAX_SPLITS = 32
VEC = {F32: 4, BF16: 8}                                # elements per 16-byte lane
TOL = {F32: 2e-4, BF16: 1.6e-2}                        # tests/test_vit_ops_gpu.py: of the reference's largest magnitude
TOL_SUMS = {F32: 5e-4, BF16: 5e-3}                     # the same file, per-channel sums
GUARD = 64                                             # elements in front of and behind a guarded tensor (test_vit_edges_gpu.py)
BUDGET_BYTES = 300 * 2 ** 20                           # device memory of one case (one exception, stated at CAP_CASES)


def randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


# ------------------------------------------------------------------------------------------------- the launchers' rules, restated
def chanmap(C: int, vec: int):
    """make_chanmap (csrc/dfd_common.h): (cvb, rpb, nvc)."""
    cv = C // vec
    cvb = cv
    if cv > 64:
        cvb = max(d for d in range(1, 65) if cv % d == 0)
    return cvb, THREADS // cvb, cv // cvb


def rowtable_rule(nw: int, T: int, C: int, vec: int):
    """rowtable_splits and the launcher of dfd_rowtable_grad: (splits, w_per, rpb, limiter)."""
    _, rpb, nvc = chanmap(C, vec)
    by_grid, by_windows = 2048 // (T * nvc), nw // (4 * rpb)
    s = max(1, min(by_grid, by_windows, ROWTAB_MAX_SPLITS))
    limiter = "one" if s == 1 else "windows" if by_windows <= min(by_grid, ROWTAB_MAX_SPLITS) else \
        "cap" if ROWTAB_MAX_SPLITS <= by_grid else "grid"
    return s, -(-nw // s), rpb, limiter


def rowtable_lanes(nw: int, splits: int, w_per: int, rpb: int):
    """Per split: (windows in it, row lanes that take at least one unrolled step of four, row lanes that take none but a tail step)."""
    out = []
    for z in range(splits):
        beg, end = z * w_per, min((z + 1) * w_per, nw)
        unrolled = sum(1 for rl in range(rpb) if beg + rl + 3 * rpb < end)
        tail_only = sum(1 for rl in range(rpb) if beg + rl < end and not beg + rl + 3 * rpb < end)
        out.append((end - beg, unrolled, tail_only))
    return out


def nparts_rule(rows: int, rpb: int, pcap: int = MAX_PARTIALS) -> int:
    """vit_pick_parts: ceil(rows / (4 rpb)) within 1 .. min(pcap, 1024)."""
    return max(1, min(-(-rows // (4 * rpb)), min(pcap, MAX_PARTIALS)))


def grid_rule(total_vectors: int, cap: int = GRID_CAP) -> int:
    """min(ceil(total / 256), cap): the launch of every grid-stride kernel here."""
    return min(-(-total_vectors // THREADS), cap)


# ----------------------------------------------------------------------------------------------------------------- rowtable_grad
# (nw windows, T, C, dtype) -> (splits, w_per, rpb) and what the case is there for.  limiter: which of the three bounds of
# rowtable_splits decides (windows = nw / (4 rpb), cap = 32, grid = 2048 / (T nvc)); one = a single split.
ROWTABLE_CASES = [
    NS(nw=6, T=49, C=64, rd=F32, plan=(1, 6, 16), limiter="one", note="the shape of tests/test_vit_ops_gpu.py: tail loop only"),
    NS(nw=6, T=49, C=64, rd=BF16, plan=(1, 6, 32), limiter="one", note="the same in bf16"),
    NS(nw=127, T=3, C=64, rd=BF16, plan=(1, 127, 32), limiter="one", note="row lanes below 31 take one unrolled step, lane 31 only the tail"),
    NS(nw=256, T=3, C=64, rd=BF16, plan=(2, 128, 32), limiter="windows", note="two full splits: blockIdx.z = 1"),
    NS(nw=259, T=3, C=64, rd=BF16, plan=(2, 130, 32), limiter="windows", note="the last split clipped to 129 windows"),
    NS(nw=4101, T=16, C=64, rd=BF16, plan=(32, 129, 32), limiter="windows", note="32 splits (nw / 128 = 32 meets the cap), last one 102 windows"),
    NS(nw=4229, T=16, C=64, rd=BF16, plan=(32, 133, 32), limiter="cap", note="nw / 128 = 33: the cap of 32 decides"),
    # C = 264 in f32: 66 vectors, largest divisor <= 64 is 33 -> cvb 33, rpb 7 (231 of 256 threads), nvc 2 (blockIdx.y = 1).
    # 60 windows: 60 / 28 = 2 splits (2048 / (50 * 2) = 20 would allow more).  588 windows: 588 / 28 = 21 > 20, the grid bound decides.
    NS(nw=60, T=50, C=264, rd=F32, plan=(2, 30, 7), limiter="windows", note="nvc 2, rpb 7: idle threads in reduce_rowlanes"),
    NS(nw=588, T=50, C=264, rd=F32, plan=(20, 30, 7), limiter="grid", note="2048 / (T nvc) = 20 decides; last split 18 windows"),
    NS(nw=3, T=5, C=4, rd=F32, plan=(1, 3, 256), limiter="one", note="C below 8: one vector"),
    NS(nw=1, T=1, C=8, rd=F32, plan=(1, 1, 128), limiter="one", note="a single row"),
    NS(nw=1, T=1, C=8, rd=BF16, plan=(1, 1, 256), limiter="one", note="a single row, one vector"),
]


@functools.lru_cache(maxsize=4)
def rowtable(i: int):
    c = ROWTABLE_CASES[i]
    what = f"rowtable_grad ({c.nw}, {c.T}, {c.C}) {c.rd}"
    g = pick((c.nw, c.T, c.C), 9100 + i, S3)
    pre = pick((c.T, c.C), 9150 + i, S3)
    check_exact(what, operands=[("g", g, (c.rd,)), ("pre-fill", pre, (F32,))], reductions=[("windows", g.abs().sum(0) + pre.abs(), 1.0)],
                results=[("dtable", g.sum(0), (F32,)), ("accumulated", g.sum(0) + pre, (F32,))])
    return NS(what=what, case=c, g=f32(g), pre=f32(pre), dtable=g.sum(0))


# ------------------------------------------------------------------------------------ channel_stats and bn_add_act_bwd: ChanMap shapes
# C -> ChanMap (cvb, rpb, nvc) in f32 (C / 4 vectors) and in bf16 (C / 8 vectors)
REDUCE_WIDTHS = {
    8: {F32: (2, 128, 1), BF16: (1, 256, 1)},          # bf16: one vector
    1024: {F32: (64, 4, 4), BF16: (64, 4, 2)},         # more than 64 vectors: blockIdx.y > 0
    536: {F32: (2, 128, 67), BF16: (1, 256, 67)},      # 134 = 2 * 67 and 67 vectors: the largest divisor <= 64 is 2 and 1
    224: {F32: (56, 4, 1), BF16: (28, 9, 1)},          # 56 * 4 = 224 and 28 * 9 = 252 threads: 32 and 4 idle lanes
}
REDUCE_ROWS_BIG = 600


def reduce_rows(rpb: int):
    return sorted({1, rpb - 1, 4 * rpb + 1, REDUCE_ROWS_BIG})


REDUCE_CASES = [(C, rd, rows) for C in REDUCE_WIDTHS for rd in DTYPES for rows in reduce_rows(REDUCE_WIDTHS[C][rd][1])]


@functools.lru_cache(maxsize=4)
def reduce_exact(C: int, rows: int):
    """y, g, other: integers; BN state with power-of-two scale and rstd.  ACT_NONE: d = g, sums of d and d * xhat in halves."""
    what = f"reducing kernels C {C} rows {rows}"
    y, g, other = pick((rows, 1, 1, C), 9200 + C, S3), pick((rows, 1, 1, C), 9201 + C, S3), pick((rows, 1, 1, C), 9202 + C, S2)
    st = bn_state(C, 9203 + C)
    xhat = (y - st[2]) * st[3]
    flat = lambda t: t.reshape(rows, C)
    stats = torch.stack([flat(y).sum(0), flat(y * y).sum(0)])
    sums = torch.stack([flat(g).sum(0), flat(g * xhat).sum(0)])
    check_exact(what, operands=[("y", y, DTYPES), ("g", g, DTYPES), ("other", other, DTYPES), ("xhat", xhat, (F32,))],
                stats=[("sum y*y", flat(y * y).sum(0), 1.0), ("sum |g xhat|", flat((g * xhat).abs()).sum(0), 0.5)],
                results=[("d", g, DTYPES), ("stats", stats, (F32,)), ("sums", sums, (F32,))])
    return NS(what=what, y=f32(y), g=f32(g), other=f32(other), st=f32(st), d=g, stats=stats, sums=sums)


@functools.lru_cache(maxsize=4)
def reduce_act(C: int, rd, act: int):
    """Gaussian data on the 600-row case: float64 d = g act'(scale y + shift + other) from the values as stored in `rd`."""
    rows = REDUCE_ROWS_BIG
    y, g, other = (randn((rows, 1, 1, C), 9300 + C + j).to(rd) for j in range(3))
    gen = torch.Generator().manual_seed(9304 + C)
    st = torch.stack([0.5 + torch.rand(C, generator=gen), torch.randn(C, generator=gen) * 0.3, torch.randn(C, generator=gen) * 0.2,
                      0.5 + torch.rand(C, generator=gen)])
    z = st[0].double() * y.double() + st[1].double() + other.double()
    d = g.double() * R.act_grad(z, act)
    dr = d.to(rd).double()                                        # the kernel sums what it stores
    xhat = (y.double() - st[2].double()) * st[3].double()
    sums = torch.stack([dr.reshape(rows, C).sum(0), (dr * xhat).reshape(rows, C).sum(0)])
    return NS(y=y, g=g, other=other, st=st, d=d, sums=sums)


# ------------------------------------------------------------------------------------------------------------------------- up2
UP2_SHAPES = [(1, 1, 1, 8), (2, 1, 5, 8), (2, 5, 1, 16), (1, 2, 2, 8), (3, 2, 7, 24), (2, 7, 7, 40)]       # N, h, w, C


def up2_taps(Y: int, h: int):
    """The tap table of bilinear x2, align_corners = False: output row Y reads rows (i0, i1) with weights (w0, w1)."""
    m = Y >> 1
    if Y & 1:
        return m, min(m + 1, h - 1), 0.75, 0.25
    return max(m - 1, 0), m, 0.25, 0.75


def up2_matrix(h: int) -> torch.Tensor:
    """[2h, h] f64: row Y holds the weights of output row Y; two taps that clamp to the same input row add up."""
    U = torch.zeros(2 * h, h, dtype=torch.float64)
    for Y in range(2 * h):
        i0, i1, w0, w1 = up2_taps(Y, h)
        U[Y, i0] += w0
        U[Y, i1] += w1
    return U


def up2_fwd64(s: torch.Tensor, act: int):
    """(up, act(up)) of s [N, h, w, C] in float64."""
    up = torch.einsum("Yy,Xx,nyxc->nYXc", up2_matrix(s.shape[1]), up2_matrix(s.shape[2]), s.double())
    return up, R.act_fwd(up, act)


def up2_bwd64(g: torch.Tensor, s: torch.Tensor, act: int):
    up, _ = up2_fwd64(s, act)
    return torch.einsum("Yy,Xx,nYXc->nyxc", up2_matrix(s.shape[1]), up2_matrix(s.shape[2]), g.double() * R.act_grad(up, act))


@functools.lru_cache(maxsize=4)
def up2_exact(shape):
    N, h, w, C = shape
    what = f"up2 {shape}"
    s, g = 16.0 * pick(shape, 9400 + h * 8 + w, S3), 16.0 * pick((N, 2 * h, 2 * w, C), 9401 + h * 8 + w, S3)
    out, ds = up2_fwd64(s, ACT_NONE)[1], up2_bwd64(g, s, ACT_NONE)
    check_exact(what, operands=[("s", s, DTYPES), ("g", g, DTYPES)],
                reductions=[("taps", up2_fwd64(s.abs(), ACT_NONE)[0], 1.0), ("transposed taps", up2_bwd64(g.abs(), s, ACT_NONE), 1.0)],
                results=[("out", out, DTYPES), ("ds", ds, DTYPES)])
    return NS(what=what, s=f32(s), g=f32(g), out=out, ds=ds)


@functools.lru_cache(maxsize=4)
def up2_gauss(shape, rd, act: int):
    N, h, w, C = shape
    s, g = randn(shape, 9450 + h * 8 + w).to(rd), randn((N, 2 * h, 2 * w, C), 9451 + h * 8 + w).to(rd)
    return NS(s=s, g=g, out=up2_fwd64(s, act)[1], ds=up2_bwd64(g, s, act))


# ------------------------------------------------------------------------------------------------------------------- subsample
SUBSAMPLE_CASES = [(2, 14, 14, 2, 24), (2, 7, 7, 2, 8), (1, 9, 5, 3, 16), (2, 8, 8, 4, 8), (1, 5, 5, 1, 8), (1, 1, 1, 2, 8)]   # N, H, W, stride, C


@functools.lru_cache(maxsize=4)
def subsample(case):
    N, H, W, s, C = case
    h, w = (H - 1) // s + 1, (W - 1) // s + 1
    what = f"subsample {case}"
    seed = 9500 + 37 * H + 5 * W + s
    a, x, bias, dx0 = pick((N, h, w, C), seed, S3), pick((N, H, W, C), seed + 1, S3), pick((C,), seed + 2, S3), pick((N, H, W, C), seed + 3, S3)
    lattice = torch.zeros(H, W, dtype=torch.bool)
    lattice[::s, ::s] = True
    if int(lattice.sum()) != h * w or not bool(lattice[(h - 1) * s, (w - 1) * s]):
        raise ConditionViolated(f"{what}: the stride lattice does not have {h} x {w} points")
    out_b, out_0 = a + bias + x[:, ::s, ::s], a + x[:, ::s, ::s]
    dx1 = dx0.clone()
    dx1[:, ::s, ::s] += a
    check_exact(what, operands=[("a", a, DTYPES), ("x", x, DTYPES), ("bias", bias, (F32,)), ("dx", dx0, DTYPES)],
                results=[("out", out_b, DTYPES), ("out without bias", out_0, DTYPES), ("dx", dx1, DTYPES)])
    return NS(what=what, h=h, w=w, a=f32(a), x=f32(x), bias=f32(bias), dx0=f32(dx0), out_b=out_b, out_0=out_0, dx1=dx1, lattice=lattice)


# --------------------------------------------------------------------------------------------------------------------- avgpool
AVGPOOL_CASES = [                                        # N, H, W, k, s, C
    (2, 14, 14, 5, 3, 32),                               # the case of tests/test_vit_ops_gpu.py: the windows tile the map
    (1, 15, 16, 5, 3, 8),                                # Ho 4, Wo 4: row 14 and columns 14, 15 are read by no window
    (2, 5, 5, 5, 3, 8),                                  # one window
    (1, 8, 8, 2, 2, 16),                                 # exact, tiled
    (1, 9, 9, 4, 2, 8),                                  # exact, windows overlap by 2, row and column 8 uncovered
    (1, 6, 6, 1, 1, 8),                                  # identity
    (1, 7, 7, 3, 1, 8),                                  # every interior pixel sits in 9 windows
]
AVGPOOL_EXACT_K = (1, 2, 4)


def avgpool_covered(H: int, W: int, k: int, s: int) -> torch.Tensor:
    """[H, W] bool: pixels that some window reads (index arithmetic: the windows start at multiples of s and are k wide)."""
    Ho, Wo = (H - k) // s + 1, (W - k) // s + 1
    rows, cols = torch.arange(H) < (Ho - 1) * s + k, torch.arange(W) < (Wo - 1) * s + k
    if k < s:                                            # gaps between the windows as well (no case here; kept for the rule's sake)
        rows, cols = rows & (torch.arange(H) % s < k), cols & (torch.arange(W) % s < k)
    return rows[:, None] & cols[None, :]


def avgpool64(x: torch.Tensor, g: torch.Tensor, k: int, s: int):
    xn = x.double().permute(0, 3, 1, 2).clone().requires_grad_()
    out = F.avg_pool2d(xn, k, s)
    out.backward(g.double().permute(0, 3, 1, 2))
    return out.detach().permute(0, 2, 3, 1).contiguous(), xn.grad.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=4)
def avgpool(case, rd=F32):
    """k in {1, 2, 4}: x and g hold k**2 times small integers, every mean is an integer (rd is ignored); else Gaussian data stored in rd."""
    N, H, W, k, s, C = case
    Ho, Wo = (H - k) // s + 1, (W - k) // s + 1
    what = f"avgpool {case}"
    exact = k in AVGPOOL_EXACT_K
    seed = 9600 + 41 * H + 7 * k + s
    if exact:
        x, g = float(k * k) * pick((N, H, W, C), seed, S3), float(k * k) * pick((N, Ho, Wo, C), seed + 1, S3)
    else:
        x, g = randn((N, H, W, C), seed).to(rd), randn((N, Ho, Wo, C), seed + 1).to(rd)
    out, dx = avgpool64(x, g, k, s)
    if exact:
        check_exact(what, operands=[("x", x, DTYPES), ("g", g, DTYPES)],
                    reductions=[("window", avgpool64(x.abs(), g, k, s)[0] * k * k, 1.0), ("windows over a pixel", avgpool64(x, g.abs(), k, s)[1] * k * k, 1.0)],
                    results=[("out", out, DTYPES), ("dx", dx, DTYPES)])
        x, g = f32(x), f32(g)
    return NS(what=what, exact=exact, Ho=Ho, Wo=Wo, x=x, g=g, out=out, dx=dx, covered=avgpool_covered(H, W, k, s))


# -------------------------------------------------------------------------------------------------- copy_rows and add_rowtable
COPY_C = (8, 24, 1024)
COPY_N = (1, 255, 257)                                   # one row; one short of and one past a workgroup of one-vector rows
COPY_MODES = ("perm", "sidx", "didx", "both", "fewer")
COPY_FILL = -7.0                                         # the destination's pre-fill (no source value)


@functools.lru_cache(maxsize=4)
def copy_rows(C: int, n: int, mode: str):
    """(src [rs, C], sidx | None, didx | None, rows of dst, want [rd, C] f64 with COPY_FILL where no row is written)."""
    gen = torch.Generator().manual_seed(9700 + C + 3 * n + COPY_MODES.index(mode))
    rs = n if mode in ("perm", "didx") else n + 5
    rdst = n if mode in ("perm", "sidx") else n + 7
    src = pick((rs, C), 9701 + C + n, S3)
    sidx = torch.randperm(rs, generator=gen)[:n].to(torch.int32) if mode in ("sidx", "both") else None
    didx = torch.randperm(rdst, generator=gen)[:n].to(torch.int32) if mode in ("perm", "didx", "both") else None
    want = torch.full((rdst, C), COPY_FILL, dtype=torch.float64)
    rows = torch.arange(n)
    want[rows if didx is None else didx.long()] = src[rows if sidx is None else sidx.long()]
    check_exact(f"copy_rows {C} {n} {mode}", operands=[("src", src, DTYPES), ("fill", want, DTYPES)])
    return NS(src=f32(src), sidx=sidx, didx=didx, rdst=rdst, want=want, untouched=rdst - n)


ADD_ROWTABLE_CASES = [(1, 7, 8), (16, 5, 40), (49, 3, 64), (49, 6, 24)]         # T, windows, C: the row count is windows * T


@functools.lru_cache(maxsize=4)
def add_rowtable(case):
    T, nw, C = case
    x, tab = pick((nw, T, C), 9800 + T + C, S3), pick((T, C), 9801 + T + C, S3)
    out = x + tab
    check_exact(f"add_rowtable {case}", operands=[("x", x, DTYPES), ("table", tab, (F32,))], results=[("out", out, DTYPES)])
    return NS(x=f32(x), tab=f32(tab), out=out)


# ------------------------------------------------------------------------------------------------ bias gather / scatter, relpos
BIAS_CASES = [(1, 1, 1), (3, 5, 255), (8, 49, 2401), (2, 7, 513)]               # H, T, L


def sparse_index(n: int, T: int, seed: int):
    """(int32 [n] index into T rows, bool [T] rows that occur).  Where T > 1 every third row, at least one, never occurs; every other
    row occurs as far as n allows."""
    gen = torch.Generator().manual_seed(seed)
    allowed = torch.tensor([t for t in range(T) if T == 1 or t % 3 != 1])
    idx = allowed[torch.randint(0, len(allowed), (n,), generator=gen)]
    m = min(n, len(allowed))
    idx[torch.randperm(n, generator=gen)[:m]] = allowed[torch.randperm(len(allowed), generator=gen)[:m]]
    used = torch.zeros(T, dtype=torch.bool)
    used[idx] = True
    if T > 1 and bool(used.all()):
        raise ConditionViolated(f"index table ({n}, {T}): every row occurs")
    return idx.to(torch.int32), used


@functools.lru_cache(maxsize=4)
def bias(case):
    H, T, L = case
    what = f"bias gather / scatter {case}"
    idx, used = sparse_index(L, T, 9900 + L)
    table, dfull, pre = pick((H, T), 9901 + L, S3), pick((H, L), 9902 + L, S3), pick((H, T), 9903 + L, S3)
    dtable = torch.zeros(H, T, dtype=torch.float64).index_add_(1, idx.long(), dfull)
    mass = torch.zeros(H, T, dtype=torch.float64).index_add_(1, idx.long(), dfull.abs()) + pre.abs()
    check_exact(what, operands=[("table", table, (F32,)), ("dfull", dfull, (F32,)), ("pre-fill", pre, (F32,))],
                reductions=[("scatter", mass, 1.0)], results=[("dtable", dtable, (F32,)), ("accumulated", dtable + pre, (F32,))])
    if not bool((dtable[:, ~used] == 0).all()):
        raise ConditionViolated(f"{what}: the reference is not zero on an unused row")
    return NS(what=what, idx=idx, used=used, table=f32(table), full=table[:, idx.long()], dfull=f32(dfull), pre=f32(pre), dtable=dtable)


RELPOS_CASES = [(8, 49, 4, 169), (3, 16, 0, 49), (5, 9, 2, 25), (1, 1, 0, 1)]   # H, nl, ng, T.  T * H = 1352, 147, 125, 1 waves: only the
                                                                                # first is a multiple of 4 (the early-return guard)


@functools.lru_cache(maxsize=4)
def relpos(case):
    """Forward on a Gaussian table (float64 reference); backward at table = 0, where d(16 sigmoid) = 4 exactly."""
    H, nl, ng, T = case
    what = f"relpos bias {case}"
    S = nl + ng
    idx, used = sparse_index(nl * nl, T, 10000 + nl)
    table = randn((T, H), 10001 + nl)
    full = torch.zeros(H, S, S, dtype=torch.float64)
    full[:, ng:, ng:] = 16.0 * torch.sigmoid(table.double()[idx.long()]).view(nl, nl, H).permute(2, 0, 1)
    dfull = pick((H, S, S), 10002 + nl, S3)
    local = dfull[:, ng:, ng:].reshape(H, nl * nl)
    dtable = 4.0 * torch.zeros(H, T, dtype=torch.float64).index_add_(1, idx.long(), local).t()
    mass = 4.0 * torch.zeros(H, T, dtype=torch.float64).index_add_(1, idx.long(), local.abs()).t()
    check_exact(what, operands=[("dfull", dfull, (F32,))], reductions=[("relpos", mass, 1.0)], results=[("dtable", dtable, (F32,))])
    return NS(what=what, idx=idx, used=used, table=table, full=full, dfull=f32(dfull), dtable=dtable.contiguous())


# ------------------------------------------------------------------------------------------------------------- im2col / col2im
# k, s, pad_top, pad_left, C, H (= W), N, (Ho, Wo).  Full output size with bottom = top and right = left padding unless noted.
IM2COL_CASES = [
    (3, 2, 1, 1, 16, 12, 2, (6, 6)), (3, 1, 1, 1, 24, 9, 2, (9, 9)), (3, 2, 1, 1, 48, 7, 2, (4, 4)),       # tests/test_vit_ops_gpu.py
    (5, 1, 2, 2, 8, 9, 2, (9, 9)),
    (7, 2, 3, 3, 8, 16, 1, (8, 8)),
    (3, 3, 0, 0, 16, 10, 2, (3, 3)),                       # row and column 9 are read by no tap
    (3, 4, 1, 1, 8, 13, 1, (4, 4)),
    (3, 2, 0, 1, 8, 12, 2, (5, 6)),                        # pad_top != pad_left: Ho = (12 - 3) / 2 + 1, Wo = (12 + 2 - 3) / 2 + 1
    (3, 2, 1, 1, 8, 12, 1, (5, 5)),                        # one less than the full 6 x 6: the last output row and column are not formed
]


def conv_shape_ok(k, s, pt, pl, C, H, W, N, Ho, Wo) -> bool:
    """conv_shape_ok (csrc/dfd_vit.hip)."""
    if min(N, H, W, Ho, Wo) < 1 or C < 8 or C % 8 or not 1 <= k <= 7 or not 1 <= s <= 4 or pt < 0 or pl < 0:
        return False
    return (Ho - 1) * s - pt <= H - 1 and (Wo - 1) * s - pl <= W - 1


def im2col64(a: torch.Tensor, k, s, pt, pl, Ho, Wo):
    """[N, Ho, Wo, k*k*C] with column (kh*k + kw)*C + c; zeros outside the map (F.unfold on the padded map, cut to Ho x Wo)."""
    N, H, W, C = a.shape
    Hp, Wp = max(pt + H, (Ho - 1) * s + k), max(pl + W, (Wo - 1) * s + k)
    ap = F.pad(a.double().permute(0, 3, 1, 2), (pl, Wp - pl - W, pt, Hp - pt - H))
    Hf, Wf = (Hp - k) // s + 1, (Wp - k) // s + 1
    unf = F.unfold(ap, k, stride=s).view(N, C, k * k, Hf, Wf)[:, :, :, :Ho, :Wo]
    return unf.permute(0, 3, 4, 2, 1).reshape(N, Ho, Wo, k * k * C)


def col2im64(dcol: torch.Tensor, shape, k, s, pt, pl):
    """Tap by tap: dx[oy*s - pt + kh, ox*s - pl + kw] += dcol[oy, ox, kh*k + kw] on a padded buffer, then the map cut out."""
    N, H, W, C = shape
    Ho, Wo = dcol.shape[1], dcol.shape[2]
    d = dcol.double().view(N, Ho, Wo, k * k, C)
    buf = torch.zeros(N, max(pt + H, (Ho - 1) * s + k), max(pl + W, (Wo - 1) * s + k), C, dtype=torch.float64)
    for kh in range(k):
        for kw in range(k):
            buf[:, kh:kh + (Ho - 1) * s + 1:s, kw:kw + (Wo - 1) * s + 1:s] += d[:, :, :, kh * k + kw]
    return buf[:, pt:pt + H, pl:pl + W].contiguous()


@functools.lru_cache(maxsize=4)
def im2col(i: int):
    k, s, pt, pl, C, H, N, (Ho, Wo) = IM2COL_CASES[i]
    what = f"im2col {IM2COL_CASES[i]}"
    if not conv_shape_ok(k, s, pt, pl, C, H, H, N, Ho, Wo):
        raise ConditionViolated(f"{what}: conv_shape_ok rejects the shape")
    x, dcol = pick((N, H, H, C), 10100 + i, S3), pick((N, Ho, Wo, k * k * C), 10150 + i, S3)
    col, dx = im2col64(x, k, s, pt, pl, Ho, Wo), col2im64(dcol, (N, H, H, C), k, s, pt, pl)
    check_exact(what, operands=[("x", x, DTYPES), ("dcol", dcol, DTYPES)],
                reductions=[("col2im", col2im64(dcol.abs(), (N, H, H, C), k, s, pt, pl), 1.0)], results=[("col", col, DTYPES), ("dx", dx, DTYPES)])
    return NS(what=what, k=k, s=s, pt=pt, pl=pl, C=C, H=H, N=N, Ho=Ho, Wo=Wo, x=f32(x), dcol=f32(dcol), col=col, dx=dx)


@functools.lru_cache(maxsize=4)
def im2col_prologue(i: int, rd):
    """Gaussian x stored in rd behind BN + GELU: the padding is zero AFTER the prologue."""
    k, s, pt, pl, C, H, N, (Ho, Wo) = IM2COL_CASES[i]
    x = randn((N, H, H, C), 10200 + i).to(rd)
    gen = torch.Generator().manual_seed(10250 + i)
    st = torch.stack([0.5 + torch.rand(C, generator=gen), torch.randn(C, generator=gen) * 0.3, torch.randn(C, generator=gen) * 0.2,
                      0.5 + torch.rand(C, generator=gen)])
    a = F.gelu(st[0].double() * x.double() + st[1].double())
    return NS(x=x, st=st, col=im2col64(a, k, s, pt, pl, Ho, Wo))


PERM_CASES = [(1, 1, 1), (5, 3, 3), (7, 2, 5), (3, 4, 7)]                         # O, I, k


@functools.lru_cache(maxsize=4)
def weight_perm(case):
    """Index arithmetic of the three modes: 1: [O][(kh, kw, i)]; 0: its inverse (+ accumulate); 2: [I][(flipped kh, kw, o)]."""
    O, I, k = case
    w = pick((O, I, k, k), 10300 + O + I + k, S3)
    pre = pick((O, I, k, k), 10301 + O + I + k, S3)
    to_gemm = w.permute(0, 2, 3, 1).reshape(O, k * k * I)
    dgrad = w.flip(2, 3).permute(1, 2, 3, 0).reshape(I, k * k * O)
    check_exact(f"conv_weight_perm {case}", operands=[("w", w, (F32,)), ("pre-fill", pre, (F32,))], results=[("accumulated", w + pre, (F32,))])
    return NS(w=f32(w), pre=f32(pre), to_gemm=to_gemm.contiguous(), dgrad=dgrad.contiguous())


# --------------------------------------------------------------------------------------------------------- past the grid cap
# One case per grid-stride kernel, f32 and C = 8 (two vectors per pixel or row): the launcher forms grid = min(ceil(total / 256), 16384)
# from `total` vectors, so a kernel's second loop trip starts at vector 16384 * 256 = 4,194,304.  N is the smallest count of images
# (windows, row blocks) whose LAST one lies wholly behind that vector: (N - 1) * per_image >= 4,194,304, per_image = vectors of one
# image in the launcher's count.  k_col2im and k_im2col loop the same way but under a cap of 32768 workgroups (twice the size):
# left out.
#   name            launcher's total                   per image                 N
#   copy_rows       n * C/4                            256 rows * 2 = 512        8193 blocks of 256 rows
#   add_rowtable    rows * C/4                         49 rows * 2 = 98          42801 windows (42800 * 98 = 4,194,400)
#   subsample_add   N * h * w * C/4 (OUTPUT pixels)    H = W = 3, s = 2: 2*2*2 = 8    524289
#   subsample_bwd   the same count (g's pixels)        8                         524289
#   avgpool_fwd     N * Ho * Wo * C/4 (OUTPUT)         H = W = 3, k 2, s 1: 2*2*2 = 8 524289
#   avgpool_bwd     N * H * W * C/4 (INPUT pixels)     H = W = 5, k 2, s 2: 25*2 = 50 83888 (83887 * 50 = 4,194,350)
#   up2_fwd         N * h * w * C/4 * 4 (OUTPUT)       h = w = 2: 16*2 = 32      131073
#   up2_grad        the same count as up2_fwd (pass 1 of the two-pass backward: one item per OUTPUT vector)    131073
#   up2_bwd         N * h * w * C/4 (INPUT pixels)     h = w = 1: 2              2097153
# up2_bwd needs s, ds (N * 32 bytes each) and g (four times that): 6 * 64 MiB, the only case above BUDGET_BYTES, and the smallest
# there is for this kernel in f32 (C = 8 is the narrowest row the entry point takes).
CAP_CASES = {
    "copy_rows": NS(per_image=512, N=8193, bytes=2 * 8193 * 256 * 32),
    "add_rowtable": NS(per_image=98, N=42801, bytes=2 * 42801 * 49 * 32),
    "subsample_add": NS(per_image=8, N=524289, bytes=524289 * (9 + 4 + 4) * 32),
    "subsample_bwd": NS(per_image=8, N=524289, bytes=524289 * (9 + 4) * 32),
    "avgpool_fwd": NS(per_image=8, N=524289, bytes=524289 * (9 + 4) * 32),
    "avgpool_bwd": NS(per_image=50, N=83888, bytes=83888 * (25 + 4) * 32),
    "up2_fwd": NS(per_image=32, N=131073, bytes=131073 * (4 + 16) * 32),
    "up2_grad": NS(per_image=32, N=131073, bytes=131073 * (4 + 4 + 16 + 16) * 32),
    "up2_bwd": NS(per_image=2, N=2097153, bytes=2097153 * (1 + 1 + 4) * 32),
}
CAP_OVER_BUDGET = ("up2_bwd",)


def cap_total(name: str) -> int:
    c = CAP_CASES[name]
    return c.N * c.per_image
