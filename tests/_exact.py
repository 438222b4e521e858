"""TEST INFRASTRUCTURE - exact-arithmetic data for the reducing kernels (pure CPU; nothing here touches the GPU).

The technique: every operand is a small integer (or a small integer times a power of two), every coefficient a power of two
times a small integer.  Then every product, every partial sum IN ANY ORDER and every stored value is exactly representable, so
a kernel has to reproduce a float64 reference bit for bit - there is no rounding noise for a dropped tail element, a partial
row counted twice or a truncating store to hide under.

`check_exact` asserts the CONDITIONS under which that argument holds, on the CPU, before anything is launched:
  * every operand, after its prologue, is exactly representable in the storage dtype;
  * every reduction has sum |term| <= 2**24 quanta (the terms are multiples of `quantum`, a power of two), so every partial
    sum in every order is a multiple of the quantum below 2**24 quanta: an f32 holds it exactly;
  * every bf16-stored result is an integer with |v| <= 256, every f32 result has |v| <= 2**24 (and is representable);
  * statistics: the same bound on the total over all rows, so device-side and host-side partial sums are both exact.
A violated condition raises ConditionViolated: an error of the test's own data, never a skip.

The prologues (BatchNorm scale/shift, gate, the BN-backward map "affine2") are kept rich - scale, rstd, gate in {0.5, 1, 2},
integer shifts and means - by INVERTING them: the operand the kernel has to see after its prologue is drawn from a small
nonzero integer set, and the raw input is (target - shift) / scale, a short dyadic number that bf16 holds exactly.  The
float64 reference then applies the prologue forward to the raw input like the kernel does.

The builders below return the raw inputs (f32 tensors holding values every storage dtype represents), the float64 reference
and have run check_exact; tests/test_exact_cpu.py evaluates the f32 oracle on the same data, tests/test_exact_gpu.py the kernels.
"""

from __future__ import annotations

import functools
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

LIM = 2.0 ** 24
S1 = (-1, 1)
S2 = (-2, -1, 1, 2)
S3 = (-3, -2, -1, 1, 2, 3)
POW2 = (0.5, 1.0, 2.0)
SPOW2 = (-2.0, -1.0, -0.5, 0.5, 1.0, 2.0)
BF16, F32 = torch.bfloat16, torch.float32
DTYPES = (F32, BF16)


class ConditionViolated(Exception):
    """The test's own data leaves the range in which the arithmetic is exact."""


# ------------------------------------------------------------------------------------------------------------- generators
def pick(shape, seed: int, vals) -> torch.Tensor:
    """f64 tensor of `shape` drawn uniformly from the value set `vals` (no zeros in the sets above: a dropped term then
    always changes the sum)."""
    g = torch.Generator().manual_seed(seed)
    table = torch.tensor(vals, dtype=torch.float64)
    return table[torch.randint(0, len(vals), tuple(shape), generator=g)]


def bn_state(C: int, seed: int) -> torch.Tensor:
    """[4, C] f64: scale in {0.5, 1, 2}, integer shift, integer mean, rstd in {0.5, 1, 2}."""
    return torch.stack([pick((C,), seed, POW2), pick((C,), seed + 1, (-3, 0, 3)), pick((C,), seed + 2, (-1, 0, 1)),
                        pick((C,), seed + 3, POW2)])


def coef3(C: int, seed: int) -> torch.Tensor:
    """[3, C] f64 coefficients of d = a*g + b*y + c: a in {0.5, 1, 2}, b in +-{0.5, 1, 2}, integer c."""
    return torch.stack([pick((C,), seed, POW2), pick((C,), seed + 1, SPOW2), pick((C,), seed + 2, (-2, -1, 0, 1, 2))])


def un_bn(target: torch.Tensor, st: torch.Tensor) -> torch.Tensor:
    """raw with scale * raw + shift == target (channels last)."""
    return (target - st[1]) / st[0]


def un_affine2(target: torch.Tensor, a2: torch.Tensor, coef: torch.Tensor) -> torch.Tensor:
    """raw with coef[0] * raw + coef[1] * a2 + coef[2] == target."""
    return (target - coef[1] * a2 - coef[2]) / coef[0]


def f32(t: torch.Tensor) -> torch.Tensor:
    out = t.to(F32)
    if not torch.equal(out.double(), t.double()):
        raise ConditionViolated("a generated value is not an f32 number")
    return out.contiguous()


# ------------------------------------------------------------------------------------------------------------- conditions
def representable(t: torch.Tensor, dtype: torch.dtype) -> bool:
    t = t.double()
    return bool(torch.isfinite(t).all()) and torch.equal(t.to(dtype).double(), t)


def check_exact(what: str, operands=(), reductions=(), results=(), stats=()) -> None:
    """operands:   (name, f64 tensor as the kernel sees it after the prologue, storage dtypes it must be exact in)
    reductions: (name, tensor of sum |term| per output element, quantum of the terms)
    results:    (name, f64 reference, dtypes it is stored in)
    stats:      (name, per-channel sum |term| over all rows, quantum)"""
    for name, t, dtypes in operands:
        for dt in dtypes:
            if not representable(t, dt):
                raise ConditionViolated(f"{what}: operand {name} is not exactly representable in {dt}")
    for name, s, q in tuple(reductions) + tuple(stats):
        top = float(s.double().abs().max()) / q
        if not top <= LIM:
            raise ConditionViolated(f"{what}: reduction {name} has sum |term| = {top:.4g} quanta > 2**24")
    for name, t, dtypes in results:
        t = t.double()
        for dt in dtypes:
            if dt == BF16:
                if not (torch.equal(t, t.round()) and float(t.abs().max()) <= 256.0):
                    raise ConditionViolated(f"{what}: bf16 result {name} is not an integer tensor with |v| <= 256 "
                                            f"(max {float(t.abs().max())})")
            elif not (float(t.abs().max()) <= LIM and representable(t, F32)):
                raise ConditionViolated(f"{what}: f32 result {name} leaves the exact range (max {float(t.abs().max())})")


def same(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    """Bit equality of values: both sides to float64, torch.equal; the report names the damage."""
    g, w = got.detach().double().cpu(), want.detach().double().cpu()
    assert g.shape == w.shape, f"{what}: shape {tuple(g.shape)} vs {tuple(w.shape)}"
    if torch.equal(g, w):
        return
    bad = (g != w) | torch.isnan(g)
    idx = tuple(int(i) for i in bad.nonzero()[0])
    raise AssertionError(f"{what}: {int(bad.sum())} of {g.numel()} elements differ; first at {idx}: got {g[idx].item()!r}, "
                         f"want {w[idx].item()!r}")


def within_one_ulp(got: torch.Tensor, want64: torch.Tensor, what: str) -> None:
    """f32 `got` against the correctly rounded f32 of the float64 quotient, one f32 ulp either way (a multiplication by the
    rounded reciprocal and a division differ by at most that)."""
    g = got.detach().float().cpu()
    w = want64.double().to(F32)
    assert g.shape == w.shape, f"{what}: shape {tuple(g.shape)} vs {tuple(w.shape)}"
    lo, hi = torch.nextafter(w, torch.full_like(w, -float("inf"))), torch.nextafter(w, torch.full_like(w, float("inf")))
    bad = ~((g >= lo) & (g <= hi))
    if bool(bad.any()):
        idx = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {g.numel()} elements are more than one f32 ulp off; first at {idx}: "
                             f"got {g[idx].item()!r}, want {w[idx].item()!r}")


def _spacing(t32: torch.Tensor) -> torch.Tensor:
    """The f32 ulp at |t|, as float64."""
    a = t32.abs()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def within_quotient_ulp(got: torch.Tensor, want64: torch.Tensor, quotient64: torch.Tensor, what: str) -> None:
    """f32 `got` = integer + quotient, the quotient term within one f32 ulp of its correctly rounded value: the sum may then be
    off by that ulp (cancellation keeps it whole) plus the half ulp of its own rounding."""
    g, w = got.detach().double().cpu(), want64.double()
    assert g.shape == w.shape, f"{what}: shape {tuple(g.shape)} vs {tuple(w.shape)}"
    tol = _spacing(quotient64.to(F32)).expand_as(w) + 0.5 * _spacing(w.to(F32))
    bad = ~((g - w).abs() <= tol)
    if bool(bad.any()):
        idx = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {g.numel()} elements are further off than one f32 ulp of the quotient term; "
                             f"first at {idx}: got {g[idx].item()!r}, want {w[idx].item()!r}")


def sums_within(got: torch.Tensor, want64: torch.Tensor, tol64: torch.Tensor, what: str) -> None:
    """|got - want| <= tol, element by element (all float64)."""
    g, w = got.detach().double().cpu(), want64.double()
    assert g.shape == w.shape == tol64.shape, f"{what}: shape {tuple(g.shape)} vs {tuple(w.shape)}"
    bad = ~((g - w).abs() <= tol64)
    if bool(bad.any()):
        idx = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {g.numel()} sums are outside their bound; first at {idx}: got {g[idx].item()!r}, "
                             f"want {w[idx].item()!r} +- {tol64[idx].item():.3g}")


def sums64(y: torch.Tensor) -> torch.Tensor:
    """[2, C] f64: per-channel sum and sum of squares over all rows of a channels-last tensor."""
    flat = y.double().reshape(-1, y.shape[-1])
    return torch.stack([flat.sum(0), (flat * flat).sum(0)])


def sums_xhat64(d: torch.Tensor, x: torch.Tensor, st: torch.Tensor) -> torch.Tensor:
    """[2, C] f64: per-channel sum of d and of d * xhat, xhat = (x - mean) * rstd."""
    C = d.shape[-1]
    xhat = (x.double() - st[2]) * st[3]
    return torch.stack([d.double().reshape(-1, C).sum(0), (d.double() * xhat).reshape(-1, C).sum(0)])


def _abs_stats(y):
    return sums64(y)[1]             # sum y*y >= sum |y| for integers


# ------------------------------------------------------------------------------------------------ 1x1 forward (pwconv)
def prologue64(a, mode, coef=None, a2=None, gate=None):
    """A operand [N, HW, K] after the GEMM prologue, float64, activation none."""
    if mode == 0:
        return a
    if mode == 3:
        return coef[0] * a + coef[1] * a2 + coef[2]
    v = coef[0] * a + coef[1]
    return v * gate[:, None, :] if mode == 2 else v


def pro_inputs(target, mode, seed):
    """Raw inputs whose prologue of `mode` (0 none, 1 BN, 2 BN + gate, 3 affine2) gives `target` [N, HW, K]."""
    N, _, K = target.shape
    if mode == 0:
        return NS(a=target, coef=None, a2=None, gate=None)
    if mode == 3:
        coef, a2 = coef3(K, seed), pick(target.shape, seed + 5, S2)
        return NS(a=un_affine2(target, a2, coef), coef=coef, a2=a2, gate=None)
    st = bn_state(K, seed)
    if mode == 1:
        return NS(a=un_bn(target, st), coef=st, a2=None, gate=None)
    gate = pick((N, K), seed + 7, POW2)
    return NS(a=un_bn(target / gate[:, None, :], st), coef=st, a2=None, gate=gate)


# (tier, (N, HW, K, Nout), set of the operand after the prologue, set of the weights): the sets keep |y| <= 256 and sum y*y <= 2**24.
# K <= 64 with few column tiles is the panel-resident kernel's at any row count (it has no plan function to assert), so K = 16 and
# 40 are labelled "panel"; the tile kernel is reached with three K steps or more and few rows.
PW_FWD_CASES = [
    ("panel", (2, 49, 16, 96), S3, S3),
    ("tile", (1, 333, 1152, 320), S1, S1),
    ("panel", (2, 130, 40, 8), S2, S3),
    ("tile", (2, 49, 320, 1280), S1, S2),
    ("tile", (2, 130, 136, 8), S2, S1),            # three K steps and few rows: the panel-resident kernel declines, column tile 32
    ("tile", (2, 49, 200, 56), S1, S2),            # column tile 64
    ("panel", (3, 70001, 32, 16), S1, S1),
    ("panel", (3, 66003, 24, 144), S1, S1),
    ("ring", (17, 64, 136, 24), S2, S1),
    ("ring", (10, 103, 192, 8), S2, S1),
    ("ring", (50, 197, 112, 672), S1, S2),
    ("gemm", (1, 256 * 80 + 17, 192, 520), S1, S1),
]
PW_MODES = (0, 1, 2, 3)


def pw_modes(tier: str):
    """The 256-tile GEMM is the plain product.  The ring kernel takes the plain and the affine2 prologue with activation none; BN and
    BN + gate with activation none run the tile kernel on its shapes (the 128-row instance at 50 x 197 rows)."""
    return (0,) if tier == "gemm" else PW_MODES


@functools.lru_cache(maxsize=4)            # the four modes of one case stay while both dtypes walk them
def pw_fwd(ci: int, mode: int):
    tier, (N, HW, K, No), aset, wset = PW_FWD_CASES[ci]
    what = f"pwconv {tier} {(N, HW, K, No)} mode {mode}"
    target = pick((N, HW, K), 100 + ci, aset)
    inp = pro_inputs(target, mode, 200 + ci)
    w = pick((No, K), 300 + ci, wset)
    A = prologue64(inp.a, mode, inp.coef, inp.a2, inp.gate)
    out = A @ w.t()
    res = pick((N, HW, No), 400 + ci, S3)
    has_stats, has_res = mode != 3 and tier != "gemm", mode in (0, 3) and tier != "gemm"
    check_exact(what,
                operands=[("a", inp.a, DTYPES), ("A", A, DTYPES), ("w", w, DTYPES), ("res", res, DTYPES)]
                + ([("a2", inp.a2, DTYPES)] if mode == 3 else []),
                reductions=[("a w^T", A.abs() @ w.abs().t(), 1.0)],
                results=[("out", out, DTYPES)] + ([("out + res", out + res, DTYPES)] if has_res else []),
                stats=[("sum y*y", _abs_stats(out), 1.0)] if has_stats else [])
    return NS(what=what, tier=tier, shape=(N, HW, K, No), mode=mode, a=f32(inp.a).view(N, HW, 1, K), w=f32(w),
              coef=None if inp.coef is None else f32(inp.coef), a2=None if inp.a2 is None else f32(inp.a2).view(N, HW, 1, K),
              gate=None if inp.gate is None else f32(inp.gate), res=f32(res).view(N, HW, 1, No), A=A,
              out=out.view(N, HW, 1, No), sums=sums64(out), has_stats=has_stats, has_res=has_res,
              out_res=(out + res).view(N, HW, 1, No))


# ------------------------------------------------------------------------------------------ 1x1 weight gradient (pwconv_wgrad)
# (N, HW, Ni, Nj): p [N, HW, 1, Ni], q [N, HW, 1, Nj]; dw [Ni, Nj].  The PW_CASES shapes of tests/test_ops_gpu.py and two whose
# row count is 64 * 40 + 1 / 64 * 40 - 1: the last reduction step of the last split holds one row / misses one row
WGRAD_TILED_CASES = [(2, 49, 96, 16), (3, 100, 24, 96), (2, 196, 40, 240), (1, 333, 320, 1152), (4, 64, 144, 24), (2, 49, 1280, 320),
                     (2, 130, 8, 40), (13, 197, 40, 24), (3, 853, 24, 40)]
WGRAD_TILED_MODES = [(pm, qm) for pm in (0, 3) for qm in (0, 1, 2)]
# the wave-autonomous kernel, M >= 196,608 rows (bf16), values from {-1, 1}
WGRAD_LARGE_CASES = [(2, 100003, 32, 8), (3, 66001, 24, 144), (3, 66003, 144, 24)]
WGRAD_LARGE_MODES = [(0, 0), (3, 0), (0, 3)]


@functools.lru_cache(maxsize=6)
def pw_wgrad(case, pmode: int, qmode: int, large: bool = False):
    N, HW, Ni, Nj = case
    what = f"pwconv_wgrad {case} p{pmode} q{qmode}"
    vals = S1 if large else S3
    P = pick((N, HW, Ni), 500 + Ni, vals)
    Q = pick((N, HW, Nj), 600 + Nj, vals)
    ip, iq = pro_inputs(P, pmode, 700 + Ni), pro_inputs(Q, qmode, 800 + Nj)
    Pa, Qa = prologue64(ip.a, pmode, ip.coef, ip.a2, ip.gate), prologue64(iq.a, qmode, iq.coef, iq.a2, iq.gate)
    M = N * HW
    dw = Pa.reshape(M, Ni).t() @ Qa.reshape(M, Nj)
    pre = pick((Ni, Nj), 900, S3)
    check_exact(what,
                operands=[("p", ip.a, DTYPES), ("q", iq.a, DTYPES), ("P", Pa, DTYPES), ("Q", Qa, DTYPES)]
                + [(n, t, DTYPES) for n, t in (("p2", ip.a2), ("q2", iq.a2)) if t is not None],
                reductions=[("p^T q", Pa.abs().reshape(M, Ni).t() @ Qa.abs().reshape(M, Nj) + pre.abs(), 1.0)],
                results=[("dw", dw, (F32,)), ("dw + preload", dw + pre, (F32,))])

    def ship(i, n):
        return NS(a=f32(i.a).view(N, HW, 1, n), coef=None if i.coef is None else f32(i.coef),
                  a2=None if i.a2 is None else f32(i.a2).view(N, HW, 1, n), gate=None if i.gate is None else f32(i.gate))

    return NS(what=what, shape=case, p=ship(ip, Ni), q=ship(iq, Nj), P=Pa, Q=Qa, dw=dw, pre=f32(pre), dw_acc=dw + pre)


# -------------------------------------------------------------------------------------- fused expand backward (pwconv_bwd_fused)
FUSED_CASES = [(2048 * 96, 64, 8), (2048 * 96 + 3, 128, 32), (3 * 256 * 256 + 5, 144, 24)]       # (M, Cm, Cin)


@functools.lru_cache(maxsize=1)
def pw_fused(case):
    M, Cm, Cin = case
    what = f"pwconv_bwd_fused {case}"
    D = pick((M, Cm), 1000 + Cm, S1)
    coef, y = coef3(Cm, 1100 + Cm), pick((M, Cm), 1200 + Cm, S2)
    dz = un_affine2(D, y, coef)
    x, w, res = pick((M, Cin), 1300, S1), pick((Cm, Cin), 1400, S1), pick((M, Cin), 1500, S3)
    d = coef[0] * dz + coef[1] * y + coef[2]
    dx, dw = d @ w, d.t() @ x
    check_exact(what, operands=[("dz", dz, (BF16,)), ("y", y, (BF16,)), ("d", d, (BF16,)), ("x", x, (BF16,)), ("w", w, (BF16,)),
                                ("res", res, (BF16,))],
                reductions=[("d w", d.abs() @ w.abs(), 1.0), ("d^T x", d.abs().t() @ x.abs(), 1.0)],
                results=[("dx", dx, (BF16,)), ("dx + res", dx + res, (BF16,)), ("dw", dw, (F32,))])
    sh = lambda t, c: f32(t).view(M, 1, 1, c)
    return NS(what=what, shape=case, dz=sh(dz, Cm), y=sh(y, Cm), coef=f32(coef), x=sh(x, Cin), w=f32(w), res=sh(res, Cin),
              dx=dx.view(M, 1, 1, Cin), dx_res=(dx + res).view(M, 1, 1, Cin), dw=dw, d=d)


# ------------------------------------------------------------------------------------------------------------- depthwise
# N, H, W, C, k, s, pt, pl: the ragged and asymmetric entries of DW_CASES in tests/test_ops_gpu.py
DW_CASES = [(2, 15, 13, 24, 3, 2, 0, 0), (2, 16, 16, 48, 5, 2, 1, 1), (2, 29, 31, 192, 3, 1, 1, 1), (3, 9, 9, 8, 3, 1, 1, 1),
            (2, 7, 7, 1152, 5, 1, 2, 2)]
DW_SQUEEZED_CASE = (6, 30, 30, 144, 3, 1, 1, 1)      # several work items per workgroup once dfd_tune keys 8-11 squeeze the grid


def _same_pad(H, Ho, k, s, p0):
    return max((Ho - 1) * s + k - p0 - H, 0)


def dwconv64(xa, w, k, s, pt, pl, Ho, Wo):
    """Depthwise convolution of NHWC float64 xa with w [C, 1, k, k], TF-SAME bottom / right padding as the kernels'."""
    N, H, W, C = xa.shape
    pb, pr = _same_pad(H, Ho, k, s, pt), _same_pad(W, Wo, k, s, pl)
    an = F.pad(xa.permute(0, 3, 1, 2), (pl, pr, pt, pb))
    return F.conv2d(an, w, stride=s, groups=C)[:, :, :Ho, :Wo].permute(0, 2, 3, 1)


def dwconv_bwd64(dy, xa, w, k, s, pt, pl):
    """(d xa, dw) of y = dwconv64(xa, w), float64."""
    xa, w = xa.clone().requires_grad_(True), w.clone().requires_grad_(True)
    dwconv64(xa, w, k, s, pt, pl, dy.shape[1], dy.shape[2]).backward(dy)
    return xa.grad, w.grad


@functools.lru_cache(maxsize=2)
def dw(case):
    """One data set per shape.  xt / dyt: the operands as the kernels see them behind the BN prologue / the BN-backward map (also
    the inputs of the variants without them); x / dz: the raw inputs whose prologue / map gives them."""
    N, H, W, C, k, s, pt, pl = case
    what = f"depthwise {case}"
    Ho, Wo = -(-H // s), -(-W // s)
    xt = pick((N, H, W, C), 2000 + C, S3 if k == 3 else S2)
    w = pick((C, 1, k, k), 2100 + C, S3)
    st = bn_state(C, 2200 + C)
    x = un_bn(xt, st)
    dyt = pick((N, Ho, Wo, C), 2300 + C, S2)
    coef, yraw = coef3(C, 2400 + C), pick((N, Ho, Wo, C), 2500 + C, S2)
    dz = un_affine2(dyt, yraw, coef)
    xa, dy = st[0] * x + st[1], coef[0] * dz + coef[1] * yraw + coef[2]
    y = dwconv64(xa, w, k, s, pt, pl, Ho, Wo)
    da, dwt = dwconv_bwd64(dy, xa, w, k, s, pt, pl)
    da_abs, dwt_abs = dwconv_bwd64(dy.abs(), xa.abs(), w.abs(), k, s, pt, pl)
    xhat = (x - st[2]) * st[3]
    check_exact(what,
                operands=[("x", x, DTYPES), ("xa", xa, DTYPES), ("w", w, DTYPES), ("dz", dz, DTYPES), ("yraw", yraw, DTYPES),
                          ("dy", dy, DTYPES)],
                reductions=[("taps", dwconv64(xa.abs(), w.abs(), k, s, pt, pl, Ho, Wo), 1.0), ("taps^T", da_abs, 1.0),
                            ("dy * xa", dwt_abs, 1.0)],
                results=[("y", y, DTYPES), ("dzin", da, DTYPES), ("dw", dwt, (F32,))],
                stats=[("sum y*y", _abs_stats(y), 1.0),
                       ("sum |dzin * xhat|", (da.abs() * xhat.abs()).reshape(-1, C).sum(0), 1.0 / 16)])
    return NS(what=what, shape=case, Ho=Ho, Wo=Wo, x=f32(x), xt=f32(xt), w=f32(w), st=f32(st), dz=f32(dz), dyt=f32(dyt),
              yraw=f32(yraw), coef=f32(coef), y=y, y_sums=sums64(y), dzin=da, dzin_sums=sums_xhat64(da, x, st), dw=dwt)


# ------------------------------------------------------------------------------------------------------------------- stem
STEM_CASES = [(2, 32, 32, 32), (2, 33, 35, 40), (3, 32, 32, 48)]          # N, H, W, Cout; stride 2, 3x3
STEM_PADS = [(0, 0), (0, 1), (1, 1)]


def stem64(x, w, s, pt, pl, Ho, Wo):
    N, H, W, _ = x.shape
    k = w.shape[2]
    pb, pr = _same_pad(H, Ho, k, s, pt), _same_pad(W, Wo, k, s, pl)
    xn = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb))
    return F.conv2d(xn, w, stride=s)[:, :, :Ho, :Wo].permute(0, 2, 3, 1)


@functools.lru_cache(maxsize=2)
def stem(case, pad):
    N, H, W, Co = case
    pt, pl = pad
    what = f"stem {case} pad {pad}"
    Ho, Wo = -(-H // 2), -(-W // 2)
    x, w = pick((N, H, W, 3), 3000 + H, S3), pick((Co, 3, 3, 3), 3100 + Co, S3)
    y = stem64(x, w, 2, pt, pl, Ho, Wo)
    dyt = pick((N, Ho, Wo, Co), 3200, S2)
    coef, yraw = coef3(Co, 3300), pick((N, Ho, Wo, Co), 3400, S2)
    dz = un_affine2(dyt, yraw, coef)
    dy = coef[0] * dz + coef[1] * yraw + coef[2]
    wz = torch.zeros((Co, 3, 3, 3), dtype=torch.float64, requires_grad=True)
    stem64(x, wz, 2, pt, pl, Ho, Wo).backward(dy)
    wa = torch.zeros((Co, 3, 3, 3), dtype=torch.float64, requires_grad=True)
    stem64(x.abs(), wa, 2, pt, pl, Ho, Wo).backward(dy.abs())
    check_exact(what, operands=[("x", x, DTYPES), ("w", w, DTYPES), ("dz", dz, DTYPES), ("yraw", yraw, DTYPES), ("dy", dy, DTYPES)],
                reductions=[("taps", stem64(x.abs(), w.abs(), 2, pt, pl, Ho, Wo), 1.0), ("dy * x", wa.grad, 1.0)],
                results=[("y", y, DTYPES), ("dw", wz.grad, (F32,))], stats=[("sum y*y", _abs_stats(y), 1.0)])
    return NS(what=what, shape=case, pad=pad, Ho=Ho, Wo=Wo, x=f32(x), w=f32(w), y=y, y_sums=sums64(y), dz=f32(dz), dyt=f32(dyt),
              yraw=f32(yraw), coef=f32(coef), dw=wz.grad.detach())


# ------------------------------------------------------------------------------------------------------------- row passes
# 56 x 56 splits H*W over workgroups in the pooling kernels; 64 x 64 is the shape with thousands of rows (many partial rows) AND a
# power-of-two H*W, where every sum is exact in f32 as well
ROW_CASES = [(4, 5, 3, 672), (2, 8, 8, 1280), (3, 56, 56, 96), (3, 64, 64, 96)]


@functools.lru_cache(maxsize=2)
def rows(case):
    N, H, W, C = case
    what = f"row passes {case}"
    HW = H * W
    pow2_hw = HW & (HW - 1) == 0
    st = bn_state(C, 4000 + C)
    at = pick(case, 4100 + C, S2)                      # scale * y + shift, what the pooling kernels add up
    y = un_bn(at, st)
    g = 2.0 * pick(case, 4200 + C, S2)                 # even: g * gate stays an integer
    rs = pick((N,), 4300, POW2)
    gate = pick((N, C), 4400, POW2)
    dpool = HW * pick((N, C), 4500, S3)                # dpool / (H*W) is an integer
    xhat = (y - st[2]) * st[3]
    rsb, gb, qb = rs[:, None, None, None], gate[:, None, None, :], (dpool / HW)[:, None, None, :]
    dzs = [g, g * gb + qb, qb.expand(N, H, W, C)]
    flat = lambda t: t.reshape(-1, C)
    # f32 at an H*W that is no power of two: the stored dz is off by e = one f32 ulp of the quotient (plus the half ulp of the sum it
    # is a term of, mode 1), so the kernel's sums are no longer sums of exact terms.  Bound of ANY f32 summation order over n rows:
    # sum e * |xhat| for the terms themselves, plus (n + 2) * 2**-24 * sum |term| for the n - 1 additions and the two multiplications
    # by xhat (Higham, Accuracy and Stability of Numerical Algorithms, 4.4), with 1 % room for the second-order terms.
    rows_n = N * H * W
    sum_tol = [None]
    for m in (1, 2):
        e = _spacing(qb.to(F32)).expand(N, H, W, C) + (0.5 * _spacing(dzs[m].to(F32)) if m == 1 else 0.0)
        u = (rows_n + 2) * 2.0 ** -24 * 1.01
        sum_tol.append(torch.stack([flat(e).sum(0) + u * flat(dzs[m]).abs().sum(0),
                                    flat(e * xhat.abs()).sum(0) + u * flat(dzs[m] * xhat).abs().sum(0)]))
    check_exact(what,
                operands=[("y", y, DTYPES), ("a", st[0] * y + st[1], DTYPES), ("g", g, DTYPES), ("g * rs", g * rsb, DTYPES)],
                reductions=[("pool", at.abs().sum((1, 2)), 1.0), ("pool bwd", (at * g).abs().sum((1, 2)), 1.0)],
                results=[(f"dz mode {m}", d, DTYPES) for m, d in enumerate(dzs)],
                stats=[("sum |g rs|", flat(g * rsb).abs().sum(0), 0.5), ("sum |g rs xhat|", flat(g * rsb * xhat).abs().sum(0), 1.0 / 32),
                       ("sum g*g", flat(g * g).sum(0), 1.0)]
                + [(f"sum |dz xhat| mode {m}", flat(d * xhat).abs().sum(0), 1.0 / 16) for m, d in enumerate(dzs)])
    return NS(what=what, shape=case, HW=HW, pow2_hw=pow2_hw, y=f32(y), g=f32(g), st=f32(st), rs=f32(rs), gate=f32(gate), dpool=f32(dpool),
              red=sums_xhat64(g, y, st), red_rs=sums_xhat64(g * rsb, y, st), bias=flat(g).sum(0), bias_rs=flat(g * rsb).sum(0),
              dz=dzs, dz_sums=[sums_xhat64(d, y, st) for d in dzs], pooled=at.sum((1, 2)) / HW, pool_bwd=(at * g).sum((1, 2)), quot=qb, dz_sum_tol=sum_tol,
              g_stats=sums64(g), at=at)


SUM_ROWS_P = (1, 33, 1025)
SUM_ROWS_L = 1003


@functools.lru_cache(maxsize=3)
def sum_rows(P: int):
    """P partial rows (and the room the two-stage sum needs behind them, filled with values that must not be added)."""
    L = SUM_ROWS_L
    room = P + (min(P, 1024) + 31) // 32 + 1
    parts = pick((room, L), 4600 + P, S3)
    pre = pick((L,), 4700, S3)
    want = parts[:P].sum(0)
    check_exact(f"sum_rows {P}", operands=[("parts", parts, (F32,))], reductions=[("rows", parts[:P].abs().sum(0) + pre.abs(), 1.0)],
                results=[("sum", want, (F32,)), ("sum + preload", want + pre, (F32,))])
    return NS(P=P, L=L, parts=f32(parts), pre=f32(pre), want=want, want_acc=want + pre)


GRAD_SUMSQ_SIZES = (1, 3, 4095, 4096, 4097, 70001)


@functools.lru_cache(maxsize=1)
def grad_sumsq():
    gs = [pick((n,), 4800 + i, S3) for i, n in enumerate(GRAD_SUMSQ_SIZES)]
    check_exact("grad_sumsq", operands=[("g", g, (F32,)) for g in gs], reductions=[("g*g", (g * g).sum().reshape(1), 1.0) for g in gs])
    chunk = 4096                                                    # one table row per chunk of a tensor, as the optimizer's tables
    want = [(g[off:off + chunk] ** 2).sum() for g in gs for off in range(0, g.numel(), chunk)]
    return NS(gs=[f32(g) for g in gs], chunk=chunk, want=torch.stack(want))


# ------------------------------------------------------------------------------------------------------- dense convolution
# k, s, p, C, Cout, H, N: the cases of test_dense_conv_as_implicit_gemm (tests/test_vit_ops_gpu.py)
CONV_CASES = [(3, 1, 1, 64, 64, 28, 6), (3, 2, 1, 24, 48, 15, 3), (3, 1, 1, 128, 128, 9, 5), (3, 2, 1, 96, 192, 14, 2),
              (3, 1, 1, 96, 64, 14, 3), (3, 1, 1, 64, 128, 56, 2), (3, 1, 1, 128, 192, 17, 1), (3, 1, 1, 64, 48, 12, 2),
              (3, 1, 1, 80, 80, 56, 2), (3, 1, 1, 96, 96, 56, 2), (3, 1, 1, 160, 160, 28, 2), (3, 1, 1, 192, 192, 28, 2),
              (3, 1, 1, 256, 256, 28, 2),
              (3, 2, 1, 80, 160, 56, 2), (3, 2, 1, 96, 192, 56, 2), (3, 2, 1, 160, 320, 28, 2), (3, 2, 1, 192, 384, 28, 2),
              (3, 2, 1, 256, 512, 28, 2),
              (3, 2, 1, 32, 80, 112, 2), (3, 2, 1, 64, 96, 112, 2), (3, 2, 1, 64, 128, 112, 2)]


def im2col64(a, k, s, p, Ho):
    """[N, Ho, Ho, k*k*C] with column (kh*k + kw)*C + c, as the GEMM forms of the dense convolution read it."""
    N, _, _, C = a.shape
    unf = F.unfold(a.permute(0, 3, 1, 2), k, padding=p, stride=s)                 # [N, C*k*k, L] in (c, kh, kw) order
    return unf.view(N, C, k * k, Ho, Ho).permute(0, 3, 4, 2, 1).reshape(N, Ho, Ho, k * k * C)


def col2im64(dcol, in_shape, k, s, p):
    N, H, W, C = in_shape
    Ho = dcol.shape[1]
    back = dcol.view(N, Ho * Ho, k * k, C).permute(0, 3, 2, 1).reshape(N, C * k * k, Ho * Ho)
    return F.fold(back, (H, W), k, padding=p, stride=s).permute(0, 2, 3, 1)


@functools.lru_cache(maxsize=2)
def conv(case):
    k, s, p, C, Co, H, N = case
    what = f"dense conv {case}"
    Ho = (H + 2 * p - k) // s + 1
    M, Kd = N * Ho * Ho, k * k * C
    xt = pick((N, H, H, C), 5000 + C, S1)
    st = bn_state(C, 5100 + C)
    x = un_bn(xt, st)
    w = pick((Co, C, k, k), 5200 + Co, S1)
    xa = st[0] * x + st[1]
    conv64 = lambda a, ww: F.conv2d(a.permute(0, 3, 1, 2), ww, stride=s, padding=p).permute(0, 2, 3, 1)
    y = conv64(xa, w)
    P = pick((N, Ho, Ho, Co), 5300 + Co, S1)
    coef, p2 = coef3(Co, 5400 + Co), pick((N, Ho, Ho, Co), 5500 + Co, S2)
    praw = un_affine2(P, p2, coef)
    Pa = coef[0] * praw + coef[1] * p2 + coef[2]
    col = im2col64(xa, k, s, p, Ho)
    dw = Pa.reshape(M, Co).t() @ col.reshape(M, Kd)
    dcol = pick((N, Ho, Ho, Kd), 5600 + C, S1)
    dx = col2im64(dcol, (N, H, H, C), k, s, p)
    check_exact(what,
                operands=[("x", x, DTYPES), ("xa", xa, DTYPES), ("w", w, DTYPES), ("p", praw, DTYPES), ("p2", p2, DTYPES), ("P", Pa, DTYPES),
                          ("dcol", dcol, DTYPES)],
                reductions=[("taps", conv64(xa.abs(), w.abs()), 1.0), ("P^T col", torch.full((1,), float(M)), 1.0),
                            ("col2im", col2im64(dcol.abs(), (N, H, H, C), k, s, p), 1.0)],
                results=[("y", y, DTYPES), ("dw", dw, (F32,)), ("dx", dx, DTYPES)], stats=[("sum y*y", _abs_stats(y), 1.0)])
    return NS(what=what, shape=case, Ho=Ho, x=f32(x), xt=f32(xt), st=f32(st), w=f32(w), y=y, y_sums=sums64(y), p=f32(praw), pt=f32(P),
              p2=f32(p2), coef=f32(coef), dw=dw, dcol=f32(dcol), dx=dx)


# ----------------------------------------------------------------------------------------- matrix products of the ViT path
def matmul_case(what, a, b, dtypes_in, dtypes_out, alpha=1.0):
    """alpha * a @ b over leading batch dimensions, with the conditions checked."""
    out = alpha * (a @ b)
    check_exact(what, operands=[("a", a, dtypes_in), ("b", b, dtypes_in)], reductions=[("a b", a.abs() @ b.abs(), 1.0)],
                results=[("out", out, dtypes_out)])
    return out


BGEMM_CASE = (2, 8, 49, 196, 16, 64)                    # B, H, Nq, Nk, dk, dv of test_bgemm_large_k_and_rect


@functools.lru_cache(maxsize=1)
def bgemm():
    B, H, Nq, Nk, dk, dv = BGEMM_CASE
    q, k, v = pick((B, H, Nq, dk), 6000, S3), pick((B, H, Nk, dk), 6001, S3), pick((B, H, Nk, dv), 6002, S1)
    S = matmul_case("bgemm q k^T", q, k.transpose(-1, -2), (F32,), (F32,))
    O = matmul_case("bgemm S v", S, v, (F32,), (F32,))
    return NS(q=f32(q), k=f32(k), v=f32(v), S=S, O=O)


ATTN_APPLY_CASES = [(2, 8, 49, 37, 64), (2, 5, 130, 65, 24), (1, 2, 256, 256, 120), (1, 8, 64, 1, 96)]      # B, H, To, Tc, D


@functools.lru_cache(maxsize=2)
def attn_apply(case):
    """out_h = alpha * f_h x_h and alpha * f_h^T x_h: f f32 [B, H, To, Tc] (the kernel rounds it to bf16), x bf16 [B, Tc, 1, H*D]."""
    B, H, To, Tc, D = case
    f = 2.0 * pick((B, H, To, Tc), 6100 + Tc, S1)              # even: alpha = 0.5 leaves integers
    x = pick((B, Tc, 1, H * D), 6200 + Tc, S1)
    g = pick((B, To, 1, H * D), 6300 + To, S1)
    heads = lambda t, T: t.view(B, T, H, D).permute(0, 2, 1, 3)
    back = lambda t, T: t.permute(0, 2, 1, 3).reshape(B, T, 1, H * D)
    out = back(matmul_case(f"attn_apply {case}", f, heads(x, Tc), (BF16,), (BF16,), 0.5), To)
    out_t = back(matmul_case(f"attn_apply^T {case}", f.transpose(-1, -2), heads(g, To), (BF16,), (BF16,), 0.5), Tc)
    return NS(shape=case, f=f32(f), x=f32(x), g=f32(g), out=out, out_t=out_t)


LINEAR_CASE = (6, 1280, 10)                             # N, K, J of the classifier head


@functools.lru_cache(maxsize=1)
def linear():
    N, Kd, J = LINEAR_CASE
    x, w, b, dout = pick((N, Kd), 6400, S3), pick((J, Kd), 6401, S3), pick((J,), 6402, S3), pick((N, J), 6403, S3)
    out = matmul_case("linear_fwd", x, w.t(), (F32,), (F32,)) + b
    dx = matmul_case("linear dx", dout, w, (F32,), (F32,))
    dwt = matmul_case("linear dw", dout.t(), x, (F32,), (F32,))
    return NS(x=f32(x), w=f32(w), b=f32(b), dout=f32(dout), out=out, dx=dx, dw=dwt, db=dout.sum(0))


GEMM_BIAS_ACT_CASE = (256 * 80 + 17, 192, 520)          # M, K, N: served by dfd_gemm_bias_act (tests/test_vit_ops_gpu.py)


@functools.lru_cache(maxsize=1)
def gemm_bias_act():
    """out = (scale * y + shift) * row_scale + residual with y = a w^T.  K is even and the operands are odd, so y is even; scale in
    {1, 2} and an even shift keep scale * y + shift even, so the row scales {0.5, 1} leave an integer for the bf16 store."""
    M, Kd, N = GEMM_BIAS_ACT_CASE
    a, w = pick((M, Kd), 6500, S1), pick((N, Kd), 6501, S1)
    y = matmul_case("gemm_bias_act product", a, w.t(), (BF16,), (BF16,))
    st = torch.stack([pick((N,), 6502, (1.0, 2.0)), pick((N,), 6503, (-2, 0, 2))])
    rs, res = pick((M,), 6504, (0.5, 1.0)), pick((M, N), 6505, S3)
    z = st[0] * y + st[1]
    out = z * rs[:, None] + res
    check_exact("gemm_bias_act epilogue", operands=[("z", z, (BF16,)), ("z * rs", z * rs[:, None], (BF16,)), ("res", res, (BF16,))],
                results=[("out", out, (BF16,))])
    return NS(a=f32(a).view(M, 1, 1, Kd), w=f32(w), st=f32(st), rs=f32(rs), res=f32(res).view(M, 1, 1, N), y=y.view(M, 1, 1, N),
              out=out.view(M, 1, 1, N))


@functools.lru_cache(maxsize=1)
def vit_small():
    """avgpool k = 2, rowtable_grad, bias_scatter, relpos_bias_bwd, subsample_add_bwd: small scatter / gather sums."""
    x = 4.0 * pick((2, 14, 14, 32), 6600, S3)                                      # a mean of four stays an integer
    pooled = F.avg_pool2d(x.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    gp = 4.0 * pick((2, 7, 7, 32), 6601, S3)
    dpool = (gp / 4.0).repeat_interleave(2, 1).repeat_interleave(2, 2)
    gt = pick((6, 49, 1, 64), 6602, S3)
    H, res = 8, 7
    n = res * res
    pos = torch.stack(torch.meshgrid(torch.arange(res), torch.arange(res), indexing="ij")).flatten(1)
    rel = (pos[..., :, None] - pos[..., None, :]).abs()
    idx = (rel[0] * res + rel[1]).to(torch.int32).reshape(-1)                       # timm Attention2d.attention_bias_idxs
    dfull = pick((H, n * n), 6603, S3)
    scat = torch.zeros(H, n, dtype=torch.float64).index_add_(1, idx.long(), dfull)
    # relative-position bias 16 * sigmoid(table[idx]) at table = 0: the derivative is 16 * 0.5 * 0.5 = 4, exactly
    nl, ng, T = 49, 4, 169
    ridx = torch.randint(0, T, (nl * nl,), generator=torch.Generator().manual_seed(6604)).to(torch.int32)
    dbias = pick((H, nl + ng, nl + ng), 6605, S3)
    local = dbias[:, ng:, ng:].reshape(H, nl * nl)
    dtable = 4.0 * torch.zeros(H, T, dtype=torch.float64).index_add_(1, ridx.long(), local).t()
    dtable_abs = 4.0 * torch.zeros(H, T, dtype=torch.float64).index_add_(1, ridx.long(), local.abs()).t()
    gs, dx0 = pick((2, 7, 7, 24), 6606, S3), pick((2, 14, 14, 24), 6607, S3)
    dx1 = dx0.clone()
    dx1[:, ::2, ::2] += gs
    check_exact("ViT scatter / gather sums",
                operands=[("x", x, DTYPES), ("gp", gp, DTYPES), ("gt", gt, DTYPES), ("gs", gs, DTYPES), ("dx0", dx0, DTYPES)],
                reductions=[("avgpool", 4.0 * x.abs().amax().reshape(1), 1.0), ("rowtable", gt.abs().sum(0), 1.0),
                            ("scatter", torch.zeros(H, n, dtype=torch.float64).index_add_(1, idx.long(), dfull.abs()), 1.0),
                            ("relpos", dtable_abs, 1.0)],
                results=[("pooled", pooled, DTYPES), ("dpool", dpool, DTYPES), ("dtable", gt.sum(0).view(49, 64), (F32,)),
                         ("scatter", scat, (F32,)), ("relpos dtable", dtable, (F32,)), ("subsample bwd", dx1, DTYPES)])
    return NS(x=f32(x), pooled=pooled, gp=f32(gp), dpool=dpool, gt=f32(gt), rowtable=gt.sum(0).view(49, 64), idx=idx, dfull=f32(dfull),
              scat=scat, n=n, ridx=ridx, dbias=f32(dbias), nl=nl, ng=ng, T=T, H=H, dtable=dtable, gs=f32(gs), dx0=f32(dx0), dx1=dx1)


# ------------------------------------------------------------------------------------------- rounding of the bf16 stores
TIE_FACTOR = 1.5
# 1.5 * m / 128 for an odd 8-bit significand m < 171 is exactly half way between two bf16 numbers: m = 129 -> the even neighbour lies
# above (193.5 -> 194), m = 131 -> below (196.5 -> 196), alternating from there
TIE_PARTNERS = tuple(m / 128.0 for m in range(129, 171, 2))


def rand_bf16(shape, seed: int) -> torch.Tensor:
    """f32 tensor of random bf16 numbers: sign, an 8-bit significand in [128, 255], an exponent in [-3, 3]."""
    g = torch.Generator().manual_seed(seed)
    sig = torch.randint(128, 256, tuple(shape), generator=g).double() / 128.0
    ex = torch.randint(-3, 4, tuple(shape), generator=g).double()
    sign = torch.randint(0, 2, tuple(shape), generator=g).double() * 2 - 1
    return (sign * sig * torch.exp2(ex)).to(F32)


def tie_partners(n: int, seed: int) -> torch.Tensor:
    """n f32 values whose product with TIE_FACTOR is a bf16 tie, both kinds alternating, over several binades and both signs."""
    g = torch.Generator().manual_seed(seed)
    base = torch.tensor(TIE_PARTNERS, dtype=torch.float64)[torch.arange(n) % len(TIE_PARTNERS)]
    ex = torch.randint(-3, 4, (n,), generator=g).double()
    sign = torch.randint(0, 2, (n,), generator=g).double() * 2 - 1
    return (sign * base * torch.exp2(ex)).to(F32)


def truncate_bf16(p: torch.Tensor) -> torch.Tensor:
    """What a store that drops the low 16 bits of the f32 would write."""
    return (p.to(F32).contiguous().view(torch.int32) & -65536).view(F32)


def rounding_reference(u: torch.Tensor, v: torch.Tensor, what: str) -> torch.Tensor:
    """bf16 reference of the single products u * v (broadcast), with the conditions of the rounding tests: both factors are bf16
    numbers (so the f32 product is exact), truncation would differ in at least 40 % of the outputs, and at least 16 outputs are
    exact ties with both kinds present (even neighbour below / above)."""
    for name, t in (("u", u), ("v", v)):
        if not representable(t, BF16):
            raise ConditionViolated(f"{what}: factor {name} is not a bf16 tensor")
    p64 = u.double() * v.double()
    p = p64.to(F32)
    if not torch.equal(p.double(), p64):
        raise ConditionViolated(f"{what}: a product of two bf16 numbers must be exact in f32")
    want = p.to(BF16)                                                         # round to nearest, ties to even
    trunc = truncate_bf16(p)
    share = float((trunc != want.float()).double().mean())
    if share < 0.40:
        raise ConditionViolated(f"{what}: truncation differs from rounding in only {share:.1%} of the outputs")
    up = (trunc.view(torch.int32) + 65536).view(F32)                          # the next bf16 number away from zero
    tie = (p64 - trunc.double()).abs() == (up.double() - p64).abs()
    tie &= trunc.double() != p64
    even_below = tie & ((trunc.view(torch.int32) >> 16) & 1 == 0)
    even_above = tie & ~even_below
    if int(tie.sum()) < 16 or int(even_below.sum()) < 4 or int(even_above.sum()) < 4:
        raise ConditionViolated(f"{what}: {int(tie.sum())} ties ({int(even_below.sum())} with the even neighbour below, "
                                f"{int(even_above.sum())} above): too few")
    assert torch.equal(want.float()[even_below], trunc[even_below]) and torch.equal(want.float()[even_above], up[even_above])
    return want


def same_bits(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    """Bit equality of two bf16 tensors."""
    assert got.dtype == BF16 and want.dtype == BF16 and got.shape == want.shape, f"{what}: {got.dtype} {tuple(got.shape)}"
    g, w = got.detach().cpu().contiguous().view(torch.int16), want.contiguous().view(torch.int16)
    if torch.equal(g, w):
        return
    bad = g != w
    idx = tuple(int(i) for i in bad.nonzero()[0])
    raise AssertionError(f"{what}: {int(bad.sum())} of {g.numel()} stored bf16 values differ from round-to-nearest-even; first at {idx}: "
                         f"got {got.detach().cpu()[idx].item()!r}, want {want[idx].item()!r}")


# (tier, M, K, Nout) of the 1x1 forward: one nonzero per row of the activations, at column m % K, so every output is ONE product.
# K = 8 where the tier takes it (the panel-resident kernel keeps every K = 8 shape); the tile kernel needs three K steps of 64 and
# few rows, the ring kernel K >= 64 and 17 row tiles or more, the 256-tile GEMM K % 64 == 0 and 160 tiles or more
ROUND_PW_CASES = [("panel", 98, 8, 96), ("panel", 70001, 8, 16), ("tile", 333, 136, 24), ("ring", 17 * 64, 136, 24),
                  ("gemm", 256 * 80 + 17, 192, 520)]


@functools.lru_cache(maxsize=1)
def round_pw(ci: int):
    tier, M, K, No = ROUND_PW_CASES[ci]
    u, w = rand_bf16((M,), 7000 + ci), rand_bf16((No, K), 7100 + ci)
    w[0, :] = TIE_FACTOR                                     # output channel 0 of the first rows: constructed ties
    n = min(M, 64)
    u[:n] = tie_partners(n, 7200 + ci)
    cols = torch.arange(M) % K
    a = torch.zeros((M, K), dtype=F32)
    a[torch.arange(M), cols] = u
    want = rounding_reference(u[:, None], w[:, cols].t(), f"1x1 forward {tier} rounding")
    return NS(tier=tier, shape=(M, K, No), a=a.view(1, M, 1, K), w=w, want=want.view(1, M, 1, No))


@functools.lru_cache(maxsize=1)
def round_rows():
    """[N, H, W, C] values times a per-channel / per-(image, channel) / per-image factor: channel 0 (image 0) carries the ties."""
    N, H, W, C = 3, 9, 7, 48                 # C % 16 == 0: the depthwise forward has its matrix-core form at this shape too
    x = rand_bf16((N, H, W, C), 7300)
    x[0].view(-1, C)[:, 0] = tie_partners(H * W, 7301)
    chan, img_chan, img = rand_bf16((C,), 7302), rand_bf16((N, C), 7303), rand_bf16((N,), 7304)
    chan[0], img_chan[0, 0], img[0] = TIE_FACTOR, TIE_FACTOR, TIE_FACTOR
    return NS(shape=(N, H, W, C), x=x, chan=chan, img_chan=img_chan, img=img,
              by_chan=rounding_reference(x, chan, "per-channel factor"),
              by_img_chan=rounding_reference(x, img_chan[:, None, None, :], "per-(image, channel) factor"),
              by_img=rounding_reference(x, img[:, None, None, None], "per-image factor"))
