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

Most builders take an activation code.  With SiLU / GELU the pre-activations are drawn from a SATURATING set, where the kernels'
formulas return exactly 0 or exactly z (act64 below), so the same argument holds for the activation-bearing instantiations:
tests/test_exact_act_cpu.py and tests/test_exact_act_gpu.py.

FasterViT's batched coordinate MLPs (csrc/dfd_coord.hip) are held to tolerance 0 the same way: coord_mlp (integer coordinates with
zeros, so that pre-activations of exactly 0 occur) and coord_cpb (the chain MLP -> table -> 16 sigmoid(table[idx]) -> dtable -> MLP
backward at a table that paired hidden units make exactly 0); tests/test_coord_gpu.py runs the kernels on them, tests/test_exact_cpu.py
plain f32 torch and the oracle's PosEmb1D.  coord_shipped holds the shipped geometries on real numbers (a tolerance test) with the
condition under which its ReLU masks are determined (relu_margin).
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


# ------------------------------------------------------------------------------------- saturated SiLU / GELU (activation codes)
ACT_NONE, ACT_SILU, ACT_GELU = 0, 1, 3
ACTS = (ACT_SILU, ACT_GELU)
SAT_NEG, SAT_POS = (-128, -96), (32, 64)
SAT = SAT_NEG + SAT_POS
SAT_LEAN = SAT_NEG + (32, 32)                       # where K or the row count is large: one positive level (still every other draw)
SAT_DOWN = 2.0 ** -5                                # brings act(z) in {0, 32, 64} back to {0, 1, 2}: carried by the weights ...
SAT_GATES = (2.0 ** -5, 2.0 ** -4)                  # ... or by the gates of the BN + gate prologue
SAT_PROBE = (-65280, -32640, -2048, -256, -128, -96, 32, 64, 128, 256, 2048, 32640, 65280)   # the sets above and the reach of the epilogue tests
SAT_PROBE_GELU = (-64, -32)                         # GELU only (the 64 Z + 32 lattice of gemm_bias_act): SiLU is not saturated there
SAT_FLOOR = {1: -96, 3: -32}                        # act code -> the largest negative pre-activation a case may use (positive: >= 32)
SAT_QUANTUM = 2.0 ** -7                             # the smallest quantum any case here works in (xhat of bn_add_act_bwd)


def bn_state_sat(C: int, seed: int) -> torch.Tensor:
    """[4, C] f64 state in front of a saturated activation: scale in {16, 32, 64}, shift in {-32, 0, 32}, integer mean, rstd in
    {0.5, 1, 2}.  z - shift is a multiple of 32 for every z of SAT, so the raw input (z - shift) / scale is a multiple of 0.5 with
    |raw| <= 10: bf16 holds it, and xhat = (raw - mean) * rstd stays a small multiple of 1/4 for the statistics."""
    return torch.stack([pick((C,), seed, (16.0, 32.0, 64.0)), pick((C,), seed + 1, (-32, 0, 32)), pick((C,), seed + 2, (-1, 0, 1)),
                        pick((C,), seed + 3, POW2)])


def pick_balanced(shape, seed: int, vals) -> torch.Tensor:
    """pick(), but every row (all dimensions behind the first, an even count) holds each value as often as its negative: the
    operands behind an activation are >= 0, and a row of weights that adds up to zero keeps the mean of the outputs at zero."""
    n = 1
    for d in shape[1:]:
        n *= d
    assert n % 2 == 0
    half = pick((shape[0], n // 2), seed, vals)
    row = torch.cat([half, -half], 1)
    g = torch.Generator().manual_seed(seed + 1)
    perm = torch.argsort(torch.rand((shape[0], n), generator=g), 1)
    return torch.gather(row, 1, perm).reshape(tuple(shape))


def act64(z: torch.Tensor, act: int) -> torch.Tensor:
    """The activation as the float64 reference applies it: identity for code none; for SiLU / GELU max(z, 0), which is the
    correctly rounded value of the true function at every saturated z (tests/test_exact_act_cpu.py proves that for the sets
    used) - and an error of the test's data anywhere else.

    Saturation of the kernels' own formulas (csrc/dfd_common.h: sigmoid_f, gelu_parts and the packed-pair twins), emulated in f32
    with exp(v) = exp2(v * log2 e) and rcp(v) = 1 / v: SiLU gives (-0, -0) for z <= -89 (exp(-z) overflows, rcp(inf) = 0) and
    (z, 1) for z >= 17 (1 + exp(-z) rounds to 1); GELU gives (-0, 0) for z <= -16 and (z, 1) for z >= 6 (exp(-z*z / 2) underflows
    or drops out of 1 - x).  Measured on an MI355X by test_saturated_activations_probe (tests/test_exact_act_gpu.py), f32 and
    bf16, forward through bn_act_apply and derivative through act_bn_bwd: every point of SAT_PROBE, -65280 .. -96 and 32 .. 65280,
    comes back as -0 / z with derivative -0 / 1 under SiLU and as -0 / z with derivative 0 / 1 under GELU, and so do -64 and -32
    under GELU - the emulation's table, sign of zero included.  So the sets stay where the emulation put them.  (The probe holds
    the points the cases use and some beyond; the exact thresholds -89 / 17 and -16 / 6 are the emulation's and were not searched
    for on the device.)"""
    if act == ACT_NONE:
        return z
    if not bool(((z <= SAT_FLOOR[act]) | (z >= 32)).all()):
        raise ConditionViolated(f"a pre-activation lies outside the saturated ranges z <= {SAT_FLOOR[act]}, z >= 32")
    return torch.where(z > 0, z, torch.zeros_like(z))


def act_grad64(z: torch.Tensor, act: int) -> torch.Tensor:
    if act == ACT_NONE:
        return torch.ones_like(z)
    act64(z, act)
    return (z > 0).to(z.dtype)


def emulate_act_f32(z: torch.Tensor, act: int):
    """(act(z), act'(z)) by the kernels' formulas, operation for operation in f32 on the CPU (an FMA as the float64 sum rounded once
    to f32 - exact for these operands up to double rounding, which cannot happen at a saturated point)."""
    f = lambda t: t.to(F32)
    fma = lambda a, b, c: f(a.double() * b.double() + c.double())
    z = f(z)
    one = torch.ones_like(z)
    log2e = f(torch.tensor(1.44269504088896340736))
    if act == ACT_SILU:
        s = one / (one + torch.exp2(f(-z * log2e)))
        return f(z * s), f(s * f(one + f(z * f(one - s))))
    assert act == ACT_GELU
    x = f(z.abs() * f(torch.tensor(0.70710678118654752)))
    t = one / fma(f(torch.tensor(0.3275911)).expand_as(x), x, one)
    ez = torch.exp2(f(f(-x * x) * log2e))
    poly = f(torch.tensor(1.061405429)).expand_as(t)
    for c in (-1.453152027, 1.421413741, -0.284496736, 0.254829592):
        poly = fma(t, poly, f(torch.tensor(c)).expand_as(t))
    half_erfc = f(f(f(torch.tensor(0.5)) * f(t * poly)) * ez)
    cdf = torch.where(z >= 0, f(one - half_erfc), half_erfc)
    return f(z * cdf), fma(f(z * f(torch.tensor(0.39894228040143268))), ez, cdf)


def true_act64(z: torch.Tensor, act: int):
    """(act(z), act'(z)) of the mathematical function, float64, written so that the tails keep their relative accuracy."""
    z = z.double()
    if act == ACT_SILU:
        s = torch.sigmoid(z)
        return z * s, s * (1 + z * (1 - s))
    cdf = 0.5 * torch.special.erfc(-z / 2.0 ** 0.5)
    return z * cdf, cdf + z * torch.exp(-0.5 * z * z) / (2 * torch.pi) ** 0.5


def flush_denormals(t: torch.Tensor) -> torch.Tensor:
    """|v| < 2**-126 -> 0: torch's f32 sigmoid / gelu on the CPU return a denormal (silu(-96) ~ -2e-40) where the kernels' formula
    returns -0; the f32 oracle is compared after this flush."""
    return torch.where(t.abs() < 2.0 ** -126, torch.zeros_like(t), t)


def quantum_of(t: torch.Tensor) -> float:
    """The largest power of two in 2**-10 .. 2**10 that divides every element."""
    q = 2.0 ** 10
    while q > 2.0 ** -10 and not torch.equal(t / q, (t / q).round()):
        q /= 2
    return q


def nonzero_share(what: str, t: torch.Tensor) -> float:
    """About half of the operands behind a saturated activation are exact zeros; a dropped term shows only where it was not one."""
    share = float((t != 0).double().mean())
    if share < 0.40:
        raise ConditionViolated(f"{what}: only {share:.1%} of the operands behind the activation are non-zero")
    return share


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
def prologue64(a, mode, coef=None, a2=None, gate=None, act=ACT_NONE):
    """A operand [N, HW, K] after the GEMM prologue, float64; `act` (modes 1 and 2) at saturated pre-activations only."""
    if mode == 0:
        return a
    if mode == 3:
        return coef[0] * a + coef[1] * a2 + coef[2]
    v = act64(coef[0] * a + coef[1], act)
    return v * gate[:, None, :] if mode == 2 else v


def pro_inputs(target, mode, seed, act=ACT_NONE):
    """Raw inputs whose prologue of `mode` (0 none, 1 BN, 2 BN + gate, 3 affine2) gives `target` [N, HW, K].  With an activation
    (modes 1 and 2) `target` is the PRE-activation z, drawn from a saturating set: the raw input is un_bn(z), the operand behind
    the prologue max(z, 0), times a gate from SAT_GATES in mode 2."""
    N, _, K = target.shape
    if mode == 0:
        return NS(a=target, coef=None, a2=None, gate=None)
    if mode == 3:
        coef, a2 = coef3(K, seed), pick(target.shape, seed + 5, S2)
        return NS(a=un_affine2(target, a2, coef), coef=coef, a2=a2, gate=None)
    if act != ACT_NONE:
        st = bn_state_sat(K, seed)
        return NS(a=un_bn(target, st), coef=st, a2=None, gate=pick((N, K), seed + 7, SAT_GATES) if mode == 2 else None)
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


# The tiers of PW_FWD_CASES that take a prologue, and a ring shape whose 64-row tiles span four images (HW = 25; M = 1000 is 16 row
# tiles, the ring kernel's minimum): with HW = 64 (aligned), 103 and 197 above, the gate table of a tile holds 4, 1, 2 and 2 images
PW_ACT_CASES = [c for c in PW_FWD_CASES if c[0] != "gemm"] + [("ring", (40, 25, 136, 24), S2, S1)]
PW_ACT_MODES = (1, 2)


@functools.lru_cache(maxsize=4)
def pw_fwd_act(ci: int, mode: int, act: int):
    """pw_fwd for BN + act and BN + act + gate at saturated pre-activations: A = max(z, 0) [* gate]; the weights carry 2**-5 in mode 1,
    the gates in mode 2, so A w^T is a sum of small integers.  The weight rows are balanced (pick_balanced)."""
    tier, (N, HW, K, No), _, wset = PW_ACT_CASES[ci]
    what = f"pwconv {tier} {(N, HW, K, No)} mode {mode} act {act}"
    z = pick((N, HW, K), 100 + ci, SAT_LEAN if N * HW >= 65536 else SAT)
    inp = pro_inputs(z, mode, 200 + ci, act)
    w = pick_balanced((No, K), 300 + ci, wset) * (SAT_DOWN if mode == 1 else 1.0)
    A = prologue64(inp.a, mode, inp.coef, None, inp.gate, act)
    out = A @ w.t()
    share = nonzero_share(what, A)
    check_exact(what, operands=[("a", inp.a, DTYPES), ("A", A, DTYPES), ("w", w, DTYPES)],
                reductions=[("a w^T", A.abs() @ w.abs().t(), 1.0)], results=[("out", out, DTYPES)],
                stats=[("sum y*y", _abs_stats(out), 1.0)])
    return NS(what=what, tier=tier, shape=(N, HW, K, No), mode=mode, act=act, a=f32(inp.a).view(N, HW, 1, K), w=f32(w), coef=f32(inp.coef),
              a2=None, gate=None if inp.gate is None else f32(inp.gate), A=A, out=out.view(N, HW, 1, No), sums=sums64(out), has_stats=True,
              has_res=False, share=share, z=z)


# The eval form: out = act(scale * y + shift) behind the product, SiLU only.  y is an integer, scale in {256, 512} and shift = +-scale / 2, so
# z = (scale / 2) (2 y +- 1) is never 0 and |z| >= 128: saturated on either side whatever the product gives
PW_EVAL_CASES = (0, 2, 4, 5)                     # indices into PW_FWD_CASES: panel-resident and tile kernel, |y| <= 127


def eval_state(C: int, seed: int) -> torch.Tensor:
    scale = pick((C,), seed, (256.0, 512.0))
    return torch.stack([scale, scale / 2 * pick((C,), seed + 1, S1)])


def eval_result(what: str, y: torch.Tensor, st: torch.Tensor, dtypes) -> torch.Tensor:
    out = act64(st[0] * y + st[1], ACT_SILU)
    for dt in dtypes:
        if not representable(out, dt):
            raise ConditionViolated(f"{what}: the activated output is not exactly representable in {dt}")
    nonzero_share(what, out)
    return out


@functools.lru_cache(maxsize=2)
def pw_eval(ci: int):
    c = pw_fwd(ci, 0)
    No = c.shape[3]
    st = eval_state(No, 450 + ci)
    return NS(what=f"pwconv_eval {c.shape}", c=c, st=f32(st), out=eval_result(f"pwconv_eval {c.shape}", c.out.double(), st, DTYPES))


# ------------------------------------------------------------------------------------------ 1x1 weight gradient (pwconv_wgrad)
# (N, HW, Ni, Nj): p [N, HW, 1, Ni], q [N, HW, 1, Nj]; dw [Ni, Nj].  The PW_CASES shapes of tests/test_ops_gpu.py and two whose
# row count is 64 * 40 + 1 / 64 * 40 - 1: the last reduction step of the last split holds one row / misses one row
WGRAD_TILED_CASES = [(2, 49, 96, 16), (3, 100, 24, 96), (2, 196, 40, 240), (1, 333, 320, 1152), (4, 64, 144, 24), (2, 49, 1280, 320),
                     (2, 130, 8, 40), (13, 197, 40, 24), (3, 853, 24, 40)]
WGRAD_TILED_MODES = [(pm, qm) for pm in (0, 3) for qm in (0, 1, 2)]
# the wave-autonomous kernel, M >= 196,608 rows (bf16), values from {-1, 1}
WGRAD_LARGE_CASES = [(2, 100003, 32, 8), (3, 66001, 24, 144), (3, 66003, 144, 24)]
WGRAD_LARGE_MODES = [(0, 0), (3, 0), (0, 3)]


# with SiLU / GELU: the tiled kernel takes BN + act and BN + act + gate on q; the wave-autonomous kernel takes them on its WIDE operand
# only, BN + act + gate with SiLU and either mode of its narrow operand, BN + act with SiLU or GELU and affine2 on the narrow one
WGRAD_TILED_ACT_MODES = [(pm, qm) for pm in (0, 3) for qm in (1, 2)]
WGRAD_LARGE_ACT_MODES = [(0, 2, ACT_SILU), (3, 2, ACT_SILU), (3, 1, ACT_SILU), (3, 1, ACT_GELU)]      # (narrow mode, wide mode, act)


def tnw_serves(case, narrow_mode: int, wide_mode: int, act: int) -> bool:
    """The conditions under which pwconv_wgrad runs the wave-autonomous kernel in bf16 (dfd_pw_tnw / tnw_launch in csrc/dfd_pwtnw.hip;
    it has no plan function): M >= 196,608, narrow operand <= 32 channels, wide one <= 128 or 144, narrow mode none / affine2, a gate
    only with SiLU and H*W >= the 32- or 16-row step, BN + act only behind affine2 and with SiLU or GELU."""
    N, HW, Ni, Nj = case
    narrow, wide = min(Ni, Nj), max(Ni, Nj)
    ok = N * HW >= 2048 * 32 * 3 and narrow <= 32 and (wide <= 128 or (wide <= 144 and wide % 16 == 0)) and narrow_mode in (0, 3)
    if wide_mode == 2:
        return ok and act == ACT_SILU and HW >= (32 if wide <= 96 else 16)
    if wide_mode == 1:
        return ok and narrow_mode == 3 and act in ACTS
    return ok and not (wide_mode == 3 and narrow_mode == 3)


@functools.lru_cache(maxsize=6)
def pw_wgrad(case, pmode: int, qmode: int, large: bool = False, act: int = ACT_NONE):
    """With `act` the operand whose mode is 1 or 2 has saturated pre-activations (max(z, 0), times a gate from SAT_GATES in mode 2);
    in mode 1 the OTHER operand carries the 2**-5 instead, so every term of the sum is an integer either way."""
    N, HW, Ni, Nj = case
    what = f"pwconv_wgrad {case} p{pmode} q{qmode}" + (f" act {act}" if act else "")
    vals = S1 if large else S3
    sat = {m: act != ACT_NONE and m in (1, 2) for m in (pmode, qmode)}
    assert not (sat[pmode] and sat[qmode])

    def target(shape, seed, mine, other):
        if sat[mine]:
            return pick(shape, seed, SAT)
        return pick(shape, seed, vals) * (SAT_DOWN if sat[other] and other == 1 else 1.0)

    P, Q = target((N, HW, Ni), 500 + Ni, pmode, qmode), target((N, HW, Nj), 600 + Nj, qmode, pmode)
    ip, iq = pro_inputs(P, pmode, 700 + Ni, act), pro_inputs(Q, qmode, 800 + Nj, act)
    Pa, Qa = prologue64(ip.a, pmode, ip.coef, ip.a2, ip.gate, act), prologue64(iq.a, qmode, iq.coef, iq.a2, iq.gate, act)
    share = min([nonzero_share(what, t) for t, m in ((Pa, pmode), (Qa, qmode)) if sat[m]], default=1.0)
    M = N * HW
    dw = Pa.reshape(M, Ni).t() @ Qa.reshape(M, Nj)
    pre = pick((Ni, Nj), 900, S3)
    check_exact(what,
                operands=[("p", ip.a, DTYPES), ("q", iq.a, DTYPES), ("P", Pa, DTYPES), ("Q", Qa, DTYPES)]
                + [(n, t, DTYPES) for n, t in (("p2", ip.a2), ("q2", iq.a2)) if t is not None],
                reductions=[("p^T q", Pa.abs().reshape(M, Ni).t() @ Qa.abs().reshape(M, Nj) + pre.abs(), 1.0)],
                results=[("dw", dw, (F32,)), ("dw + preload", dw + pre, (F32,))])
    if quantum_of(Pa) * quantum_of(Qa) < 1.0:
        raise ConditionViolated(f"{what}: the terms of the sum are no integers")

    def ship(i, n):
        return NS(a=f32(i.a).view(N, HW, 1, n), coef=None if i.coef is None else f32(i.coef),
                  a2=None if i.a2 is None else f32(i.a2).view(N, HW, 1, n), gate=None if i.gate is None else f32(i.gate))

    return NS(what=what, shape=case, p=ship(ip, Ni), q=ship(iq, Nj), P=Pa, Q=Qa, dw=dw, pre=f32(pre), dw_acc=dw + pre, act=act, share=share)


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
# the matrix-core forward plans another tile behind an activating prologue here (two images per tile instead of one; three images: ragged)
DW_MM_ACT_CASE = (3, 9, 9, 96, 5, 2, 2, 2)
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
def dw(case, act: int = ACT_NONE):
    """One data set per shape.  xt / dyt: the operands as the kernels see them behind the BN prologue / the BN-backward map (also
    the inputs of the variants without them); x / dz: the raw inputs whose prologue / map gives them.
    With `act` the prologue is BN + SiLU / GELU at saturated pre-activations z: xt = max(z, 0) in {0, 32, 64}, the weights carry 2**-5
    and the output gradient 2**5, so y, the data gradient and its act' epilogue (dzin = da where z > 0, else 0) are small integers."""
    N, H, W, C, k, s, pt, pl = case
    what = f"depthwise {case}" + (f" act {act}" if act else "")
    Ho, Wo = -(-H // s), -(-W // s)
    if act:
        z = pick((N, H, W, C), 2000 + C, SAT)
        st = bn_state_sat(C, 2200 + C)
        x, xt = un_bn(z, st), act64(z, act)
        w = pick((C, 1, k, k), 2100 + C, S3) * SAT_DOWN
        dyt = pick((N, Ho, Wo, C), 2300 + C, S2) / SAT_DOWN
        share = nonzero_share(what, xt)
    else:
        xt = pick((N, H, W, C), 2000 + C, S3 if k == 3 else S2)
        w = pick((C, 1, k, k), 2100 + C, S3)
        st = bn_state(C, 2200 + C)
        x = un_bn(xt, st)
        z = xt
        dyt = pick((N, Ho, Wo, C), 2300 + C, S2)
        share = 1.0
    coef, yraw = coef3(C, 2400 + C), pick((N, Ho, Wo, C), 2500 + C, S2)
    dz = un_affine2(dyt, yraw, coef)
    xa, dy = act64(st[0] * x + st[1], act), coef[0] * dz + coef[1] * yraw + coef[2]
    y = dwconv64(xa, w, k, s, pt, pl, Ho, Wo)
    da, dwt = dwconv_bwd64(dy, xa, w, k, s, pt, pl)
    da_abs, dwt_abs = dwconv_bwd64(dy.abs(), xa.abs(), w.abs(), k, s, pt, pl)
    dzin = da * act_grad64(z, act)
    xhat = (x - st[2]) * st[3]
    check_exact(what,
                operands=[("x", x, DTYPES), ("xa", xa, DTYPES), ("w", w, DTYPES), ("dz", dz, DTYPES), ("yraw", yraw, DTYPES),
                          ("dy", dy, DTYPES)],
                reductions=[("taps", dwconv64(xa.abs(), w.abs(), k, s, pt, pl, Ho, Wo), 1.0), ("taps^T", da_abs, 1.0),
                            ("dy * xa", dwt_abs, quantum_of(dy) * quantum_of(xa) if act else 1.0)],
                results=[("y", y, DTYPES), ("da", da, DTYPES), ("dzin", dzin, DTYPES), ("dw", dwt, (F32,))],
                stats=[("sum y*y", _abs_stats(y), 1.0),
                       ("sum |dzin * xhat|", (dzin.abs() * xhat.abs()).reshape(-1, C).sum(0), 1.0 / 16)])
    if quantum_of(xa) * quantum_of(w) < 1.0 or quantum_of(dy) * quantum_of(w) < 1.0 or quantum_of(xhat) < 1.0 / 16:
        raise ConditionViolated(f"{what}: a term is no multiple of its quantum")
    return NS(what=what, shape=case, Ho=Ho, Wo=Wo, x=f32(x), xt=f32(xt), w=f32(w), st=f32(st), dz=f32(dz), dyt=f32(dyt),
              yraw=f32(yraw), coef=f32(coef), y=y, y_sums=sums64(y), da=da, dzin=dzin, dzin_sums=sums_xhat64(dzin, x, st), dw=dwt,
              act=act, share=share)


@functools.lru_cache(maxsize=2)
def dw_eval(case):
    """dwconv_eval: act(scale * dwconv(x) + shift) stored activated (SiLU), on the integer data of dw(case); and the channel sums of the
    stored tensor per image, which the kernel leaves as per-(tile, image) partial rows."""
    c = dw(case)
    C = case[3]
    what = f"dwconv_eval {case}"
    st = eval_state(C, 2600 + C)
    out = eval_result(what, c.y, st, DTYPES)
    check_exact(what, reductions=[("sums of the stored tensor", out.sum((1, 2)), quantum_of(out))], results=[("sums", out.sum((1, 2)), (F32,))])
    return NS(what=what, c=c, st=f32(st), out=out, img_sums=out.sum((1, 2)))


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
def rows(case, act: int = ACT_NONE):
    """With `act`: scale * y + shift = z from the saturating set, the pooling kernels add up max(z, 0), and dz = (...) * act'(z) is the
    plain dz where z > 0 and 0 elsewhere."""
    N, H, W, C = case
    what = f"row passes {case}" + (f" act {act}" if act else "")
    HW = H * W
    pow2_hw = HW & (HW - 1) == 0
    if act:
        st = bn_state_sat(C, 4000 + C)
        z = pick(case, 4100 + C, SAT)
        at, mask = act64(z, act), act_grad64(z, act)
        share = nonzero_share(what, at)
    else:
        st = bn_state(C, 4000 + C)
        z = pick(case, 4100 + C, S2)
        at, mask, share = z, torch.ones_like(z), 1.0   # scale * y + shift, what the pooling kernels add up
    y = un_bn(z, st)
    g = 2.0 * pick(case, 4200 + C, S2)                 # even: g * gate stays an integer
    rs = pick((N,), 4300, POW2)
    gate = pick((N, C), 4400, POW2)
    dpool = HW * pick((N, C), 4500, S3)                # dpool / (H*W) is an integer
    xhat = (y - st[2]) * st[3]
    rsb, gb, qb = rs[:, None, None, None], gate[:, None, None, :], (dpool / HW)[:, None, None, :]
    dzs = [g * mask, (g * gb + qb) * mask, qb.expand(N, H, W, C) * mask]
    flat = lambda t: t.reshape(-1, C)
    # f32 at an H*W that is no power of two: the stored dz is off by e = one f32 ulp of the quotient (plus the half ulp of the sum it
    # is a term of, mode 1), so the kernel's sums are no longer sums of exact terms.  Bound of ANY f32 summation order over n rows:
    # sum e * |xhat| for the terms themselves, plus (n + 2) * 2**-24 * sum |term| for the n - 1 additions and the two multiplications
    # by xhat (Higham, Accuracy and Stability of Numerical Algorithms, 4.4), with 1 % room for the second-order terms.
    rows_n = N * H * W
    sum_tol = [None]
    for m in (1, 2):
        e = (_spacing(qb.to(F32)).expand(N, H, W, C) + (0.5 * _spacing(dzs[m].to(F32)) if m == 1 else 0.0)) * mask
        u = (rows_n + 2) * 2.0 ** -24 * 1.01
        sum_tol.append(torch.stack([flat(e).sum(0) + u * flat(dzs[m]).abs().sum(0),
                                    flat(e * xhat.abs()).sum(0) + u * flat(dzs[m] * xhat).abs().sum(0)]))
    check_exact(what,
                operands=[("y", y, DTYPES), ("z", st[0] * y + st[1], DTYPES), ("a", at, DTYPES), ("g", g, DTYPES), ("g * rs", g * rsb, DTYPES)],
                reductions=[("pool", at.abs().sum((1, 2)), 1.0), ("pool bwd", (at * g).abs().sum((1, 2)), 1.0)],
                results=[(f"dz mode {m}", d, DTYPES) for m, d in enumerate(dzs)] + [("act(z)", at, DTYPES)],
                stats=[("sum |g rs|", flat(g * rsb).abs().sum(0), 0.5), ("sum |g rs xhat|", flat(g * rsb * xhat).abs().sum(0), 1.0 / 32),
                       ("sum g*g", flat(g * g).sum(0), 1.0)]
                + [(f"sum |dz xhat| mode {m}", flat(d * xhat).abs().sum(0), 1.0 / 16) for m, d in enumerate(dzs)])
    if not torch.equal(st[0] * y + st[1], z) or quantum_of(xhat) < 1.0 / 16:
        raise ConditionViolated(f"{what}: the BN of the raw input is not the pre-activation, or xhat is finer than 1/16")
    return NS(what=what, shape=case, HW=HW, pow2_hw=pow2_hw, y=f32(y), g=f32(g), st=f32(st), rs=f32(rs), gate=f32(gate), dpool=f32(dpool),
              red=sums_xhat64(g, y, st), red_rs=sums_xhat64(g * rsb, y, st), bias=flat(g).sum(0), bias_rs=flat(g * rsb).sum(0),
              dz=dzs, dz_sums=[sums_xhat64(d, y, st) for d in dzs], pooled=at.sum((1, 2)) / HW, pool_bwd=(at * g).sum((1, 2)), quot=qb, dz_sum_tol=sum_tol,
              g_stats=sums64(g), at=at, act=act, share=share)


ADD_ACT_CASE = (3, 7, 7, 40)


@functools.lru_cache(maxsize=2)
def bn_add(act: int):
    """bn_add_act / bn_add_act_bwd: out = act(scale * y + shift + other), d = g * act'(..), sums (d, d * xhat).  The pre-activation z is
    from the saturating set, the addend a small integer, so the raw y = (z - other - shift) / scale is a multiple of 1/64."""
    N, H, W, C = ADD_ACT_CASE
    what = f"bn_add_act {ADD_ACT_CASE} act {act}"
    st = bn_state_sat(C, 4900)
    z, other, g = pick(ADD_ACT_CASE, 4901, SAT), pick(ADD_ACT_CASE, 4902, S3), pick(ADD_ACT_CASE, 4903, S3)
    y = (z - other - st[1]) / st[0]
    pre = st[0] * y + st[1] + other
    out, d = act64(pre, act), g * act_grad64(pre, act)
    xhat = (y - st[2]) * st[3]
    nonzero_share(what, out)
    check_exact(what, operands=[("y", y, DTYPES), ("other", other, DTYPES), ("g", g, DTYPES), ("bn(y)", st[0] * y + st[1], (F32,))],
                results=[("out", out, DTYPES), ("d", d, DTYPES)],
                stats=[("sum |d|", d.abs().reshape(-1, C).sum(0), 1.0), ("sum |d xhat|", (d * xhat).abs().reshape(-1, C).sum(0), SAT_QUANTUM)])
    if not torch.equal(pre, z) or quantum_of(xhat) < SAT_QUANTUM:
        raise ConditionViolated(f"{what}: the pre-activation is not the chosen z, or xhat is finer than 2**-7")
    return NS(what=what, act=act, y=f32(y), other=f32(other), g=f32(g), st=f32(st), out=out, d=d, d_sums=sums_xhat64(d, y, st), pre=pre)


def probe_points(act: int):
    return SAT_PROBE + (SAT_PROBE_GELU if act == ACT_GELU else ())


@functools.lru_cache(maxsize=2)
def act_probe(act: int):
    """Every probe point in every channel position of a [1, points, 1, 16] tensor: the raw input is z / 32 behind a BN of scale 32."""
    C = 16
    pts = probe_points(act)
    z = torch.tensor(pts, dtype=torch.float64).view(1, -1, 1, 1).expand(1, len(pts), 1, C).contiguous()
    st = torch.stack([torch.full((C,), 32.0), torch.zeros(C), torch.zeros(C), torch.ones(C)]).double()
    y = un_bn(z, st)
    fwd, grad = torch.where(z > 0, z, torch.zeros_like(z)), (z > 0).double()
    check_exact("activation probe", operands=[("y", y, DTYPES), ("z", z, DTYPES)])
    return NS(z=z, y=f32(y), st=f32(st), ones=f32(torch.ones_like(z)), fwd=fwd, grad=grad)


MX_ROWS_CASE = (257, 256)                              # M, K of mx_quant_rows behind a saturated prologue (tests/test_mx_gpu.py)


@functools.lru_cache(maxsize=2)
def mx_rows(act: int):
    """mx_quant_rows behind BN + act: the values to quantise are max(z, 0) in {0, 32, 64}, which e4m3 with a power-of-two block scale
    holds exactly; the first block of row 0 is negative throughout (an all-zero block behind the activation)."""
    M, Kd = MX_ROWS_CASE
    z = pick((M, Kd), 4950, SAT)
    z[0, :32] = pick((32,), 4951, SAT_NEG)
    st = bn_state_sat(Kd, 4952)
    a = un_bn(z, st)
    want = act64(st[0] * a + st[1], act)
    nonzero_share(f"mx_quant_rows act {act}", want)
    check_exact(f"mx_quant_rows act {act}", operands=[("a", a, DTYPES), ("act(z)", want, DTYPES + (torch.float8_e4m3fn,))])
    return NS(a=f32(a), st=f32(st), want=want)


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
def conv(case, act: int = ACT_NONE):
    """With `act`: BN + act in front of the convolution at saturated pre-activations, xa = max(z, 0) in {0, 32}; the weights (balanced
    rows) carry 2**-5, so y is a sum of up to 9 C values from {-1, 0, 1}; the weight gradient is a multiple of 32."""
    k, s, p, C, Co, H, N = case
    what = f"dense conv {case}" + (f" act {act}" if act else "")
    Ho = (H + 2 * p - k) // s + 1
    M, Kd = N * Ho * Ho, k * k * C
    if act:
        z = pick((N, H, H, C), 5000 + C, SAT_LEAN)
        st = bn_state_sat(C, 5100 + C)
        x, xt = un_bn(z, st), act64(z, act)
        w = pick_balanced((Co, C, k, k), 5200 + Co, S1) * SAT_DOWN
        share = nonzero_share(what, xt)
    else:
        xt = pick((N, H, H, C), 5000 + C, S1)
        st = bn_state(C, 5100 + C)
        x = un_bn(xt, st)
        w = pick((Co, C, k, k), 5200 + Co, S1)
        share = 1.0
    xa = act64(st[0] * x + st[1], act)
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
    qa = quantum_of(xa) if act else 1.0                      # |P| = 1 and |col| <= qa: at most M quanta per sum
    if float(xa.abs().max()) > qa or quantum_of(xa) * quantum_of(w) < 1.0:
        raise ConditionViolated(f"{what}: the operand behind the prologue is not in {{-q, 0, q}}, or a tap is no integer")
    check_exact(what,
                operands=[("x", x, DTYPES), ("xa", xa, DTYPES), ("w", w, DTYPES), ("p", praw, DTYPES), ("p2", p2, DTYPES), ("P", Pa, DTYPES),
                          ("dcol", dcol, DTYPES)],
                reductions=[("taps", conv64(xa.abs(), w.abs()), 1.0), ("P^T col", torch.full((1,), float(M)), 1.0),
                            ("col2im", col2im64(dcol.abs(), (N, H, H, C), k, s, p), 1.0)],
                results=[("y", y, DTYPES), ("dw", dw, (F32,)), ("dx", dx, DTYPES)], stats=[("sum y*y", _abs_stats(y), 1.0)])
    return NS(what=what, shape=case, Ho=Ho, x=f32(x), xt=f32(xt), st=f32(st), w=f32(w), y=y, y_sums=sums64(y), p=f32(praw), pt=f32(P),
              p2=f32(p2), coef=f32(coef), dw=dw, dcol=f32(dcol), dx=dx, xa=xa, act=act, share=share)


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


# N, K, J of the classifier head.  (6, 1280, 10): fewer rows than one 8-row trip of the weight gradient, K a multiple of 64.
# (72, 176, 2), the EfficientFormerV2-S0 head: K % 64 = 48, nine 8-row trips, a second trip of the bias-gradient loop.
# (13, 224, 3): one 8-row trip and a remainder of 5, K % 64 = 32, a wave that holds 3 of its 4 outputs.
LINEAR_CASES = [(6, 1280, 10), (72, 176, 2), (13, 224, 3)]


@functools.lru_cache(maxsize=len(LINEAR_CASES))
def linear(case=LINEAR_CASES[0]):
    N, Kd, J = case
    x, w, b, dout = pick((N, Kd), 6400, S3), pick((J, Kd), 6401, S3), pick((J,), 6402, S3), pick((N, J), 6403, S3)
    out = matmul_case(f"linear_fwd {case}", x, w.t(), (F32,), (F32,)) + b
    dx = matmul_case(f"linear dx {case}", dout, w, (F32,), (F32,))
    dwt = matmul_case(f"linear dw {case}", dout.t(), x, (F32,), (F32,))
    db = dout.sum(0)
    check_exact(f"linear bias {case}", operands=[("b", b, (F32,))], reductions=[("db", dout.abs().sum(0), 1.0)],
                results=[("out", out, (F32,)), ("db", db, (F32,))])
    return NS(x=f32(x), w=f32(w), b=f32(b), dout=f32(dout), out=out, dx=dx, dw=dwt, db=db)


GEMM_BIAS_ACT_CASE = (256 * 80 + 17, 192, 520)          # M, K, N: served by dfd_gemm_bias_act (tests/test_vit_ops_gpu.py)


@functools.lru_cache(maxsize=2)
def gemm_bias_act(act: int = ACT_NONE):
    """out = act(scale * y + shift) * row_scale + residual with y = a w^T.  K is even and the operands are odd, so y is even; scale in
    {1, 2} and an even shift keep scale * y + shift even, so the row scales {0.5, 1} leave an integer for the bf16 store.
    With the GELU epilogue: scale 32 and shift 32 * (an odd number) put z = 32 (y + odd) into 64 Z + 32, which is never 0 and
    saturated either side; the row scales 2**-5 and 2**-4 bring max(z, 0) back to a small integer."""
    M, Kd, N = GEMM_BIAS_ACT_CASE
    a, w = pick((M, Kd), 6500, S1), pick((N, Kd), 6501, S1)
    y = matmul_case("gemm_bias_act product", a, w.t(), (BF16,), (BF16,))
    if act:
        st = torch.stack([torch.full((N,), 32.0, dtype=torch.float64), 32.0 * pick((N,), 6503, (-3, -1, 1, 3))])
        rs = pick((M,), 6504, SAT_GATES)
    else:
        st = torch.stack([pick((N,), 6502, (1.0, 2.0)), pick((N,), 6503, (-2, 0, 2))])
        rs = pick((M,), 6504, (0.5, 1.0))
    res = pick((M, N), 6505, S3)
    z = st[0] * y + st[1]
    if act and not torch.equal((z - 32) / 64, ((z - 32) / 64).round()):
        raise ConditionViolated("gemm_bias_act: a pre-activation is not in 64 Z + 32")
    za = act64(z, act)
    if act:
        nonzero_share("gemm_bias_act", za)
    out = za * rs[:, None] + res
    check_exact("gemm_bias_act epilogue", operands=[("z", z, (BF16,) if not act else (F32,)), ("act(z) * rs", za * rs[:, None], (BF16,)),
                                                    ("res", res, (BF16,))],
                results=[("out", out, (BF16,))])
    return NS(a=f32(a).view(M, 1, 1, Kd), w=f32(w), st=f32(st), rs=f32(rs), res=f32(res).view(M, 1, 1, N), y=y.view(M, 1, 1, N),
              out=out.view(M, 1, 1, N), act=act, z=z)


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


# ------------------------------------------------------------------- batched coordinate MLPs of FasterViT (csrc/dfd_coord.hip)
# (T, D, Hd) of table = relu(coords w0^T + b0) w2^T, the smallest shapes at which each branch of the kernels turns: one row / one
# column / one hidden quad; the shipped tables (16 and 49 rows x dim, 49 and 169 rows x heads); T = 64 | 65 (16 or 44 rows per row
# group in the backward), T = 88 | 89 (dtable staged 32 or 16 columns per pass) with D no multiple of either; T = 176 (the largest
# table) with Hd = 36 (one hidden chunk, 28 idle lanes); Hd = 1024 (the widest); D = 65 (one column behind the forward's 64-column
# chunk) at T = 25 (one row behind its 8-row chunk)
COORD_SHAPES = [(1, 1, 4), (16, 320, 512), (49, 256, 512), (49, 1024, 512), (49, 16, 512), (169, 8, 512), (64, 33, 1024), (65, 17, 512),
                (88, 40, 512), (89, 40, 512), (176, 70, 36), (25, 65, 512)]
COORD_GRID16 = len(COORD_SHAPES)                       # one more case: the 4 x 4 carrier grid's own coordinates (multiples of 1/2), dim 24
COORD_CASES = tuple(range(len(COORD_SHAPES) + 1))
COORD_SET = (-3, -2, -1, 0, 1, 2, 3)
COORD_B0 = (-3, -1, 0, 1, 3)


def grid_coords(s: int) -> torch.Tensor:
    """[s*s, 2] f64: (y, x) / (s // 2) - 1, the coordinates PosEmbMLPSwinv1D feeds its MLP."""
    ar = torch.arange(0, s, dtype=torch.float64)
    grid = torch.stack(torch.meshgrid([ar, ar], indexing="ij"))
    return ((grid - s // 2) / (s // 2)).flatten(1).t().contiguous()


def mlp64(coords, w0, b0, w2, dtable):
    """(pre-activation, table, dw0, db0, dw2) of table = relu(coords w0^T + b0) w2^T under the output gradient dtable, float64 by
    autograd: torch.relu passes no gradient at a pre-activation of exactly 0."""
    w0, b0, w2 = (t.clone().requires_grad_(True) for t in (w0, b0, w2))
    pre = coords @ w0.t() + b0
    table = torch.relu(pre) @ w2.t()
    table.backward(dtable)
    return pre.detach(), table.detach(), w0.grad, b0.grad, w2.grad


def _mlp_conditions(what, coords, w0, b0, w2, dtable, ref, q_dt=1.0):
    """check_exact for one MLP job: every sum stated as sum |term| per output (dw0 / db0 through dh)."""
    pre, table, dw0, db0, dw2 = ref
    qc = quantum_of(coords)
    h_abs = coords.abs() @ w0.abs().t() + b0.abs()                     # >= |pre| >= h: bounds the pre-activation's own sum too
    dh_abs = dtable.abs() @ w2.abs()
    mask = (pre > 0).double()
    check_exact(what,
                operands=[("coords", coords, (F32,)), ("w0", w0, (F32,)), ("b0", b0, (F32,)), ("w2", w2, (F32,)), ("dtable", dtable, (F32,))],
                reductions=[("coords w0^T + b0", h_abs, qc), ("h w2^T", h_abs @ w2.abs().t(), qc), ("dtable^T h", dtable.abs().t() @ h_abs, qc * q_dt),
                            ("dtable w2", dh_abs, q_dt), ("dh^T coords", (dh_abs * mask).t() @ coords.abs(), qc * q_dt),
                            ("sum dh", (dh_abs * mask).sum(0), q_dt)],
                results=[("table", table, (F32,)), ("dw0", dw0, (F32,)), ("db0", db0, (F32,)), ("dw2", dw2, (F32,))])
    if quantum_of(pre) < qc or quantum_of(dtable) < q_dt:
        raise ConditionViolated(f"{what}: a term is no multiple of its quantum")


@functools.lru_cache(maxsize=None)                       # the largest case holds 1024 x 512 doubles: the batch tests reuse all of them
def coord_mlp(ci: int):
    """One MLP job on integer data: coords in [-3, 3] (zeros included), w0 and w2 from S2, b0 from (-3, -1, 0, 1, 3), dtable from S3.
    Pre-activations of exactly 0 occur (h = 0 and no gradient through them); the builder asserts that they do wherever the case has a
    thousand pre-activations, and that some of them would carry a gradient if the mask let it through."""
    if ci == COORD_GRID16:
        T, D, Hd = 16, 24, 512
        coords = grid_coords(4)
    else:
        T, D, Hd = COORD_SHAPES[ci]
        coords = pick((T, 2), 8000 + ci, COORD_SET)
    what = f"coord MLP {(T, D, Hd)}" + (" on the 4 x 4 grid" if ci == COORD_GRID16 else "")
    w0, b0, w2 = pick((Hd, 2), 8100 + ci, S2), pick((Hd,), 8200 + ci, COORD_B0), pick((D, Hd), 8300 + ci, S2)
    dtable = pick((T, D), 8400 + ci, S3)
    ref = mlp64(coords, w0, b0, w2, dtable)
    _mlp_conditions(what, coords, w0, b0, w2, dtable, ref)
    pre = ref[0]
    at_zero = pre == 0
    if T * Hd >= 1000:
        share = float(at_zero.double().mean())
        if not 0.02 <= share <= 0.25:
            raise ConditionViolated(f"{what}: {share:.1%} of the pre-activations are exactly 0")
        if not bool(((dtable @ w2) * at_zero.double() != 0).any()):
            raise ConditionViolated(f"{what}: no unit with a pre-activation of 0 would carry a gradient")
    return NS(what=what, shape=(T, D, Hd), coords=f32(coords), w0=f32(w0), b0=f32(b0), w2=f32(w2), dtable=f32(dtable), pre=pre,
              table=ref[1], dw0=ref[2], db0=ref[3], dw2=ref[4], zeros=int(at_zero.sum()))


# (n_local, n_global, T, H, index): window attention with 4 carrier tokens, level 3's window attention, the carrier grid's attention -
# all with the relative position index of their window - and one job whose random index leaves table rows without a reference
CPB_GEOMS = [(49, 4, 169, 8, "window"), (49, 0, 169, 16, "window"), (16, 0, 49, 8, "window"), (49, 4, 169, 8, "sparse")]
SIGMOID_SAT = (-128, 64)                                # sigmoid_f gives exactly 0 / exactly 1 there (act64: z <= -89 / z >= 17)


def window_index(ws: int) -> torch.Tensor:
    """int32 [ws^4]: the relative position index of a ws x ws window (PosEmbMLPSwinv2D)."""
    ar = torch.arange(ws)
    pos = torch.flatten(torch.stack(torch.meshgrid([ar, ar], indexing="ij")), 1)
    rc = (pos[:, :, None] - pos[:, None, :]).permute(1, 2, 0).contiguous() + (ws - 1)
    return (rc[:, :, 0] * (2 * ws - 1) + rc[:, :, 1]).reshape(-1).to(torch.int32)


@functools.lru_cache(maxsize=None)
def coord_cpb(gi: int):
    """The whole "cpb" chain, exact end to end: MLP -> table -> bias = 16 sigmoid(table[idx]) -> dbias -> dtable -> MLP backward.
    The hidden units come in pairs with the same w0 / b0 row and opposite w2 columns, so the table of a non-trivial MLP is exactly 0
    in any summation order: bias = 8 in the local block and 0 in the carrier rows / columns, dtable = 16 * 0.5 * 0.5 * scatter(dbias),
    and the MLP backward goes on from there on integers.  `sat_*`: a second table from SIGMOID_SAT for the forward gather alone
    (bias = 0 or 16 by the row the index names; the derivative is 0 there, so the backward is checked at table = 0)."""
    nl, ng, T, H, kind = CPB_GEOMS[gi]
    Hd, S = 512, nl + ng
    what = f"cpb chain {CPB_GEOMS[gi]}"
    gen = torch.Generator().manual_seed(8500 + gi)
    if kind == "window":
        idx = window_index(int(nl ** 0.5))
    else:
        rows = torch.randperm(T, generator=gen)[: T // 2]                           # half of the rows are never named
        idx = rows[torch.randint(0, rows.numel(), (nl * nl,), generator=gen)].to(torch.int32)
    if int(idx.min()) < 0 or int(idx.max()) >= T:
        raise ConditionViolated(f"{what}: the index leaves the table")
    used = torch.zeros(T, dtype=torch.bool).index_fill_(0, idx.long(), True)
    if kind == "sparse" and int((~used).sum()) < T // 4:
        raise ConditionViolated(f"{what}: too few table rows without a reference")
    coords = pick((T, 2), 8600 + gi, COORD_SET)
    half_w0, half_b0, half_w2 = pick((Hd // 2, 2), 8700 + gi, S2), pick((Hd // 2,), 8800 + gi, COORD_B0), pick((H, Hd // 2), 8900 + gi, S2)
    w0, b0 = half_w0.repeat_interleave(2, 0), half_b0.repeat_interleave(2, 0)
    w2 = torch.stack([half_w2, -half_w2], 2).reshape(H, Hd)
    dbias = pick((H, S, S), 9000 + gi, S3)
    local = dbias[:, ng:, ng:].reshape(H, nl * nl)
    dtable = 4.0 * torch.zeros(H, T, dtype=torch.float64).index_add_(1, idx.long(), local).t().contiguous()
    dtable_abs = 4.0 * torch.zeros(H, T, dtype=torch.float64).index_add_(1, idx.long(), local.abs()).t()
    ref = mlp64(coords, w0, b0, w2, dtable)
    if float(ref[1].abs().max()) != 0.0 or float(torch.relu(ref[0]).max()) == 0.0:
        raise ConditionViolated(f"{what}: the table is not exactly 0 behind a non-trivial hidden layer")
    if bool((dtable[~used] != 0).any()) or not bool((dtable[used] != 0).any()):
        raise ConditionViolated(f"{what}: dtable is not zero exactly in the rows the index never names")
    check_exact(what, operands=[("dbias", dbias, (F32,))], reductions=[("scatter", dtable_abs, 1.0)], results=[("dtable", dtable, (F32,))])
    _mlp_conditions(what, coords, w0, b0, w2, dtable, ref, 4.0)
    bias = torch.zeros(H, S, S, dtype=torch.float64)
    bias[:, ng:, ng:] = 8.0
    sat_table = pick((T, H), 9100 + gi, SIGMOID_SAT)
    sat_bias = torch.zeros(H, S, S, dtype=torch.float64)
    sat_bias[:, ng:, ng:] = 16.0 * (sat_table[idx.long()] > 0).double().view(nl, nl, H).permute(2, 0, 1)
    return NS(what=what, geom=(nl, ng, T, H), shape=(T, H, Hd), idx=idx, used=used, coords=f32(coords), w0=f32(w0), b0=f32(b0), w2=f32(w2),
              dbias=f32(dbias), bias=bias, dtable=dtable, pre=ref[0], table=ref[1], dw0=ref[2], db0=ref[3], dw2=ref[4],
              sat_table=f32(sat_table), sat_bias=sat_bias)


# The shipped geometries on real numbers: (dim, tokens) of the position tables, (window, heads, tokens) of the attention biases
SHIPPED_POS = [(256, 49), (256, 16), (1024, 49)]
SHIPPED_CPB = [(7, 8, 53), (7, 16, 49), (4, 8, 16)]
SHIPPED_SEED = 0


def relu_margin(what: str, coords: torch.Tensor, w0: torch.Tensor, b0: torch.Tensor) -> float:
    """A hidden unit whose pre-activation changes sign between f32 and float64 moves dw0 / db0 by a whole term, not by rounding.  So
    every pre-activation v (float64, of the f32 operands) has to satisfy |v| > 4 * 2**-24 * (|cx w0x| + |cy w0y| + |b0|): four times
    the worst rounding of any f32 evaluation order, fused or not.  Returns the smallest |v| / bound; raises below 1."""
    c, w, b = coords.double(), w0.double(), b0.double()
    v = c @ w.t() + b
    bound = 4.0 * 2.0 ** -24 * (c.abs() @ w.abs().t() + b.abs())
    ratio = float((v.abs() / bound.clamp_min(1e-300)).min())
    if not bool((v.abs() > bound).all()):
        raise ConditionViolated(f"{what}: a pre-activation lies within f32 rounding of 0 (|v| / bound = {ratio:.3g}): its ReLU mask is "
                                f"not determined")
    return ratio


def randomise_cpb(module: torch.nn.Module, gen: torch.Generator) -> None:
    """As tests/test_fastervit_gpu.py randomise(): first layer N(0, 0.5), second N(0, 0.05), bias N(0, 0.1), drawn in f32."""
    with torch.no_grad():
        for name, p in module.named_parameters():
            if name.endswith("bias"):
                p.copy_(torch.randn(p.shape, generator=gen) * 0.1)
            else:
                p.copy_(torch.randn(p.shape, generator=gen) * (0.5 if p.shape[-1] == 2 else 0.05))


@functools.lru_cache(maxsize=2)
def coord_shipped(seed: int = SHIPPED_SEED):
    """The six coordinate MLPs of a hierarchical-attention block at the shipped sizes, weights as the model tests draw them.  Per job:
    the project's own coordinate / index buffers and the f32 parameters (what the kernels get), the oracle module carrying the same
    parameters in float64, its output and the gradients under a Gaussian output gradient.  relu_margin has passed for every job."""
    from deepfakedetection_amd.fastervit import PosEmbMLPSwinv1D, PosEmbMLPSwinv2D
    from oracle.fastervit_ref import PosEmb1D, PosEmb2D

    gen = torch.Generator().manual_seed(seed)
    jobs = []
    for kind, spec in [("pos", s) for s in SHIPPED_POS] + [("cpb", s) for s in SHIPPED_CPB]:
        if kind == "pos":
            dim, tokens = spec
            ours, ref32 = PosEmbMLPSwinv1D(dim, tokens), PosEmb1D(dim, tokens)
            coords, idx, nl, ng = ours._coords, None, 0, 0
        else:
            ws, heads, tokens = spec
            ours, ref32 = PosEmbMLPSwinv2D(ws, heads, tokens), PosEmb2D(ws, heads, tokens)
            coords, idx, nl, ng = ours._coords2d, ours._idx32, ws * ws, tokens - ws * ws
            if not torch.equal(idx.long(), ref32.relative_position_index.reshape(-1)):
                raise ConditionViolated(f"shipped {kind} {spec}: the project's index is not the oracle's")
        randomise_cpb(ref32, gen)
        w0, b0, w2 = (p.detach().clone() for p in (ref32.cpb_mlp[0].weight, ref32.cpb_mlp[0].bias, ref32.cpb_mlp[2].weight))
        what = f"shipped {kind} {spec} seed {seed}"
        margin = relu_margin(what, coords, w0, b0)
        out32 = (ref32.table(tokens)[0] if kind == "pos" else ref32.bias(tokens)[0]).detach()       # the oracle as the model tests run it
        ref64 = ref32.double()                                                      # the same f32 numbers, held as float64
        if kind == "pos":
            # PosEmb1D.table builds its grid in f32 inside the call, which a float64 module cannot take: the float64 reference is
            # the oracle's cpb_mlp on the same grid, after the grid has been checked against the oracle's formula
            if float((coords.double() - grid_coords(int(tokens ** 0.5))).abs().max()) > 2.0 ** -24:
                raise ConditionViolated(f"{what}: the project's coordinates are not the oracle's")
            out = ref64.cpb_mlp(coords.double())
        else:
            if not torch.equal(coords.double(), ref64.relative_coords_table.reshape(-1, 2)):
                raise ConditionViolated(f"{what}: the project's coordinates are not the oracle's")
            out = ref64.bias(tokens)[0]
        drift = float((out32.double() - out.detach()).abs().max() / out.detach().abs().max())
        if not drift <= 2e-6:
            raise ConditionViolated(f"{what}: the f32 oracle is {drift:.3g} of max |ref| away from its float64 form")
        g = torch.randn(out.shape, generator=gen)
        grads = torch.autograd.grad(out, [ref64.cpb_mlp[0].weight, ref64.cpb_mlp[0].bias, ref64.cpb_mlp[2].weight], g.double())
        jobs.append(NS(kind=kind, spec=spec, coords=coords.clone(), idx=idx, n_local=nl, n_global=ng, w0=w0, b0=b0, w2=w2, g=g,
                       out=out.detach(), dw0=grads[0], db0=grads[1], dw2=grads[2], margin=margin, drift=drift))
    return jobs


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
