"""TEST INFRASTRUCTURE - data for the attention path's kernels at every tier (pure CPU; nothing here touches the GPU).

The batched GEMM (dfd_bgemm: three kernels), the softmax rows (dfd_attn_softmax_fwd / _bwd: R rows per workgroup, TEAM threads per
(head, row) pair) and the fused window attention (dfd_wattn_fwd / _bwd: two templates, 16-token tiles) each choose a kernel or a
launch shape from the problem size.  The builders below hold one case per choice and per boundary between two choices, with the tier
each case is MEANT to land on; tests/test_attn_tiers_cpu.py asserts the tiers through the planner exports (dfd_bgemm_plan,
dfd_attn_softmax_plan: host code) and evaluates plain f32 torch on the same data, tests/test_attn_tiers_gpu.py runs the kernels.

Products: the technique of tests/_exact.py (small nonzero integers, conditions asserted by check_exact, float64 reference, tolerance 0).

Softmax at tolerance 0: the logits are 256 * a_h * sel with sel in {0, 1} marking one key or 2**k keys of a row and a_h a positive
integer.  Every unmarked logit is at least 256 below the row maximum, so its exponential is 0 in f32 (e**-256 ~ 1e-111); the marked
ones give exp(0) = 1, the row sum is exactly 2**k and P is exactly 2**-k on the marked keys.  The fused window attention reaches
the same state with GROUPS of 2**k keys whose k rows are identical (scale * q k ties inside a group for any q) and a bias of 0 on the
query's group, -256 elsewhere: o is then the exact mean of the group's v rows.
"""

from __future__ import annotations

import functools
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

from tests._exact import BF16, DTYPES, F32, S1, S2, S3, ConditionViolated, check_exact, f32, matmul_case, pick, representable

GENERAL, SMALL, KRED, UNSUPPORTED = 0, 1, 2, -2          # dfd_bgemm_plan's answers (include/dfd_hip.h)

# ----------------------------------------------------------------------------------------------------------------- dfd_bgemm
# name -> (tier, (M, N, K), (nb, nh), options).  Options: a / b / c = storage order of the operand ("mk" | "km", "kn" | "nk", "mn" | "nm":
# the second letter is the unit-stride index), epi = bias and alpha = 0.5, round = operand that is rounded to bf16 after loading.
BGEMM_CASES = {
    "kred 8x8x512": (KRED, (8, 8, 512), (2, 2), {}),                        # the threshold itself
    "kred 5x3x1000": (KRED, (5, 3, 1000), (2, 3), {}),                      # M, N < 8, K no multiple of 256
    "kred 5x3x1000 epi": (KRED, (5, 3, 1000), (3, 2), {"epi": True}),
    "kred 8x8x512 km nk nm": (KRED, (8, 8, 512), (1, 3), {"a": "km", "b": "nk", "c": "nm"}),
    "small 16x16x385": (SMALL, (16, 16, 385), (2, 2), {}),                  # first K past the 48 KiB rule
    "small 9x8x1000": (SMALL, (9, 8, 1000), (3, 1), {}),                    # M = 9: one past kred
    "small 9x8x1000 epi": (SMALL, (9, 8, 1000), (1, 3), {"epi": True}),
    "small 16x1x615": (SMALL, (16, 1, 615), (2, 3), {}),                    # N = 1, first K past the rule with Np = 4
    "small 13x11x700": (SMALL, (13, 11, 700), (2, 2), {}),                  # two chunks of 256 and a remainder of 188
    "small 13x11x700 km nk": (SMALL, (13, 11, 700), (2, 2), {"a": "km", "b": "nk"}),
    "small 13x11x700 km": (SMALL, (13, 11, 700), (1, 2), {"a": "km"}),
    "small 16x1x615 nk nm": (SMALL, (16, 1, 615), (3, 1), {"b": "nk", "c": "nm"}),
    "general 8x8x511": (GENERAL, (8, 8, 511), (2, 2), {}),                  # the other side of K >= 512
    "general 16x16x384": (GENERAL, (16, 16, 384), (2, 2), {}),              # panels of exactly 48 KiB
    "general 17x16x385": (GENERAL, (17, 16, 385), (2, 1), {}),              # M = 17: one past small
    "general 3x5x1": (GENERAL, (3, 5, 1), (3, 2), {}),                      # M, N no multiples of 4, K = 1
    "general 49x37x32": (GENERAL, (49, 37, 32), (2, 3), {}),
    "general 49x37x32 epi": (GENERAL, (49, 37, 32), (3, 2), {"epi": True}),
    "general 64x64x300": (GENERAL, (64, 64, 300), (1, 2), {}),              # panels of exactly 150 KiB
    "general 49x37x32 nm": (GENERAL, (49, 37, 32), (2, 2), {"c": "nm"}),    # C written transposed through sc
    "general 49x37x32 km nk": (GENERAL, (49, 37, 32), (2, 2), {"a": "km", "b": "nk"}),
    "general 17x16x385 round a": (GENERAL, (17, 16, 385), (2, 2), {"round": "a"}),
    "general 17x16x385 round b": (GENERAL, (17, 16, 385), (2, 2), {"round": "b"}),
}
BGEMM_REFUSED = [((64, 64, 301), False), ((8, 8, 2401), True)]              # ((M, N, K), round_a): DFD_EUNSUPPORTED
BGEMM_ALL_DTYPES = "general 49x37x32"                                        # all eight (A, B, C) dtype combinations run here
BGEMM_MODEL_DTYPES = ("kred 8x8x512", "small 16x16x385")                     # the three combinations the models use run here
MODEL_DTYPES = [(F32, F32, F32), (F32, BF16, BF16), (BF16, BF16, F32)]
ALL_DTYPES = [(a, b, c) for a in DTYPES for b in DTYPES for c in DTYPES]


def bgemm_lds(M: int, N: int, K: int) -> int:
    """Bytes of the two f32 panels of the general kernel (the quantity the 48 KiB and 150 KiB rules are about)."""
    return (K * ((M + 3) & ~3) + K * ((N + 3) & ~3)) * 4


def _stored(t: torch.Tensor, transposed: bool):
    """(contiguous f32 storage of [nb, nh, R, C] `t`, (sb, sh, sr, sc)) - row-major, or with the last two dimensions swapped."""
    nb, nh, R, C = t.shape
    if transposed:
        return f32(t.transpose(-1, -2)), (nh * R * C, R * C, 1, R)
    return f32(t), (nh * R * C, R * C, C, 1)


@functools.lru_cache(maxsize=4)
def bgemm_case(name: str):
    tier, (M, N, K), (nb, nh), opt = BGEMM_CASES[name]
    what = f"bgemm {name}"
    if not 2 <= nb * nh <= 6:
        raise ConditionViolated(f"{what}: nb * nh must lie in 2 .. 6 (the per-(b, h) base offsets)")
    vals = S3 if K <= 64 else S1
    epi, rnd = opt.get("epi", False), opt.get("round")
    seed = 7000 + 13 * M + 7 * N + K
    a, b = pick((nb, nh, M, K), seed, vals), pick((nb, nh, K, N), seed + 1, vals)
    alpha = 1.0
    if epi:
        a, alpha = 2.0 * a, 0.5                                   # even: alpha = 0.5 leaves integers
    bias = pick((nh, M, N), seed + 2, S3) if epi else None
    a_in, b_in = a, b
    if rnd is not None:
        # f32 operands that are NO bf16 numbers: v (1 + 2**-10) rounds (to nearest, no tie) to the integer v.  The reference rounds first.
        noisy = (a if rnd == "a" else b) * (1.0 + 2.0 ** -10)
        if representable(noisy, BF16) or not torch.equal(noisy.to(F32).to(BF16).double(), a if rnd == "a" else b):
            raise ConditionViolated(f"{what}: the noisy operand is a bf16 number, or does not round to the integer")
        a_in, b_in = (noisy, b) if rnd == "a" else (a, noisy)
    dts_in = DTYPES if rnd is None else (F32,)
    out = matmul_case(what, a, b, DTYPES, DTYPES, alpha)
    if epi:
        out = out + bias
        check_exact(what, operands=[("bias", bias, (F32,))], results=[("out + bias", out, DTYPES)])
    check_exact(what, operands=[("a as stored", a_in, dts_in), ("b as stored", b_in, dts_in)])
    A, sa = _stored(a_in, opt.get("a", "mk") == "km")
    B, sb = _stored(b_in, opt.get("b", "kn") == "nk")
    c_t = opt.get("c", "mn") == "nm"
    sc = (nh * M * N, M * N, 1, M) if c_t else (nh * M * N, M * N, N, 1)
    return NS(what=what, tier=tier, M=M, N=N, K=K, nb=nb, nh=nh, A=A, sa=sa, B=B, sb=sb, sc=sc, c_t=c_t, c_shape=(nb, nh, N, M) if c_t else (nb, nh, M, N),
              alpha=alpha, bias=None if bias is None else f32(bias), round_a=rnd == "a", round_b=rnd == "b", dtypes_in=dts_in, out=out,
              a64=a, b64=b)


# The talking-head weight and bias gradients of EfficientFormerV2 as attn_core_bwd (deepfakedetection_amd/vit_functions.py) calls them:
# (H, L = Nq * Nk, images).  dW[g][h] = sum_{b, l} d[b, g, l] p[b, h, l]: per image a [H, L] x [L, H] product with nh = 1 and zero head
# strides, the second operand read transposed through its strides; db[g] = sum d[b, g, :] against a ones operand whose strides are all 0.
TH_GRAD_CASES = [(8, 2401, 3), (8, 784, 4)]


@functools.lru_cache(maxsize=2)
def th_grad(case):
    H, L, B = case
    what = f"talking-head gradients {case}"
    d, p = pick((B, H, L), 7500 + L, S1), pick((B, H, L), 7501 + L, S1)
    parts_w = matmul_case(what + " dW rows", d, p.transpose(-1, -2), (F32,), (F32,))                  # [B, H, H]
    parts_b = matmul_case(what + " db rows", d, torch.ones(B, L, 1, dtype=torch.float64), (F32,), (F32,))      # [B, H, 1]
    dw, db = torch.einsum("bgl,bhl->gh", d, p), d.sum((0, 2))
    check_exact(what, reductions=[("over images", parts_w.abs().sum(0), 1.0), ("over images, bias", parts_b.abs().sum(0), 1.0)],
                results=[("dW", dw, (F32,)), ("db", db, (F32,))])
    return NS(what=what, H=H, L=L, B=B, d=f32(d), p=f32(p), parts_w=parts_w, parts_b=parts_b.view(B, H), dw=dw, db=db)


# q, k, v heads read in place from [B * T][H * hd] bf16 projection outputs (the 16-byte staging path of the general kernel: unit-stride
# rows whose length and pitch are multiples of 8 on a 16-byte aligned base), head_dim 40 as in FasterViT-1.  The GPU test runs it once more
# on storage that starts 8 bytes into an allocation: no base is 16-byte aligned then and every operand takes the element path.
HEADS_CASE = (2, 3, 17, 40, 24)                           # B, H, T, dk, dv


@functools.lru_cache(maxsize=1)
def bgemm_heads():
    B, H, T, dk, dv = HEADS_CASE
    q, k, v = pick((B, T, H, dk), 7600, S2), pick((B, T, H, dk), 7601, S2), pick((B, T, H, dv), 7602, S3)
    w = pick((B, H, T, T), 7603, S3)                                                                   # f32 A operand of w v
    heads = lambda t: t.permute(0, 2, 1, 3)
    S = matmul_case("bgemm heads q k^T", heads(q), heads(k).transpose(-1, -2), (BF16,), DTYPES)
    O = matmul_case("bgemm heads w v", w, heads(v), DTYPES, DTYPES)
    return NS(q=f32(q).view(B * T, H * dk), k=f32(k).view(B * T, H * dk), v=f32(v).view(B * T, H * dv), w=f32(w), S=S,
              O=O.permute(0, 2, 1, 3).reshape(B * T, H * dv))


# ------------------------------------------------------------------------------------------------------------- softmax rows
# (H, Nk, R, TEAM): the launch shape dfd_attn_softmax_plan must report, computed from the rule once and kept as literals
SOFTMAX_LATTICE = [
    (16, 16, 16, 1), (8, 4, 32, 1), (16, 1, 16, 1),       # TEAM 1: FasterViT-1/-2/-3 carrier tokens; H lowers R to 32; clamp and lowering
    (8, 16, 16, 2), (3, 7, 36, 2), (2, 3, 64, 2),         # TEAM 2: ..., H no power of two, R clamped to 64
    (4, 16, 16, 4), (1, 3, 64, 4),
    (8, 53, 4, 8), (2, 16, 16, 8),
    (5, 100, 2, 16), (16, 256, 1, 16),
    (1, 256, 1, 32), (1, 29, 8, 32),
]
SOFTMAX_EXACT = [(16, 16), (8, 53), (1, 256)]             # TEAM 1, 8, 32
SOFTMAX_BIG_LOGITS = (8, 53)                              # |S| ~ 80: the max subtraction
SOFTMAX_TOL = NS(P=2e-5, T2=2e-5, dS=2e-4, dW1=5e-4)      # tests/test_vit_ops_gpu.py, test_attn_softmax_rows_match_autograd


def plan_rule(H: int, Nk: int):
    """The rule of csrc/dfd_vit.hip restated: (R, TEAM)."""
    R = min(256 // Nk, 64)
    while H * R > 256:
        R -= 1
    team = 1
    while team < 32 and team * 2 * H * R <= 256:
        team *= 2
    return R, team


def softmax_rows(R: int):
    """(B, Nq) with B * Nq >= 2 R + 1 rows (and at least 4: the exact cases mark 1, 2, 4, 8 keys by row) and a last workgroup that is
    not full (where R > 1)."""
    B = 3
    Nq = -(-max(2 * R + 1, 4) // B)
    while R > 1 and (B * Nq) % R == 0:
        Nq += 1
    return B, Nq


def softmax64(S, th, g):
    """float64: (P, T2, dS, dT1, dW1) of T1 = conv(S, w1) + b1, P = softmax(T1), T2 = conv(P, w2) + b2 under the gradient g of T2."""
    S = S.double().clone().requires_grad_()
    H = S.shape[1]
    if th is None:
        P = S.softmax(-1)
        P.backward(g.double())
        return NS(P=P.detach(), T2=P.detach(), dS=S.grad, dT1=None, dW1=None)
    w1, b1, w2, b2 = [t.double().clone().requires_grad_() for t in th]
    T1 = F.conv2d(S, w1.view(H, H, 1, 1), b1)
    T1.retain_grad()
    P = T1.softmax(-1)
    T2 = F.conv2d(P, w2.view(H, H, 1, 1), b2)
    T2.backward(g.double())
    return NS(P=P.detach(), T2=T2.detach(), dS=S.grad, dT1=T1.grad, dW1=w1.grad)


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=2)
def softmax_case(H: int, Nk: int, talk: bool, amplitude: float = 2.0):
    """Gaussian logits (standard deviation `amplitude`) on the lattice point (H, Nk), f32 inputs and the float64 reference."""
    R, team = plan_rule(H, Nk)
    B, Nq = softmax_rows(R)
    if B * Nq < 2 * R + 1 or (R > 1 and (B * Nq) % R == 0):
        raise ConditionViolated(f"softmax rows ({H}, {Nk}): {B * Nq} rows do not leave a ragged last workgroup of R = {R}")
    shape = (B, H, Nq, Nk)
    S = _randn(shape, 8000 + H * 257 + Nk) * amplitude
    th = None
    if talk:
        th = (_randn((H, H), 8001) * 0.4, _randn((H,), 8002), _randn((H, H), 8003) * 0.4, _randn((H,), 8004))
    g = _randn(shape, 8005)
    return NS(shape=shape, R=R, team=team, S=S, th=th, g=g, ref=softmax64(S, th, g))


def _conv64(w, x):
    return torch.einsum("hg,bgij->bhij", w, x)


@functools.lru_cache(maxsize=2)
def softmax_exact(H: int, Nk: int, talk: bool):
    """Logits 256 a_h sel; P = 2**-k on the 2**k marked keys of a row (k = row index mod 4, capped by Nk) and 0 elsewhere, exactly."""
    what = f"exact softmax ({H}, {Nk}) talk {talk}"
    R, team = plan_rule(H, Nk)
    B, Nq = softmax_rows(R)
    while B * Nq * 15 < 4 * (Nk + 15) or (R > 1 and (B * Nq) % R == 0):     # enough rows (15 marks per 4) to mark every key somewhere
        Nq += 1
    gen = torch.Generator().manual_seed(8100 + H * 257 + Nk)
    order = torch.randperm(Nk, generator=gen)                               # the rows take their keys from this order, cyclically:
    sel = torch.zeros(B, Nq, Nk, dtype=torch.float64)                       # distinct inside a row, and every key is marked in some row
    count = torch.zeros(B, Nq, 1, dtype=torch.float64)
    at = 0
    for r in range(B * Nq):
        k = r % 4
        while (1 << k) > Nk:
            k -= 1
        keys = order[(at + torch.arange(1 << k)) % Nk]
        at += 1 << k
        sel[r // Nq, r % Nq, keys] = 1.0
        count[r // Nq, r % Nq] = float(1 << k)
    if not bool((sel.sum((0, 1)) > 0).all()):
        raise ConditionViolated(f"{what}: a key is marked in no row (a kernel that left it out would go unnoticed)")
    a = pick((H,), 8101, (1, 2, 3))
    S = 256.0 * a.view(1, H, 1, 1) * sel.view(B, 1, Nq, Nk)
    P = (sel / count).view(B, 1, Nq, Nk).expand(B, H, Nq, Nk).contiguous()
    th_f = th_b = None
    T1, T2 = S, P
    if talk:
        w1 = pick((H, H), 8102, (-1, 0, 1))
        c = w1 @ a
        for h in range(H):                                        # the row sums against a stay positive: every head keeps its maximum on the marked keys
            if c[h] < 1:
                w1[h, h] += torch.ceil((1 - c[h]) / a[h])
        if not bool(((w1 @ a) >= 1).all()):
            raise ConditionViolated(f"{what}: a row of w1 has no positive sum against the amplitudes")
        b1, w2, b2 = pick((H,), 8103, S3), pick((H, H), 8104, (-1, 0, 1)), pick((H,), 8105, S3)
        T1 = _conv64(w1, S) + b1.view(1, H, 1, 1)
        T2 = _conv64(w2, P) + b2.view(1, H, 1, 1)
        th_f = (f32(w1), f32(b1), f32(w2), f32(b2))
        w1b = pick((H, H), 8106, (-1, 0, 1))                      # the backward takes P as an input: its own w1 from {-1, 0, 1}
        th_b = (f32(w1b), None, f32(w2), None)
    # every unmarked logit at least 256 below the row maximum, every marked one AT the maximum
    top = T1.max(-1, keepdim=True).values
    marked = sel.view(B, 1, Nq, Nk).expand_as(T1) > 0
    if not (bool((T1[marked] == top.expand_as(T1)[marked]).all()) and bool((top.expand_as(T1)[~marked] - T1[~marked] >= 256).all())):
        raise ConditionViolated(f"{what}: a marked logit is below its row maximum, or an unmarked one less than 256 below it")
    dT2 = pick((B, H, Nq, Nk), 8107, S3)
    dP = _conv64(w2.t(), dT2) if talk else dT2                                                         # W2^T dT2
    dT1 = P * (dP - (dP * P).sum(-1, keepdim=True))
    dS = _conv64(w1b.t(), dT1) if talk else dT1
    check_exact(what, operands=[("S", S, (F32,)), ("T1", T1, (F32,)), ("dT2", dT2, (F32,))],
                reductions=[("W1 S", _conv64(w1.abs(), S.abs()) if talk else S.abs(), 1.0), ("dP P", (dP * P).abs().sum(-1), 2.0 ** -3)],
                results=[("P", P, (F32,)), ("T2", T2, (F32,)), ("dT1", dT1, (F32,)), ("dS", dS, (F32,))])
    return NS(what=what, shape=(B, H, Nq, Nk), R=R, team=team, S=f32(S), th=th_f, th_bwd=th_b, P=P, T2=T2, dT2=f32(dT2), dT1=dT1, dS=dS)


# ------------------------------------------------------------------------------------------------ fused window attention
WATTN_HD = 32
WATTN_SCALE = 0.125
WATTN_EXACT = [(5, 53, 2), (3, 32, 2), (6, 17, 1)]        # n, T, H: four tiles with 11 padded tokens; the NT = 2 boundary; two tiles, 15 padded
WATTN_LOG2_GROUP = (0, 1, 2, 3)


@functools.lru_cache(maxsize=2)
def wattn_exact(case, k: int):
    """qkv [n, T, 3 C] of integers: keys in groups of 2**k with identical k rows, bias 0 on a query's chosen group and -256 elsewhere.
    o = the mean of the group's v rows (v holds multiples of 2**k), dv = 2**-k times the sum of the dO rows of the queries that chose
    the key's group (dO holds multiples of 2**k).  k = 0: L is the selected logit, dq, dk and dbias are exactly zero."""
    n, T, H = case
    hd, C, gs = WATTN_HD, H * WATTN_HD, 1 << k
    G = T // gs
    what = f"exact window attention {case} groups of {gs}"
    if G < 2:
        raise ConditionViolated(f"{what}: fewer than two groups")
    seed = 9000 + 100 * T + 10 * k
    q = pick((n, T, H, hd), seed, S2)
    kgrp = pick((n, G, H, hd), seed + 1, S2)
    kk = pick((n, T, H, hd), seed + 2, S2)                                 # tokens behind the last whole group keep rows of their own
    kk[:, :G * gs] = kgrp.repeat_interleave(gs, dim=1)
    v = float(gs) * pick((n, T, H, hd), seed + 3, S3)
    dO = float(gs) * pick((n, T, H, hd), seed + 4, S3)
    gen = torch.Generator().manual_seed(seed + 5)
    choice = torch.stack([torch.randperm(T, generator=gen) % G for _ in range(H)])      # [H, T]: every group is some query's choice
    group_of = torch.arange(T) // gs                                       # >= G behind the last whole group: never chosen
    on = group_of.view(1, 1, T) == choice.view(H, T, 1)                    # [H, query, key]
    bias = torch.where(on, 0.0, -256.0).double()
    logits = WATTN_SCALE * torch.einsum("nihd,njhd->nhij", q, kk)
    if float(logits.abs().max()) > 32.0:
        raise ConditionViolated(f"{what}: |scale q k| = {float(logits.abs().max())} > 32")
    Sfull = logits + bias
    top = Sfull.max(-1, keepdim=True).values
    onx = on.view(1, H, T, T).expand_as(Sfull)
    if not (bool((Sfull[onx] == top.expand_as(Sfull)[onx]).all()) and bool((top.expand_as(Sfull)[~onx] - Sfull[~onx] >= 128).all())):
        raise ConditionViolated(f"{what}: the chosen group does not tie at the maximum, or another key is less than 128 below it")
    P = on.double() / gs                                                   # [H, T, T], the same for every window
    o = torch.einsum("hij,njhd->nihd", P, v)
    dv = torch.einsum("hij,nihd->njhd", P, dO)
    check_exact(what, operands=[("q", q, (BF16,)), ("k", kk, (BF16,)), ("v", v, (BF16,)), ("dO", dO, (BF16,)), ("bias", bias, (F32,)),
                                ("P", P, (BF16,))],
                reductions=[("q k", torch.einsum("nihd,njhd->nhij", q.abs(), kk.abs()), 1.0), ("P v", torch.einsum("hij,njhd->nihd", P, v.abs()), 1.0),
                            ("P^T dO", torch.einsum("hij,nihd->njhd", P, dO.abs()), 1.0)],
                results=[("o", o, (BF16,)), ("dv", dv, (BF16,))])
    L = None
    if k == 0:
        L = top.squeeze(-1)                                                # [n, H, T]: the selected logit (its bias is 0)
        check_exact(what, results=[("L", L, (F32,))])
    qkv = torch.cat([t.reshape(n, T, C) for t in (q, kk, v)], -1)
    return NS(what=what, n=n, T=T, H=H, k=k, qkv=f32(qkv), bias=f32(bias), dO=f32(dO.reshape(n, T, C)), o=o.reshape(n, T, C), dv=dv.reshape(n, T, C), L=L,
              q=q, kk=kk, v=v, P=P)
