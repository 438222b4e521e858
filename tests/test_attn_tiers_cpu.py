"""The CPU twin of tests/test_attn_tiers_gpu.py: needs no GPU.

Runs every builder of tests/_attn_cases.py (so the exactness conditions are checked here), evaluates plain f32 torch on the same data
against the float64 results at tolerance 0, and asserts through the planner exports dfd_bgemm_plan / dfd_attn_softmax_plan (host code
of libdfd_hip.so) that every case lands on the tier it is listed under.
"""

from __future__ import annotations

import ctypes

import pytest
import torch
import torch.nn.functional as F

from deepfakedetection_amd import _lib
from oracle import ops_ref as R
from tests import _attn_cases as A
from tests._exact import BF16, same


def bgemm_plan(M, N, K, round_a=False, round_b=False):
    return _lib.load().dfd_bgemm_plan(M, N, K, int(round_a), int(round_b))


def softmax_plan(H, Nk):
    r, team = ctypes.c_int(-1), ctypes.c_int(-1)
    code = _lib.load().dfd_attn_softmax_plan(H, Nk, ctypes.byref(r), ctypes.byref(team))
    return code, r.value, team.value


# ----------------------------------------------------------------------------------------------------------------- planners
def test_abi_148_exports():
    lib = _lib.load()
    assert lib.dfd_version() >= 148
    assert lib.dfd_bgemm_plan(0, 1, 1, 0, 0) == -1 and lib.dfd_bgemm_plan(1, 1, 0, 0, 0) == -1
    assert lib.dfd_attn_softmax_plan(17, 16, None, None) == -1 and lib.dfd_attn_softmax_plan(1, 257, None, None) == -1
    assert lib.dfd_attn_softmax_plan(0, 16, None, None) == -1 and lib.dfd_attn_softmax_plan(4, 0, None, None) == -1
    assert lib.dfd_attn_softmax_plan(16, 256, None, None) == 0            # null outputs are allowed


@pytest.mark.parametrize("name", list(A.BGEMM_CASES))
def test_bgemm_case_lands_on_its_tier(name):
    tier, (M, N, K), _, opt = A.BGEMM_CASES[name]
    assert bgemm_plan(M, N, K, opt.get("round") == "a", opt.get("round") == "b") == tier


def test_bgemm_tier_boundaries():
    """Both sides of every threshold, and the refusals."""
    assert bgemm_plan(8, 8, 512) == A.KRED and bgemm_plan(8, 8, 511) == A.GENERAL
    assert bgemm_plan(9, 8, 1000) == A.SMALL and bgemm_plan(8, 9, 1000) == A.SMALL
    assert A.bgemm_lds(16, 16, 384) == 48 * 1024 and bgemm_plan(16, 16, 384) == A.GENERAL and bgemm_plan(16, 16, 385) == A.SMALL
    assert bgemm_plan(16, 1, 614) == A.GENERAL and bgemm_plan(16, 1, 615) == A.SMALL
    assert bgemm_plan(17, 16, 385) == A.GENERAL and bgemm_plan(16, 17, 385) == A.GENERAL
    assert A.bgemm_lds(64, 64, 300) == 150 * 1024 and bgemm_plan(64, 64, 300) == A.GENERAL
    for (M, N, K), round_a in A.BGEMM_REFUSED:
        assert A.bgemm_lds(M, N, K) > 150 * 1024
        assert bgemm_plan(M, N, K, round_a) == A.UNSUPPORTED
    assert bgemm_plan(8, 8, 2401) == A.KRED and bgemm_plan(8, 8, 2401, False, True) == A.UNSUPPORTED
    assert bgemm_plan(8, 8, 2400, True) == A.GENERAL                       # the rounding flags exclude kred and small: 150 KiB exactly
    for H, L, _ in A.TH_GRAD_CASES:
        assert bgemm_plan(H, H, L) == A.KRED and bgemm_plan(H, 1, L) == A.KRED


@pytest.mark.parametrize("H,Nk,R,team", A.SOFTMAX_LATTICE)
def test_softmax_lattice_point_has_its_launch_shape(H, Nk, R, team):
    assert softmax_plan(H, Nk) == (0, R, team)
    assert A.plan_rule(H, Nk) == (R, team)
    B, Nq = A.softmax_rows(R)
    assert B * Nq >= 2 * R + 1 and (R == 1 or (B * Nq) % R != 0)


def test_softmax_plan_is_the_restated_rule_everywhere():
    """H = 1 .. 16, Nk = 1 .. 256: the export and the rule of tests/_attn_cases.py agree, and the lattice holds every TEAM there is."""
    teams = set()
    for H in range(1, 17):
        for Nk in range(1, 257):
            code, r, team = softmax_plan(H, Nk)
            assert (code, r, team) == (0,) + A.plan_rule(H, Nk), (H, Nk)
            assert 1 <= r <= 64 and r * Nk <= 256 and H * r <= 256
            teams.add(team)
    assert teams == {t for _, _, _, t in A.SOFTMAX_LATTICE} == {1, 2, 4, 8, 16, 32}
    assert {A.plan_rule(H, Nk)[1] for H, Nk in A.SOFTMAX_EXACT} == {1, 8, 32}


# ------------------------------------------------------------------------------------------------------------------ products
@pytest.mark.parametrize("name", list(A.BGEMM_CASES))
def test_bgemm_cases_in_f32(name):
    c = A.bgemm_case(name)
    a = c.A.transpose(-1, -2) if c.sa[2] == 1 and c.sa[3] != 1 else c.A            # back to [nb, nh, M, K]
    b = c.B.transpose(-1, -2) if c.sb[2] == 1 and c.sb[3] != 1 else c.B
    a, b = a.reshape(c.nb, c.nh, c.M, c.K), b.reshape(c.nb, c.nh, c.K, c.N)
    if c.round_a:
        a = R.rnd(a, BF16)
    if c.round_b:
        b = R.rnd(b, BF16)
    same(a, c.a64, c.what + ": A as the kernel sees it")
    same(b, c.b64, c.what + ": B as the kernel sees it")
    out = c.alpha * (a @ b)
    if c.bias is not None:
        out = out + c.bias
    same(out, c.out, c.what)
    same(R.rnd(out, BF16), c.out, c.what + " stored as bf16")


@pytest.mark.parametrize("case", A.TH_GRAD_CASES)
def test_talking_head_gradients_in_f32(case):
    c = A.th_grad(case)
    parts = c.d @ c.p.transpose(-1, -2)
    same(parts, c.parts_w, c.what + " rows")
    same(parts.sum(0), c.dw, c.what + " dW")
    same(c.d.sum(-1), c.parts_b, c.what + " bias rows")
    same(c.d.sum((0, 2)), c.db, c.what + " db")


def test_bgemm_heads_in_f32():
    c = A.bgemm_heads()
    B, H, T, dk, dv = A.HEADS_CASE
    heads = lambda t, d: t.view(B, T, H, d).permute(0, 2, 1, 3)
    same(heads(c.q, dk) @ heads(c.k, dk).transpose(-1, -2), c.S, "heads q k^T")
    same((c.w @ heads(c.v, dv)).permute(0, 2, 1, 3).reshape(B * T, H * dv), c.O, "heads w v")


# ------------------------------------------------------------------------------------------------------------------- softmax
def softmax_f32(S, th):
    H = S.shape[1]
    if th is None:
        P = S.softmax(-1)
        return P, P
    w1, b1, w2, b2 = th
    P = F.conv2d(S, w1.view(H, H, 1, 1), b1).softmax(-1)
    return P, F.conv2d(P, w2.view(H, H, 1, 1), b2)


@pytest.mark.parametrize("talk", [True, False])
@pytest.mark.parametrize("H,Nk", A.SOFTMAX_EXACT)
def test_exact_softmax_in_f32(H, Nk, talk):
    c = A.softmax_exact(H, Nk, talk)
    assert (c.R, c.team) == softmax_plan(H, Nk)[1:]
    P, T2 = softmax_f32(c.S, c.th)
    same(P, c.P, c.what + " P")
    same(T2, c.T2, c.what + " T2")
    # the backward formula in f32 on the exact P
    P32, d2 = c.P.float(), c.dT2
    if talk:
        w1, _, w2, _ = c.th_bwd
        dP = torch.einsum("gh,bgij->bhij", w2, d2)
    else:
        dP = d2
    dT1 = P32 * (dP - (dP * P32).sum(-1, keepdim=True))
    same(dT1, c.dT1, c.what + " dT1")
    same(torch.einsum("gh,bgij->bhij", w1, dT1) if talk else dT1, c.dS, c.what + " dS")
    # every row has marked keys, and all of 1, 2, 4, 8 occur as far as Nk allows
    counts = set((c.P[:, 0] > 0).sum(-1).flatten().tolist())
    assert counts == {n for n in (1, 2, 4, 8) if n <= Nk}


@pytest.mark.parametrize("talk", [True, False])
@pytest.mark.parametrize("H,Nk,R,team", A.SOFTMAX_LATTICE)
def test_softmax_lattice_data_in_f32(H, Nk, R, team, talk):
    """The f32 oracle stays inside the bounds the kernels are held to (relative to the largest entry)."""
    c = A.softmax_case(H, Nk, talk)
    assert (c.R, c.team) == (R, team)
    P, T2 = softmax_f32(c.S, c.th)
    for got, want, tol in ((P, c.ref.P, A.SOFTMAX_TOL.P), (T2, c.ref.T2, A.SOFTMAX_TOL.T2)):
        assert float((got.double() - want).abs().max()) <= tol * float(want.abs().max())


@pytest.mark.parametrize("talk", [True, False])
def test_softmax_big_logits_data_in_f32(talk):
    H, Nk = A.SOFTMAX_BIG_LOGITS
    c = A.softmax_case(H, Nk, talk, 20.0)
    assert 60.0 <= float(c.S.abs().max()) <= 120.0
    P, T2 = softmax_f32(c.S, c.th)
    for got, want, tol in ((P, c.ref.P, A.SOFTMAX_TOL.P), (T2, c.ref.T2, A.SOFTMAX_TOL.T2)):
        assert float((got.double() - want).abs().max()) <= tol * float(want.abs().max())


# --------------------------------------------------------------------------------------------------- fused window attention
@pytest.mark.parametrize("k", A.WATTN_LOG2_GROUP)
@pytest.mark.parametrize("case", A.WATTN_EXACT)
def test_exact_window_attention_in_f32(case, k):
    c = A.wattn_exact(case, k)
    n, T, H = case
    C = H * A.WATTN_HD
    q, kk, v = [t.view(n, T, H, A.WATTN_HD).permute(0, 2, 1, 3) for t in c.qkv.split(C, dim=-1)]
    S = q @ kk.transpose(-1, -2) * A.WATTN_SCALE + c.bias
    P = R.rnd(S.softmax(-1), BF16)
    same(P, c.P.expand(n, H, T, T), c.what + " P")
    same(R.rnd((P @ v).permute(0, 2, 1, 3).reshape(n, T, C), BF16), c.o, c.what + " o")
    dO = c.dO.view(n, T, H, A.WATTN_HD).permute(0, 2, 1, 3)
    same(R.rnd((P.transpose(-1, -2) @ dO).permute(0, 2, 1, 3).reshape(n, T, C), BF16), c.dv, c.what + " dv")
    if k == 0:
        same(torch.logsumexp(S, -1), c.L, c.what + " L")
    assert n % 4 != 0                      # a ragged last group of windows: idle waves in the bias-gradient sum
    # every group is chosen by some query of some head, so no key's dv is trivially zero everywhere
    assert bool((c.P.sum((0, 1))[: (T >> k) << k] > 0).all())
