"""The attention path's kernels at every tier: dfd_bgemm's three kernels, the (R, TEAM) lattice of the softmax rows, and the fused
window attention on an exact gather.  Data, tiers and float64 references: tests/_attn_cases.py; the CPU twin that checks the data's
own conditions and the tiers on any machine: tests/test_attn_tiers_cpu.py.

Every comparison on constructed data is at tolerance 0 (tests/_exact.py, `same`).  The Gaussian softmax cases keep the bounds of
test_attn_softmax_rows_match_autograd (tests/test_vit_ops_gpu.py), relative to the tensor's largest entry: 2e-5 for P and T2, 2e-4 for
dS and dT1, 5e-4 for the talking-head weight gradient formed from dT1.  Every bgemm and softmax case first asserts, through
dfd_bgemm_plan / dfd_attn_softmax_plan, the kernel or launch shape it is listed under: a changed threshold fails here instead of
silently moving the case to another kernel.

Device assumptions of the tolerance-zero softmax and window-attention cases, beyond exact f32 arithmetic on exactly representable
values: __expf(0) == 1, __expf(x) == 0 for x <= -128, 1.0f / 2**k and the hardware reciprocal of 2**k are exact, __logf(1) == 0.
"""

from __future__ import annotations

import ctypes

import pytest
import torch

from tests import _attn_cases as A
from tests._exact import BF16, F32, same

pytestmark = pytest.mark.gpu


def _k():
    from deepfakedetection_amd import kernels

    return kernels


def dev(t, rd=None):
    if t is None:
        return None
    return (t if rd is None else t.to(rd)).cuda()


def bgemm_plan(M, N, K, round_a=False, round_b=False):
    return _k()._L().dfd_bgemm_plan(M, N, K, int(round_a), int(round_b))


def softmax_plan(H, Nk):
    r, team = ctypes.c_int(-1), ctypes.c_int(-1)
    assert _k()._L().dfd_attn_softmax_plan(H, Nk, ctypes.byref(r), ctypes.byref(team)) == 0
    return r.value, team.value


# ----------------------------------------------------------------------------------------------------------------- dfd_bgemm
def run_bgemm(c, da=F32, db=F32, dc=F32):
    K = _k()
    assert bgemm_plan(c.M, c.N, c.K, c.round_a, c.round_b) == c.tier, f"{c.what}: another kernel serves this shape now"
    C = torch.full(c.c_shape, 77.0, dtype=dc, device="cuda")
    K.bgemm(dev(c.A, da), c.sa, dev(c.B, db), c.sb, C, c.sc, c.nb, c.nh, c.M, c.N, c.K, alpha=c.alpha, bias=dev(c.bias),
            round_a=c.round_a, round_b=c.round_b)
    same(C.transpose(-1, -2) if c.c_t else C, c.out, f"{c.what} {da} x {db} -> {dc}")


@pytest.mark.parametrize("name", list(A.BGEMM_CASES))
def test_bgemm_tier_is_exact(name):
    run_bgemm(A.bgemm_case(name))


@pytest.mark.parametrize("name,dts", [(A.BGEMM_ALL_DTYPES, d) for d in A.ALL_DTYPES if d != (F32, F32, F32)]
                         + [(n, d) for n in A.BGEMM_MODEL_DTYPES for d in A.MODEL_DTYPES[1:]],
                         ids=lambda v: v if isinstance(v, str) else "-".join(str(d).split(".")[-1] for d in v))
def test_bgemm_dtype_combinations_are_exact(name, dts):
    run_bgemm(A.bgemm_case(name), *dts)


@pytest.mark.parametrize("case", A.TH_GRAD_CASES)
def test_bgemm_talking_head_gradients_as_the_model_calls_them(case):
    """attn_core_bwd's three calls (deepfakedetection_amd/vit_functions.py): zero head strides with nh = 1, the second operand read
    transposed through its strides, the all-strides-zero ones operand; then the fixed-order row sum over the images."""
    K = _k()
    c = A.th_grad(case)
    H, L, B = case
    assert bgemm_plan(H, H, L) == A.KRED and bgemm_plan(H, 1, L) == A.KRED
    d, p = dev(c.d), dev(c.p)
    rows = B + (B + 31) // 32 + 1
    part = torch.full((rows, H * H), 77.0, device="cuda")
    K.bgemm(d, (H * L, 0, L, 1), p, (H * L, 0, 1, L), part, (H * H, 0, H, 1), B, 1, H, H, L)
    same(part[:B].view(B, H, H), c.parts_w, c.what + ": per-image rows of dW")
    same(K.sum_rows(part.view(-1), B, H * H, torch.empty(H * H, device="cuda")).view(H, H), c.dw, c.what + ": dW")
    ones = torch.ones(8, device="cuda")
    partb = torch.full((rows, H), 77.0, device="cuda")
    K.bgemm(d, (H * L, 0, L, 1), ones, (0, 0, 0, 0), partb, (H, 0, 1, 1), B, 1, H, 1, L)
    same(partb[:B], c.parts_b, c.what + ": per-image rows of db")
    same(K.sum_rows(partb.view(-1), B, H, torch.empty(H, device="cuda")), c.db, c.what + ": db")


@pytest.mark.parametrize("offset", [0, 4], ids=["aligned", "8-byte-base"])
def test_bgemm_bf16_rows_staged_by_16_bytes_or_by_element(offset):
    """q, k, v heads read in place from bf16 [B * T][H * 40] projection outputs.  On a 16-byte aligned allocation every head's base is
    aligned (80 bytes per head) and the rows are staged by 16-byte loads, plain and transposed; 4 elements into an allocation no
    base is, and the same call takes the element path."""
    K = _k()
    c = A.bgemm_heads()
    B, H, T, dk, dv = A.HEADS_CASE
    assert bgemm_plan(T, T, dk) == A.GENERAL and bgemm_plan(T, dv, T) == A.GENERAL

    def place(t):
        flat = torch.zeros(t.numel() + 8, dtype=BF16, device="cuda")
        flat[offset:offset + t.numel()] = t.to(BF16).cuda().view(-1)
        view = flat[offset:offset + t.numel()].view(t.shape)
        assert view.data_ptr() % 16 == 2 * offset
        return view

    q, k, v = place(c.q), place(c.k), place(c.v)
    S = torch.full((B, H, T, T), 77.0, device="cuda")
    K.bgemm(q, (T * H * dk, dk, H * dk, 1), k, (T * H * dk, dk, 1, H * dk), S, (H * T * T, T * T, T, 1), B, H, T, T, dk)
    same(S, c.S, "heads q k^T")
    O = torch.full((B * T, H * dv), 77.0, dtype=BF16, device="cuda")
    K.bgemm(dev(c.w), (H * T * T, T * T, T, 1), v, (T * H * dv, dv, H * dv, 1), O, (T * H * dv, dv, H * dv, 1), B, H, T, dv, T)
    same(O, c.O, "heads w v")


@pytest.mark.parametrize("shape,round_a", A.BGEMM_REFUSED)
def test_bgemm_refuses_panels_beyond_150_kib(shape, round_a):
    K = _k()
    M, N, Kd = shape
    assert bgemm_plan(M, N, Kd, round_a) == A.UNSUPPORTED
    a, b, c = torch.zeros((2, M, Kd), device="cuda"), torch.zeros((2, Kd, N), device="cuda"), torch.zeros((2, M, N), device="cuda")
    with pytest.raises(RuntimeError, match="DFD_EUNSUPPORTED"):
        K.bgemm(a, (M * Kd, 0, Kd, 1), b, (Kd * N, 0, N, 1), c, (M * N, 0, N, 1), 2, 1, M, N, Kd, round_a=round_a)


# ------------------------------------------------------------------------------------------------------------- softmax rows
def close(got, want, rel, what):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    scale = max(float(want.abs().max()), 1e-6)
    err = float((got - want).abs().max()) / scale
    print(f"{what}: max err {err:.3e} of max |ref| {scale:.3e} (bound {rel:.1e})")
    assert err <= rel, f"{what}: max err {err:.3e} of max |ref| {scale:.3e} > {rel:.1e}"


def run_softmax(c, what, backward=True):
    K = _k()
    th = None if c.th is None else tuple(dev(t) for t in c.th)
    P, T2 = K.attn_softmax_fwd(dev(c.S), th)
    close(P, c.ref.P, A.SOFTMAX_TOL.P, what + " P")
    close(T2, c.ref.T2, A.SOFTMAX_TOL.T2, what + " T2")
    if not backward:
        return
    dT1, dS = K.attn_softmax_bwd(dev(c.g), P, th)
    close(dS, c.ref.dS, A.SOFTMAX_TOL.dS, what + " dS")
    if th is not None:
        close(dT1, c.ref.dT1, A.SOFTMAX_TOL.dS, what + " dT1")
        close(torch.einsum("bgij,bhij->gh", dT1.double().cpu(), c.S.double()), c.ref.dW1, A.SOFTMAX_TOL.dW1, what + " dW1 from dT1")
    else:
        assert dT1 is None


@pytest.mark.parametrize("talk", [True, False])
@pytest.mark.parametrize("H,Nk,R,team", A.SOFTMAX_LATTICE)
def test_attn_softmax_rows_on_the_launch_lattice(H, Nk, R, team, talk):
    """Every TEAM from 1 to 32, R clamped to 64 and lowered by H, H no power of two, Nk = 1 and 256, and a last workgroup that is not
    full; the (R, TEAM) literals are what the rule of csrc/dfd_vit.hip gives for (H, Nk)."""
    assert softmax_plan(H, Nk) == (R, team), "the launch shape of this lattice point moved"
    run_softmax(A.softmax_case(H, Nk, talk), f"softmax rows ({H}, {Nk}) R {R} TEAM {team} talk {talk}")


@pytest.mark.parametrize("talk", [True, False])
def test_attn_softmax_rows_with_logits_near_80(talk):
    """exp(80) overflows nothing in f32 but exp(89) does: without the subtraction of the row maximum these rows are inf / inf."""
    H, Nk = A.SOFTMAX_BIG_LOGITS
    run_softmax(A.softmax_case(H, Nk, talk, 20.0), f"softmax rows ({H}, {Nk}) |S| ~ 80 talk {talk}", backward=False)


@pytest.mark.parametrize("talk", [True, False])
@pytest.mark.parametrize("H,Nk", A.SOFTMAX_EXACT)
def test_attn_softmax_rows_are_exact_on_marked_keys(H, Nk, talk):
    """Tolerance 0: P is 2**-k on the 2**k marked keys of a row and 0 elsewhere (tests/_attn_cases.py), T2, dT1 and dS short dyadic
    numbers.  A key left out of a TEAM member's walk, a partial sum combined twice or a row of the ragged last workgroup
    skipped changes a power of two, not a last bit.  Device assumptions: __expf(0) == 1, __expf(x) == 0 for x <= -256 and
    1.0f / 2**k exact."""
    K = _k()
    c = A.softmax_exact(H, Nk, talk)
    assert softmax_plan(H, Nk) == (c.R, c.team)
    th = None if c.th is None else tuple(dev(t) for t in c.th)
    P, T2 = K.attn_softmax_fwd(dev(c.S), th)
    same(P, c.P, c.what + " P")
    same(T2, c.T2, c.what + " T2")
    th_b = None if c.th_bwd is None else tuple(dev(t) for t in c.th_bwd)
    dT1, dS = K.attn_softmax_bwd(dev(c.dT2), dev(c.P.float()), th_b)
    if talk:
        same(dT1, c.dT1, c.what + " dT1")
    same(dS, c.dS, c.what + " dS")


# ------------------------------------------------------------------------------------------------ fused window attention
@pytest.mark.parametrize("k", A.WATTN_LOG2_GROUP)
@pytest.mark.parametrize("case", A.WATTN_EXACT)
def test_fused_window_attention_gathers_exactly(case, k):
    """Keys in groups of 2**k with identical k rows, a bias of 0 on the query's group and -256 elsewhere: P is exactly 2**-k on the group
    after the bf16 pack, o the exact mean of the group's v rows, dv the exact scatter-add of the dO rows (times 2**-k).  One-hot
    (k = 0): L is the selected logit and dq, dk, dbias are exactly zero - for live windows, padded tokens and the idle waves of the
    ragged last group of windows (n % 4 != 0 in every case).  With k > 0 the backward recomputes P through __expf(x - L) with an
    inexact log 2**k, which the bf16 pack rounds back to 2**-k for dv; dq, dk and dbias stay with the tolerance test of
    tests/test_vit_ops_gpu.py.  Device assumptions: __expf(0) == 1, __expf(x) == 0 for x <= -128, the reciprocal of 2**k exact,
    __logf(1) == 0."""
    K = _k()
    c = A.wattn_exact(case, k)
    n, T, H = case
    C = H * A.WATTN_HD
    assert K.wattn_supported(BF16, T, A.WATTN_HD) and n % 4 != 0
    qd, bd = dev(c.qkv, BF16).view(n, T, 1, 3 * C), dev(c.bias)
    o, L = K.wattn_fwd(qd, bd, H, A.WATTN_SCALE)
    same(o.view(n, T, C), c.o, c.what + " o")
    o2, L2 = K.wattn_fwd(qd, bd, H, A.WATTN_SCALE, want_lse=False)
    assert L2 is None and torch.equal(o, o2)
    if k == 0:
        same(L, c.L, c.what + " L")
    dqkv, dbias = K.wattn_bwd(qd, dev(c.dO, BF16).view(n, T, 1, C), L, bd, H, A.WATTN_SCALE, True)
    dqkv = dqkv.view(n, T, 3 * C)
    same(dqkv[..., 2 * C:], c.dv, c.what + " dv")
    if k == 0:
        zero = torch.zeros(n, T, C, dtype=torch.float64)
        same(dqkv[..., :C], zero, c.what + " dq")
        same(dqkv[..., C:2 * C], zero, c.what + " dk")
        same(dbias, torch.zeros(H, T, T, dtype=torch.float64), c.what + " dbias")
