"""The classifier head, the loss, softmax / arg-max, dropout and the AdamW step (csrc/dfd_misc.hip) at the shapes and on the data
where they can go wrong.

tests/test_ops_gpu.py (test_head_loss, test_adamw_matches_torch) holds these kernels at (N, K, J) = (6, 1280, {2, 10, 1000}) on
N(0, 1) logits and on four 16-byte-aligned tensors.  At those sizes the eight-row loop of the weight gradient, the second trip of the
bias-gradient and row-mean loops, every `k < K` / `i < n` guard and the scalar path of the AdamW kernel never run.  Here:

  * linear forward / backward at the shipped head widths that are no multiple of 64 (176, 224, 288, 1536), at N below, at and
    above one 8-row trip and above 256, at both sides of the K <= 16 switch, with every set of gradient flags and with
    caller-owned destinations;
  * both cross entropies on saturated logits, logits with a large common offset, rows of equal logits, J in {1, 2, 3, 257, 1000},
    label smoothing 0 and 0.1, three gradient scales, targets placed at class 0 and class J - 1, and a -inf logit off the target;
  * softmax / arg-max on the same regimes, exact ties across lanes, trips and waves, and rows that hold NaN or infinities;
  * dropout as a bit-exact f32 restatement with `u` planted at the threshold and just below it;
  * AdamW over chunks of 1 .. 65536 elements at aligned and misaligned addresses, with a gradient scale and canaries.

Every reference is float64 from the f32 inputs (torch on the CPU; oracle/ops_ref.py where it has the operation).  The tolerances are
test_head_loss's and test_adamw_matches_torch's under the same close(): 1e-4 linear forward, 2e-4 dx / dw / db / dlogits, 1e-5 loss,
probabilities and AdamW.  Every comparison prints its measured error first (pytest -s shows them).
"""

from __future__ import annotations

import functools
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from oracle import ops_ref as R
from tests.test_ops_gpu import close, dev

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")


def _k():
    from deepfakedetection_amd import kernels

    return kernels


def measured(got: torch.Tensor, want: torch.Tensor, rel: float, what: str) -> None:
    """close() of tests/test_ops_gpu.py, with the figure it compares printed first."""
    g, w = got.detach().float().cpu(), want.detach().float().cpu()
    if g.shape == w.shape and g.numel():
        err = float((g - w).abs().max()) / max(float(w.abs().max()), 1e-6)
        print(f"[head] {what}: err {err:.3e} (bound {rel:.0e})")
    close(got, want, rel, what)


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, f"{what}: shape {tuple(g.shape)} vs {tuple(w.shape)}"
    bad = g != w
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {g.numel()} elements differ in their bits, first at {tuple(int(i) for i in bad.nonzero()[0])}"


# ------------------------------------------------------------------------------------------------------------------ linear
# (72, 176, 2): the EfficientFormerV2-S0 head: K % 64 = 48, nine trips of the 8-row loop, a second trip of the db loop
# (13, 224, 3): one 8-row trip and a remainder of 5, a wave holding 3 of its 4 outputs
# (8, 288, 17): a second blockIdx.y holding one output; in k_linear_bwd_x the unrolled j + 12 < J trip and a one-element tail
# (300, 1536, 2): the EfficientNet-B3 head above 256 rows
# (5, 17, 5) / (5, 16, 5): the two sides of the K <= 16 switch to k_linear_fwd_smallk
# (9, 1280, 1): a single output
LINEAR_SHAPES = [(72, 176, 2), (13, 224, 3), (8, 288, 17), (300, 1536, 2), (5, 17, 5), (5, 16, 5), (9, 1280, 1)]


@functools.lru_cache(maxsize=None)
def linear_case(case):
    N, Kd, J = case
    g = torch.Generator().manual_seed(7100 + 31 * N + 7 * Kd + J)
    x = torch.randn((N, Kd), generator=g)
    w = torch.randn((J, Kd), generator=g) * Kd ** -0.5
    b = torch.randn(J, generator=g) * 0.1
    dout = torch.randn((N, J), generator=g)
    x64, w64, b64, d64 = x.double(), w.double(), b.double(), dout.double()
    return NS(x=x, w=w, b=b, dout=dout, out_nb=x64 @ w64.t(), out=x64 @ w64.t() + b64, dx=d64 @ w64, dw=d64.t() @ x64, db=d64.sum(0))


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("case", LINEAR_SHAPES)
def test_linear_fwd(case, bias):
    K = _k()
    c = linear_case(case)
    got = K.linear_fwd(dev(c.x), dev(c.w), dev(c.b) if bias else None)
    measured(got, c.out if bias else c.out_nb, 1e-4, f"linear fwd {case} bias={bias}")


@pytest.mark.parametrize("case", LINEAR_SHAPES)
def test_linear_bwd(case):
    K = _k()
    N, Kd, J = case
    c = linear_case(case)
    x, w, dout = dev(c.x), dev(c.w), dev(c.dout)
    dx, dw, db = K.linear_bwd(dout, x, w, True, True, True)
    measured(dx, c.dx, 2e-4, f"linear dx {case}")
    measured(dw, c.dw, 2e-4, f"linear dw {case}")
    measured(db, c.db, 2e-4, f"linear db {case}")
    dx1, dw1, db1 = K.linear_bwd(dout, x, w, True, False, True)
    assert dw1 is None and db1 is None, "a gradient that was not asked for"
    measured(dx1, c.dx, 2e-4, f"linear dx alone {case}")
    dx2, dw2, db2 = K.linear_bwd(dout, x, w, False, True, True)
    assert dx2 is None, "a gradient that was not asked for"
    measured(dw2, c.dw, 2e-4, f"linear dw without dx {case}")
    measured(db2, c.db, 2e-4, f"linear db without dx {case}")
    dx3, dw3, db3 = K.linear_bwd(dout, x, w, False, True, False)
    assert dx3 is None and db3 is None, "a gradient that was not asked for"
    measured(dw3, c.dw, 2e-4, f"linear dw alone {case}")
    # caller-owned destinations (gradient-arena slots): they are what comes back, every element is overwritten, same bits
    out_dw = torch.full((J, Kd), NAN, device="cuda")
    out_db = torch.full((J,), NAN, device="cuda")
    dx4, dw4, db4 = K.linear_bwd(dout, x, w, True, True, True, out_dw=out_dw, out_db=out_db)
    assert dw4 is out_dw and db4 is out_db
    same_bits(dx4, dx, f"linear dx beside destinations {case}")
    same_bits(out_dw, dw, f"linear dw in its destination {case}")
    same_bits(out_db, db, f"linear db in its destination {case}")


# ------------------------------------------------------------------------------------------------------------------ logits
REGIMES = ("normal", "saturated", "offset", "equal")
CE_SHAPES = [(1, 2), (7, 3), (257, 2), (300, 257), (6, 1000), (4, 1)]
EPS = (0.0, 0.1)
GRAD_SCALES = (1.0, 0.25, 128.0)


def make_logits(N: int, J: int, regime: str, seed: int) -> torch.Tensor:
    """f32 [N, J].  normal: N(0, 1); saturated: N(0, 1) * 30, the target is often far below the maximum; offset: N(0, 1) + 10000,
    rounded to f32 (a grid of 2**-10 there) before anything else sees it; equal: every row one value."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn((N, J), generator=g)
    if regime == "normal":
        return a
    if regime == "saturated":
        return a * 30
    if regime == "offset":
        return a + 10000
    assert regime == "equal"
    return (a[:, :1] * 3).expand(N, J).contiguous()


def ce_logits(shape, regime) -> torch.Tensor:
    """The logits of one cross-entropy case.

    A single saturated row needs a condition on the draw.  The loss of a row whose target is its maximum, `gap` above the next
    logit, is log(1 + exp(-gap)), and an f32 loss reaches it through se = 1 + exp(-gap) >= 1, which f32 holds to 2**-24 = 6e-8
    and no better (torch's own f32 cross entropy has the same floor).  Among other rows that is noise under the mean.  At N = 1
    it is the whole result: for 5 < gap < 26 the loss lies between 1e-11 and 7e-3 and 6e-8 is more than 1e-5 of it (or of
    close()'s floor of 1e-6), whatever the kernel does.  (1, 2) "saturated" therefore takes the first seed whose gap lies outside
    that window (42.7: the loss is 3e-19 with the target at the maximum and 42.7 with it at the other class); N(0, 1) logits
    do not reach a gap of 5."""
    N, J = shape
    lg = make_logits(N, J, regime, 7200 + 1009 * REGIMES.index(regime) + 13 * N + J + (5 if (shape, regime) == ((1, 2), "saturated") else 0))
    if N == 1 and J > 1:
        top = lg.double().topk(2, 1).values
        assert not 5 < float(top[0, 0] - top[0, 1]) < 26, "a single row whose loss f32 cannot hold to 1e-5"
    return lg


def hard_targets(N: int, J: int):
    """Target vectors that together hold class 0 and class J - 1 (one vector; two at N = 1)."""
    if N == 1:
        return [torch.zeros(1, dtype=torch.int64), torch.full((1,), J - 1, dtype=torch.int64)]
    tg = torch.randint(0, J, (N,), generator=torch.Generator().manual_seed(7300 + N + J))
    tg[0], tg[-1] = 0, J - 1
    return [tg]


def _ce_hard(K, lg: torch.Tensor, tg: torch.Tensor, eps: float, what: str):
    """One (logits, targets, eps): the loss and dlogits at every gradient scale, and the loss alone.  Returns what the kernel
    gave at the last scale."""
    N, J = lg.shape
    l64 = lg.double().requires_grad_(True)
    want = R.ce_label_smooth(l64, tg, eps)
    (dwant,) = torch.autograd.grad(want, l64)
    lgd, tgd = dev(lg), dev(tg)
    alone, none = K.ce_loss(lgd, tgd, eps, 1.0, False)
    assert none is None
    for gs in GRAD_SCALES:
        loss, dl = K.ce_loss(lgd, tgd, eps, gs, True)
        measured(loss.reshape(1), want.detach().reshape(1), 1e-5, f"{what} eps={eps} gs={gs}: loss")
        measured(dl, dwant * gs, 2e-4, f"{what} eps={eps} gs={gs}: dlogits")
        same_bits(alone.reshape(1), loss.reshape(1), f"{what} eps={eps} gs={gs}: loss without and with the gradient")
        if J == 1:
            assert float(loss) == 0.0 and int(torch.count_nonzero(dl)) == 0, f"{what}: one class has loss 0 and no gradient"
    return want.detach(), dwant, loss, dl


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("shape", CE_SHAPES)
def test_ce_hard_targets(shape, regime):
    K = _k()
    N, J = shape
    lg = ce_logits(shape, regime)
    targets = hard_targets(N, J)
    seen = torch.cat(targets)
    assert bool((seen == 0).any()) and bool((seen == J - 1).any())
    for ti, tg in enumerate(targets):
        for eps in EPS:
            _ce_hard(K, lg, tg, eps, f"ce {shape} {regime} targets {ti}")


@pytest.mark.parametrize("shape", [s for s in CE_SHAPES if s[1] > 1])
def test_ce_minus_infinity_off_the_target_without_smoothing(shape):
    """label_smoothing = 0 and one -inf logit per row at a class that is not the target: torch's loss is finite (the class has
    probability 0 and no weight in the loss) and its gradient there is 0.

    Before ABI 145 k_ce_rows formed eps * smooth = 0 * inf: measured on that library, the loss was NaN at every shape here
    (reference 0.7504 at (7, 3), 6.176 at (300, 257), 7.645 at (6, 1000), and 0 at J = 2, where the row has one finite logit)."""
    K = _k()
    N, J = shape
    lg = ce_logits(shape, "normal").clone()
    for ti, tg in enumerate(hard_targets(N, J)):
        hole = (tg + 1 + torch.arange(N) % (J - 1)) % J          # 1 .. J - 1 classes behind the target: never the target
        assert not bool((hole == tg).any())
        lh = lg.clone()
        lh[torch.arange(N), hole] = -INF
        want, dwant, loss, dl = _ce_hard(K, lh, tg, 0.0, f"ce {shape} -inf targets {ti}")
        assert bool(torch.isfinite(want)) and bool(torch.isfinite(dwant).all()), "the reference itself"
        assert bool(torch.isfinite(loss).item()), f"loss {float(loss)!r}, reference {float(want)!r}"
        at = dl.cpu()[torch.arange(N), hole]
        assert int(torch.count_nonzero(at)) == 0 and int(torch.count_nonzero(dwant[torch.arange(N), hole])) == 0


def soft_targets(N: int, J: int, shift: int) -> torch.Tensor:
    """f32 [N, J] >= 0 whose rows sum to 1, 0.5 and 0 in turn (mix.BatchMixer's rows sum to 1; the kernel does not need that)."""
    g = torch.Generator().manual_seed(7400 + N + J)
    t = torch.softmax(torch.randn((N, J), generator=g) * 2, 1)
    scale = torch.tensor([1.0, 0.5, 0.0])[(torch.arange(N) + shift) % 3]
    return (t * scale[:, None]).contiguous()


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("shape", CE_SHAPES)
def test_ce_soft_targets(shape, regime):
    K = _k()
    N, J = shape
    lg = ce_logits(shape, regime)
    lgd = dev(lg)
    for shift in range(3 if N < 3 else 1):                      # fewer than three rows: one run per row sum
        t = soft_targets(N, J, shift)
        sums = t.sum(1)
        if N >= 3:
            assert bool((sums == 0).any()) and bool(((sums - 0.5).abs() < 1e-5).any()) and bool(((sums - 1).abs() < 1e-5).any())
        td = dev(t)
        for eps in EPS:
            l64 = lg.double().requires_grad_(True)
            q = t.double() * (1 - eps) + eps / J
            want = -(q * torch.log_softmax(l64, 1)).sum(1).mean()
            (dwant,) = torch.autograd.grad(want, l64)
            alone, none = K.ce_loss_soft(lgd, td, eps, 1.0, False)
            assert none is None
            for gs in GRAD_SCALES:
                what = f"soft ce {shape} {regime} sums {shift} eps={eps} gs={gs}"
                loss, dl = K.ce_loss_soft(lgd, td, eps, gs, True)
                measured(loss.reshape(1), want.detach().reshape(1), 1e-5, f"{what}: loss")
                measured(dl, dwant * gs, 2e-4, f"{what}: dlogits")
                same_bits(alone.reshape(1), loss.reshape(1), f"{what}: loss without and with the gradient")


# ------------------------------------------------------------------------------------------------------------------ softmax / arg-max
SOFTMAX_SHAPES = [(1, 1), (300, 2), (7, 3), (5, 257), (6, 1000)]
MARGIN = 1e-3
# The arg-max is compared on rows whose two largest reference probabilities lie more than MARGIN apart; at most 2 % of the rows may
# fall out.  With J = 257 or 1000 most draws have a closer pair somewhere in their five or six rows: these seeds do not (searched on
# the CPU, on the reference alone: the first seed >= 7500 that satisfies the rule; the test asserts the rule again).
SOFTMAX_SEEDS = {
    ((1, 1), "normal"): 7500, ((1, 1), "saturated"): 7500, ((1, 1), "offset"): 7500,
    ((300, 2), "normal"): 7500, ((300, 2), "saturated"): 7500, ((300, 2), "offset"): 7500,
    ((7, 3), "normal"): 7500, ((7, 3), "saturated"): 7500, ((7, 3), "offset"): 7500,
    ((5, 257), "normal"): 7500, ((5, 257), "saturated"): 7500, ((5, 257), "offset"): 7500,
    ((6, 1000), "normal"): 7503, ((6, 1000), "saturated"): 7500, ((6, 1000), "offset"): 7503,
}


def decided_rows(want: torch.Tensor) -> torch.Tensor:
    if want.shape[1] == 1:
        return torch.ones(want.shape[0], dtype=torch.bool)
    top = want.topk(2, 1).values
    return top[:, 0] - top[:, 1] > MARGIN


@pytest.mark.parametrize("regime", REGIMES[:3])
@pytest.mark.parametrize("shape", SOFTMAX_SHAPES)
def test_softmax_argmax(shape, regime):
    K = _k()
    N, J = shape
    lg = make_logits(N, J, regime, SOFTMAX_SEEDS[shape, regime])
    want = torch.softmax(lg.double(), 1)
    decided = decided_rows(want)
    assert int((~decided).sum()) <= 0.02 * N, f"{int((~decided).sum())} of {N} rows have their two largest probabilities within {MARGIN}"
    lgd = dev(lg)
    probs, preds = K.softmax_argmax(lgd, True)
    none, preds_alone = K.softmax_argmax(lgd, False)
    assert none is None
    assert torch.equal(preds, preds_alone), "arg-max with and without the probabilities"
    measured(probs, want, 1e-5, f"softmax {shape} {regime}")
    preds = preds.cpu()
    assert bool(((preds >= 0) & (preds < J)).all())
    assert torch.equal(preds[decided], want.argmax(1)[decided]), f"arg-max {shape} {regime}"


# the two places of the row's maximum (bit-equal logits): the lowest index wins.  Thread t of 256 holds the columns t, t + 256, ...
#   (0, 1) at J = 2      neighbouring lanes of one wave
#   (3, 700)             wave 0 against wave 2's third trip
#   (69, 261)            thread 5's second trip (wave 0) against thread 69's first (wave 1)
#   (255, 256)           the last lane of wave 3 against thread 0's second trip
#   (40, 266)            inside wave 0: thread 10's second trip against thread 40's first, the lower index in the higher lane
TIES = [(2, (0, 1)), (1000, (3, 700)), (1000, (69, 261)), (1000, (255, 256)), (1000, (40, 266))]


@pytest.mark.parametrize("J,where", TIES)
def test_argmax_ties_go_to_the_lowest_index(J, where):
    K = _k()
    N = 5
    lg = make_logits(N, J, "normal", 7600 + J + where[1])
    top = lg.max(1).values + torch.arange(1, N + 1) * 0.25          # another margin above the rest in every row
    for j in where:
        lg[:, j] = top
    assert torch.equal(lg.double().argmax(1), torch.full((N,), where[0])) and bool((lg[:, where[0]] == lg[:, where[1]]).all())
    probs, preds = K.softmax_argmax(dev(lg), True)
    none, preds_alone = K.softmax_argmax(dev(lg), False)
    same_bits(probs[:, where[0]], probs[:, where[1]], "the probabilities of bit-equal logits")
    assert preds.cpu().tolist() == [where[0]] * N and preds_alone.cpu().tolist() == [where[0]] * N, (preds.cpu().tolist(), where)


@pytest.mark.parametrize("J", [2, 257, 1000])
def test_argmax_of_non_finite_rows(J):
    """Rows that hold a NaN or an infinity have no probabilities (all NaN, as torch's softmax gives), and their arg-max is what
    torch.argmax(torch.softmax(row)) gives on the CPU - 0, the index the CPU branch of orchestrator.class_probabilities returns -
    so that it stays an index into the row.  Only softmax_argmax runs here and the result is read on the host.

    Before ABI 145 the arg-max started from the index 0x7fffffff, which no NaN probability replaces: measured on that library,
    preds = 2147483647 for each of the four non-finite rows at every J here (their probabilities all NaN, the arg-max of the two
    finite rows as torch's)."""
    K = _k()
    fin = make_logits(2, J, "normal", 7700 + J)
    one_nan, all_nan, all_ninf, one_pinf = fin[0].clone(), torch.full((J,), NAN), torch.full((J,), -INF), fin[1].clone()
    one_nan[J // 2] = NAN                                           # J = 1000: thread 244's second trip
    one_pinf[J - 1] = INF
    lg = torch.stack([fin[0], one_nan, all_nan, all_ninf, one_pinf, fin[1]])
    bad = [1, 2, 3, 4]
    want_preds = torch.argmax(torch.softmax(lg, 1), 1)
    assert want_preds[bad].tolist() == [0, 0, 0, 0]
    probs, preds = K.softmax_argmax(dev(lg), True)
    none, preds_alone = K.softmax_argmax(dev(lg), False)
    probs, preds, preds_alone = probs.cpu(), preds.cpu(), preds_alone.cpu()
    print(f"[head] non-finite rows J={J}: preds {preds.tolist()}, without probs {preds_alone.tolist()}, torch {want_preds.tolist()}")
    assert bool(torch.isnan(probs[bad]).all()), "a non-finite row has no probabilities"
    assert bool(((preds >= 0) & (preds < J)).all()) and bool(((preds_alone >= 0) & (preds_alone < J)).all()), preds.tolist()
    assert torch.equal(preds, want_preds) and torch.equal(preds_alone, want_preds), (preds.tolist(), want_preds.tolist())
    # the finite rows of the batch: what they are without the others
    fprobs, fpreds = K.softmax_argmax(dev(fin), True)
    same_bits(probs[[0, 5]], fprobs, "finite rows beside non-finite ones")
    assert torch.equal(preds[[0, 5]], fpreds.cpu())
    measured(fprobs, torch.softmax(fin.double(), 1), 1e-5, f"softmax of the finite rows J={J}")


# ------------------------------------------------------------------------------------------------------------------ dropout
@pytest.mark.parametrize("p", [0.0, 0.2, 0.5])
@pytest.mark.parametrize("n", [1, 255, 257, 7681])
def test_dropout_is_one_f32_multiplication(n, p):
    """out = u >= p ? x * (1 / (1 - p)) : 0 with p and the quotient in f32: bit for bit.  u == p is kept, the next f32 towards 0
    is dropped; at p = 0 everything is kept and the factor is 1."""
    K = _k()
    g = torch.Generator().manual_seed(7800 + n)
    x, u = torch.randn(n, generator=g).numpy(), torch.rand(n, generator=g).numpy()
    p32 = np.float32(p)
    below = np.nextafter(p32, np.float32(0))                       # p = 0: 0 itself, kept
    inv = np.float32(np.float32(1) / (np.float32(1) - p32))
    plants = [(p32, below)] if n >= 2 else [(p32,), (below,)]
    for plant in plants:
        uu = u.copy()
        uu[: len(plant)] = plant
        want = np.where(uu >= p32, x * inv, np.float32(0)).astype(np.float32)
        got = K.dropout(dev(torch.from_numpy(x)), dev(torch.from_numpy(uu)), p).cpu().numpy()
        assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32)), (n, p, plant)
        for i, v in enumerate(plant):
            kept = p == 0.0 or v == p32
            assert got[i] == (x[i] * inv if kept else 0.0), f"u = {v!r} at p = {p}: {'kept' if kept else 'dropped'} expected"
        if p == 0.0:
            assert np.array_equal(got.view(np.int32), x.view(np.int32))


# ------------------------------------------------------------------------------------------------------------------ AdamW
ADAMW_COUNTS = (1, 3, 4, 5, 1023, 65536)
# which of (p, g, m, v) start one float into their buffer (4 bytes off a 16-byte boundary): any one sends the chunk down the scalar path
ADAMW_PLACINGS = {"aligned": (0, 0, 0, 0), "all off": (1, 1, 1, 1), "g off": (0, 1, 0, 0), "m off": (0, 0, 1, 0)}
CANARY = 12345.678


def _place(host: torch.Tensor, off: bool):
    """(buffer, view): `host` in device memory with canaries on both sides; the view starts 4 bytes (off) or 16 bytes into the buffer."""
    lead = 1 if off else 4
    buf = torch.full((lead + host.numel() + (1 if off else 4),), CANARY, device="cuda")
    view = buf[lead: lead + host.numel()]
    view.copy_(host)
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == (4 if off else 0)
    return buf, view


def adamw_ref(p, grads, hps):
    """The kernel's recurrence (k_adamw, `upd`) in float64 from the f32 inputs and the f32 hyper-parameter records."""
    p = p.double()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for g, hp in zip(grads, hps):
        lr, b1, b2, eps, wd, bc1, bc2, gs = hp.double().tolist()
        step, rs2, decay = lr / bc1, 1.0 / bc2 ** 0.5, 1.0 - lr * wd
        gg = g.double() * gs
        m = b1 * m + (1 - b1) * gg
        v = b2 * v + (1 - b2) * gg * gg
        p = p * decay - step * (m / (v.sqrt() * rs2 + eps))
    return p, m, v


@pytest.mark.parametrize("wd", [0.0, 5e-2])
@pytest.mark.parametrize("gs", [1.0, 0.5])
def test_adamw_chunks_at_any_alignment(gs, wd):
    """Three steps over one table that holds every chunk size four times: at 16-byte-aligned addresses (float4 loop and its tail),
    with all four addresses 4 bytes off, with only the gradient off and with only exp_avg off (the scalar loop).  Each copy against
    float64; the floats around every view untouched; and the copies of one chunk equal bit for bit, since both loops run the same
    `upd` and the library is built without FMA contraction."""
    K = _k()
    gen = torch.Generator().manual_seed(7900)
    steps = 3
    hps = [torch.tensor([3e-3, 0.9, 0.999, 1e-8, wd, 1 - 0.9 ** s, 1 - 0.999 ** s, gs], dtype=torch.float32) for s in range(1, steps + 1)]
    data, rows, chunks = {}, [], []
    for cnt in ADAMW_COUNTS:
        p0 = torch.randn(cnt, generator=gen)
        grads = [torch.randn(cnt, generator=gen) for _ in range(steps)]
        data[cnt] = (p0, grads)
        for name, offs in ADAMW_PLACINGS.items():
            placed = [_place(h, bool(o)) for h, o in zip((p0, grads[0], torch.zeros(cnt), torch.zeros(cnt)), offs)]
            rows.append([view.data_ptr() for _, view in placed] + [cnt])
            chunks.append((cnt, name, placed))
    table = torch.tensor(rows, dtype=torch.int64).cuda()
    for s in range(steps):
        for cnt, _, placed in chunks:
            placed[1][1].copy_(data[cnt][1][s])
        K.adamw_step(table, hps[s].cuda())
    torch.cuda.synchronize()
    results = {}
    for cnt, name, placed in chunks:
        p0, grads = data[cnt]
        want = adamw_ref(p0, grads, hps)
        got = [view.cpu() for _, view in placed]
        for what, gi, wi in (("p", 0, 0), ("exp_avg", 2, 1), ("exp_avg_sq", 3, 2)):
            measured(got[gi], want[wi], 1e-5, f"adamw gs={gs} wd={wd} cnt={cnt} {name}: {what}")
        same_bits(got[1], grads[-1], f"adamw cnt={cnt} {name}: the gradient is only read")
        for (buf, view), what in zip(placed, ("p", "g", "exp_avg", "exp_avg_sq")):
            lead = (view.data_ptr() - buf.data_ptr()) // 4
            around = torch.cat([buf[:lead], buf[lead + cnt:]])
            same_bits(around, torch.full_like(around, CANARY), f"adamw cnt={cnt} {name}: the floats around {what}")
        results[cnt, name] = got
    for cnt in ADAMW_COUNTS:
        for name in list(ADAMW_PLACINGS)[1:]:
            for what, gi in (("p", 0), ("exp_avg", 2), ("exp_avg_sq", 3)):
                same_bits(results[cnt, name][gi], results[cnt, "aligned"][gi], f"adamw gs={gs} wd={wd} cnt={cnt}: {what} '{name}' against aligned")
