"""Fused autograd functions of the FasterViT engine.

  ConvBlockFunction        conv3x3 (+bias) BN GELU conv3x3 (+bias) BN [* gamma] + x          faster_vit.py ConvBlock
  FVDownsampleFunction     LayerNorm2d -> conv3x3 s2                                          Downsample
  TokenInitFunction        dw3x3 (+bias) -> AvgPool2d(k, s)  -> carrier tokens                TokenInitializer
  HATFunction              hierarchical attention block: carrier-token attention + MLP, window attention + MLP
                           over [carrier ; window] tokens, split                              HAT
(the stem uses vit_functions.ConvStemFunction / DenseConvBNFunction with ReLU, the tail TailFunction with one head).

Dense 3x3 convolutions run as im2col + the MFMA GEMM kernels; Linear layers run on the same GEMM kernels with the
bias (and LayerScale, residual, DropPath scale) applied by the BatchNorm-apply pass under an identity statistic
(mean 0, variance 1, eps 0), so `Linear + bias` needs no kernel of its own and its bias gradient is the BN-beta
gradient.  Window bookkeeping (partition, carrier-token concatenation and split) is `dfd_copy_rows` with index
maps built once per batch size.

Every stage follows the plumbing of functions.py: its tensor inputs are cut into records, `Layer` for a convolution or Linear
layer (cut_layers; lin_layer) or a LayerNorm, and for the HAT block also the records below (`Table`, `AttnSub`, `MlpSub`, `Stream`, cut by
cut_hat in the order hat_slots states once); tensors reach the backward through ctx.save_for_backward only, the records are
rebuilt there and never kept on ctx; gradients come back through Layer.grads() / hat_grads().  Reference call sites: trainers/fastervit.py:271 (train), :235 (evaluate),
orchestration/orchestrator.py:529,590; arithmetic per fastervit 1.0.0 faster_vit.py (restated in
oracle/fastervit_ref.py).
"""

from __future__ import annotations

import contextlib
import threading
from dataclasses import dataclass
from itertools import islice

import torch

from . import kernels as K
from ._lib import ACT_GELU, ACT_NONE, ACT_RELU
from .functions import BNRef, Layer, _bn_state, _c, _prep, _rows, _slot, bn_backward, cut_layers
from .vit_functions import _gemm_weight, _partial_rows, pwbn_bwd, pwbn_fwd

_ident_cache: dict = {}


def ident(device: torch.device, C: int):
    """(ones [C], BNRef with mean 0 / variance 1 / eps 0): the identity statistic that turns the BN-apply kernels into
    `+ bias`."""
    key = (device.type, device.index, C)
    hit = _ident_cache.get(key)
    if hit is None:
        with torch.inference_mode(False):
            ones = torch.ones(C, dtype=torch.float32, device=device)
            zeros = torch.zeros(C, dtype=torch.float32, device=device)
        hit = (ones, BNRef(zeros, ones, None, 0.0, 0.0))
        if not (device.type == "cuda" and torch.cuda.is_current_stream_capturing()):
            _ident_cache[key] = hit             # tensors born inside a capture belong to that graph's pool: not cached
    return hit


def tok4(t: torch.Tensor) -> torch.Tensor:
    """[n, T, C] token tensor as the [n, T, 1, C] NHWC view the row kernels take."""
    return t if t.dim() == 4 else t.view(t.shape[0], t.shape[1], 1, t.shape[2])


# =========================================================================== Linear on the GEMM kernels
def lin_layer(w, bias, ls=None, need_w=False, need_b=False, need_ls=False) -> Layer:
    """A Linear layer as the Layer of its identity statistic: gamma is ones, beta the bias (its gradient lands in L.dbeta)."""
    ones, ref = ident(w.device, w.shape[0])
    return Layer(w, None, ones, bias, ref, ls, need_w, need_beta=need_b and bias is not None, need_ls=need_ls)


def lin_fwd(x, w_nk, L: Layer, act=ACT_NONE, residual=None, row_scale=None):
    return pwbn_fwd(x, w_nk, L, False, None, act, residual, row_scale, raw_unused=True)


def lin_bwd(g, x, y, st, w_kn, L: Layer, act, need_dx, dx_residual=None, row_scale=None):
    """-> dx; (dw, dbeta = the bias gradient, dls) land on L"""
    return pwbn_bwd(g, x, y, st, w_kn, L, act, False, need_dx, dx_residual, row_scale, identity=True)


# =========================================================================== coordinate MLPs, batched per level (f32)
@dataclass
class CoordJob:
    """One PosEmbMLPSwinv1D ("pos": table [T, C] added to the tokens) or PosEmbMLPSwinv2D ("cpb": relative-position attention
    bias [H, S, S] = 16 sigmoid(table[idx])) of a hierarchical-attention block."""

    kind: str                       # "pos" | "cpb"
    coords: torch.Tensor            # [T, 2] f32 constant
    idx: torch.Tensor | None = None     # cpb: int32 [n_local^2]
    n_local: int = 0
    n_global: int = 0


class CoordTablesFunction(torch.autograd.Function):
    """Every coordinate MLP of a level: Linear(2, 512) -> ReLU -> Linear(512, D, bias=False) on constant coordinates, and for
    the "cpb" jobs the gather + 16 sigmoid that turns the table into the attention bias.  Inputs: (w0, b0, w2) per job.
    Outputs: one tensor per job ("pos": table [T, D]; "cpb": bias [H, S, S]).  2 launches forward, 2 backward
    (csrc/dfd_coord.hip) — the per-layer form cost ~16 launches per block and sat on every block's critical path."""

    @staticmethod
    def forward(ctx, jobs, *params):
        dev = params[0].device
        tables, outs = [], []
        cj, rp = [], []
        for i, job in enumerate(jobs):
            w0, b0, w2 = params[3 * i:3 * i + 3]
            T, D = job.coords.shape[0], w2.shape[0]
            tab = torch.empty((T, D), dtype=torch.float32, device=dev)
            tables.append(tab)
            cj.append((job.coords, w0, b0, w2, tab))
            if job.kind == "cpb":
                S = job.n_local + job.n_global
                full = torch.empty((D, S, S), dtype=torch.float32, device=dev)
                rp.append((tab, job.idx, full, job.n_local, job.n_global))
                outs.append(full)
            else:
                outs.append(tab)
        K.coord_tables_fwd(cj, rp)
        # never keep an OUTPUT on ctx: output -> grad_fn (this node) -> ctx -> output is a cycle Python's collector cannot see
        # through; it would pin this node and the AccumulateGrad nodes behind it across iterations (and a stale AccumulateGrad
        # node on the legacy stream breaks a later hipGraph capture).  Only the raw tables of the "cpb" jobs are needed.
        ctx.jobs, ctx.params = jobs, params
        ctx.shapes = [tuple(t.shape) for t in tables]
        ctx.raw = [t if job.kind == "cpb" else None for t, job in zip(tables, jobs)]
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gouts):
        jobs, params, shapes, raw = ctx.jobs, ctx.params, ctx.shapes, ctx.raw
        need = ctx.needs_input_grad[1:]
        dev = params[0].device
        grads: list = [None] * len(params)
        cj, rp = [], []
        for i, job in enumerate(jobs):
            g = gouts[i]
            nw0, nb0, nw2 = need[3 * i:3 * i + 3]
            if g is None or not (nw0 or nb0 or nw2):
                continue
            w0, b0, w2 = params[3 * i:3 * i + 3]
            T, D = shapes[i]
            g = _c(g.float())
            if job.kind == "cpb":
                dtab = torch.empty((T, D), dtype=torch.float32, device=dev)
                rp.append((raw[i], job.idx, g, dtab, job.n_local, job.n_global))
                g = dtab
            dw0, db0, dw2 = _place(None, w0, nw0), _place(None, b0, nb0), _place(None, w2, nw2)
            grads[3 * i], grads[3 * i + 1], grads[3 * i + 2] = dw0, db0, dw2
            cj.append((job.coords, w0, b0, w2, g, dw0, db0, dw2))
        K.coord_tables_bwd(rp, cj)
        return (None, *grads)


def coord_tables(jobs: list, params: list) -> list:
    """[table | bias per job] for `jobs` (CoordJob) with their (w0, b0, w2) parameter triples flattened in `params`."""
    return list(CoordTablesFunction.apply(jobs, *params))


# =========================================================================== attention / MLP sub-blocks on [n, T, C]
_derived_tls = threading.local()


@contextlib.contextmanager
def derived_weights(table: dict | None):
    """Inside the block the Linear layers take the (w_nk, w_kn) pairs of `table` ({weight.data_ptr(): pair}, refreshed for the
    whole network by ONE batched launch per forward pass — kernels.DerivedWeights) instead of one small launch each: the
    `derived` of vit_functions._prep."""
    prev = getattr(_derived_tls, "table", None)
    _derived_tls.table = table
    try:
        yield
    finally:
        _derived_tls.table = prev


def window_attention_fwd(qkv, bias, H: int):
    """softmax(q k^T * scale + bias) v on qkv [n, T, 1, 3C] (q | k | v per token, read in place) -> (O [n, T, 1, C], saved).
    The fused MFMA kernel (csrc/dfd_attn.hip) where kernels.wattn_supported (saved = the log-sum-exp rows), else batched
    GEMM -> softmax rows -> batched GEMM (saved = P, f32 [n, H, T, T])."""
    n, T, _, C3 = qkv.shape
    C = C3 // 3
    hd = C // H
    if K.wattn_supported(qkv.dtype, T, hd):
        # fused MFMA attention: S and P stay in registers; the backward recomputes P from L
        return K.wattn_fwd(qkv, bias, H, hd ** -0.5)
    S = torch.empty((n, H, T, T), dtype=torch.float32, device=qkv.device)
    q, k, v = qkv.view(n * T, 3 * C)[:, 0:C], qkv.view(n * T, 3 * C)[:, C:2 * C], qkv.view(n * T, 3 * C)[:, 2 * C:]
    K.bgemm(q, (T * 3 * C, hd, 3 * C, 1), k, (T * 3 * C, hd, 1, 3 * C), S, (H * T * T, T * T, T, 1), n, H, T, T, hd,
            alpha=hd ** -0.5, bias=bias)
    Pm, _ = K.attn_softmax_fwd(S, None)
    O = torch.empty((n, T, 1, C), dtype=qkv.dtype, device=qkv.device)
    K.bgemm(Pm, (H * T * T, T * T, T, 1), v, (T * 3 * C, hd, 3 * C, 1), O, (T * C, hd, C, 1), n, H, T, hd, T)
    return O, Pm


def window_attention_bwd(qkv, dO, saved, bias, H: int, need_bias: bool):
    """-> (dqkv [n, T, 1, 3C], dbias [H*T*T] f32 or None) of window_attention_fwd; dO [n, T, 1, C]."""
    n, T, _, C3 = qkv.shape
    C = C3 // 3
    hd = C // H
    dev = qkv.device
    L = T * T
    if K.wattn_supported(qkv.dtype, T, hd):
        return K.wattn_bwd(qkv, dO, saved, bias, H, hd ** -0.5, need_bias)            # saved holds the log-sum-exp rows here
    Pm = saved
    q, k, v = qkv.view(n * T, 3 * C)[:, 0:C], qkv.view(n * T, 3 * C)[:, C:2 * C], qkv.view(n * T, 3 * C)[:, 2 * C:]
    dT2 = torch.empty((n, H, T, T), dtype=torch.float32, device=dev)
    K.bgemm(dO, (T * C, hd, C, 1), v, (T * 3 * C, hd, 1, 3 * C), dT2, (H * L, L, T, 1), n, H, T, T, hd)
    dqkv = torch.empty_like(qkv)
    dq, dk, dv = dqkv.view(n * T, 3 * C)[:, 0:C], dqkv.view(n * T, 3 * C)[:, C:2 * C], dqkv.view(n * T, 3 * C)[:, 2 * C:]
    K.bgemm(Pm, (H * L, L, 1, T), dO, (T * C, hd, C, 1), dv, (T * 3 * C, hd, 3 * C, 1), n, H, T, hd, T)
    dS_buf = torch.empty((_partial_rows(n), H, T, T), dtype=torch.float32, device=dev)
    _, dS = K.attn_softmax_bwd(dT2, Pm, None, out=dS_buf[:n])
    scale = hd ** -0.5
    K.bgemm(dS, (H * L, L, T, 1), k, (T * 3 * C, hd, 3 * C, 1), dq, (T * 3 * C, hd, 3 * C, 1), n, H, T, hd, T, alpha=scale)
    K.bgemm(dS, (H * L, L, 1, T), q, (T * 3 * C, hd, 3 * C, 1), dk, (T * 3 * C, hd, 3 * C, 1), n, H, T, hd, T, alpha=scale)
    dfull = None
    if need_bias:
        dfull = torch.empty(H * L, dtype=torch.float32, device=dev)
        K.sum_rows(dS_buf.view(-1), n, H * L, dfull)
    return dqkv, dfull


# =========================================================================== records of the HAT block
# Like functions.Layer: tensors, one need flag per tensor (need_<field>) and the gradient the backward produced (d<field>); built
# afresh from the arguments in `forward` and from ctx.saved_tensors in `backward`.  A LayerNorm is a Layer of gamma and beta alone.
@dataclass
class Table:
    """An output of CoordTablesFunction: a position table [T, C] or a relative-position attention bias [H, T, T]."""

    tab: torch.Tensor | None = None
    need_tab: bool = False
    dtab: torch.Tensor | None = None


@dataclass
class AttnSub:
    ln: Layer
    qkv: Layer
    proj: Layer             # proj.ls: the sub-block's LayerScale (gamma3, or gamma1 on the carrier tokens), None without one
    bias: Table


@dataclass
class MlpSub:
    ln: Layer
    fc1: Layer
    fc2: Layer              # fc2.ls: gamma4 / gamma2


@dataclass
class Stream:
    """What one token stream of the block goes through: position table, attention sub-block, MLP sub-block.  A block has the
    window stream and, with carrier tokens, the carrier stream in front of it."""

    pos: Table
    attn: AttnSub
    mlp: MlpSub


def _stream_slots(s: Stream):
    """(record, field) of the stream's tensor inputs in input order, and of its two LayerScales, which come behind both streams."""
    a, m = s.attn, s.mlp
    return ([(s.pos, "tab"), (a.ln, "gamma"), (a.ln, "beta"), (a.qkv, "w"), (a.qkv, "beta"), (a.proj, "w"), (a.proj, "beta"), (a.bias, "tab"),
             (m.ln, "gamma"), (m.ln, "beta"), (m.fc1, "w"), (m.fc1, "beta"), (m.fc2, "w"), (m.fc2, "beta")],
            [(a.proj, "ls"), (m.fc2, "ls")])


def hat_slots(win: Stream, car: Stream | None) -> list:
    """(record, field) of every tensor input of HATFunction behind (x, ct, cfg) and in front of the two DropPath row scales: the
    window stream, the carrier stream, gamma3, gamma4, gamma1, gamma2.  The one statement of that order: hat_inputs, cut_hat and
    hat_grads all walk it."""
    streams = [_stream_slots(s) for s in (win, car) if s is not None]
    return [slot for main, _ in streams for slot in main] + [slot for _, scales in streams for slot in scales]


def hat_inputs(win: Stream, car: Stream | None, rs_win=None, rs_ct=None) -> list:
    """HATFunction's tensor inputs behind (x, ct, cfg): the tensors of the records, then the two DropPath row scales."""
    return [getattr(r, f) for r, f in hat_slots(win, car)] + [rs_win, rs_ct]


def cut_hat(t, need, carrier: bool):
    """(window stream, carrier stream or None, (rs_win, rs_ct)) from HATFunction's tensor inputs `t` behind (x, ct, cfg).
    need: the slice of ctx.needs_input_grad that lines up with t (None in a forward: every flag False)."""
    def blank():
        ln1, qkv, proj, ln2, fc1, fc2 = (Layer(None, None, None, None) for _ in range(6))
        return Stream(Table(), AttnSub(ln1, qkv, proj, Table()), MlpSub(ln2, fc1, fc2))

    win, car = blank(), blank() if carrier else None
    slots = hat_slots(win, car)
    for i, (r, f) in enumerate(slots):
        setattr(r, f, t[i])
        if need is not None and need[i] and t[i] is not None:
            setattr(r, "need_" + f, True)
    for L in [L for s in (win, car) if s is not None for L in (s.attn.qkv, s.attn.proj, s.mlp.fc1, s.mlp.fc2)]:
        L.gamma, L.bn = ident(L.w.device, L.w.shape[0])           # see lin_layer
    return win, car, tuple(t[len(slots):])


def hat_grads(win: Stream, car: Stream | None) -> list:
    """One gradient per tensor input of hat_inputs, in its order: those on the records, each masked by its own flag, and none for
    the row scales."""
    return [getattr(r, "d" + f) if getattr(r, "need_" + f) else None for r, f in hat_slots(win, car)] + [None, None]


def _place(val, param, need: bool, slot=None):
    """Where a wanted f32 gradient of `param` lives: its gradient-arena slot if the parameter has a free one (slot: that slot, where
    the caller has claimed it already), else a tensor of its own.  val: the freshly computed gradient, moved into the slot by one
    launch or handed back as it is; None: the buffer itself, for the caller's kernel to write."""
    if not need:
        return None
    if slot is None:
        slot = _slot(param, True, tuple(param.shape))
    if val is None:
        return slot if slot is not None else torch.empty_like(param)
    if slot is None:
        return val.view(param.shape)
    return K.axpby(val.reshape(-1), None, 1.0, 0.0, out=slot.view(-1)).view(param.shape)


def _ln_bwd(dxn, x, ln: Layer, lnst, residual=None):
    """LayerNorm backward with the skip connection's gradient added in the same kernel -> dx; (dgamma, dbeta) land on ln, summed
    straight into the parameters' gradient-arena slots when both are wanted and the slots are adjacent (weight, bias: they are)."""
    C = ln.gamma.numel()
    sw = _slot(ln.gamma, ln.need_gamma, (C,))
    sb = _slot(ln.beta, ln.need_beta, (C,))
    if sw is not None and sb is not None and sb.data_ptr() == sw.data_ptr() + 4 * C:
        dx, ln.dgamma, ln.dbeta = K.layernorm_bwd(dxn, x, ln.gamma, lnst, residual, torch.as_strided(sw, (2, C), (C, 1)))
        return dx
    dx, dg, db = K.layernorm_bwd(dxn, x, ln.gamma, lnst, residual)
    ln.dgamma, ln.dbeta = _place(dg, ln.gamma, ln.need_gamma, sw), _place(db, ln.beta, ln.need_beta, sb)
    return dx


N_ATTN_SAVED, N_MLP_SAVED = 12, 10          # tensors attn_sub_fwd / mlp_sub_fwd keep for their backward


def attn_sub_fwd(x, A: AttnSub, heads: int, row_scale):
    """x + [rs *] [ls *] proj(softmax(q k^T * scale + bias) v) with q, k, v = qkv(LN(x)) -> (out, saved)."""
    dt = x.dtype
    derived = getattr(_derived_tls, "table", None)
    xn, lnst = K.layernorm_fwd(x, A.ln.gamma, A.ln.beta, 1e-5)
    wq_nk, wq_kn = _prep(A.qkv.w, dt, derived)
    qkv, yq, stq = lin_fwd(xn, wq_nk, A.qkv)
    O, Pm = window_attention_fwd(qkv, A.bias.tab, heads)
    wp_nk, wp_kn = _prep(A.proj.w, dt, derived)
    out, yp, stp = lin_fwd(O, wp_nk, A.proj, ACT_NONE, x, row_scale)
    return out, (x, xn, lnst, qkv, yq, stq, Pm, O, yp, stp, wq_kn, wp_kn)


def attn_sub_bwd(g, saved, A: AttnSub, heads: int, row_scale, need_dx: bool):
    """-> dx (None unless need_dx); the parameter and bias gradients land on A's records."""
    x, xn, lnst, qkv, yq, stq, Pm, O, yp, stp, wq_kn, wp_kn = saved
    T = x.shape[1]
    need_xn = need_dx or A.ln.need_bn
    upstream = need_xn or A.qkv.need_w or A.qkv.need_beta or A.bias.need_tab
    dO = lin_bwd(g, O, yp, stp, wp_kn, A.proj, ACT_NONE, upstream, None, row_scale)
    if not upstream:
        return None
    dqkv, dfull = window_attention_bwd(qkv, dO, Pm, A.bias.tab, heads, A.bias.need_tab)
    if A.bias.need_tab:
        A.bias.dtab = dfull.view(heads, T, T)
    dxn = lin_bwd(dqkv, xn, yq, stq, wq_kn, A.qkv, ACT_NONE, need_xn)
    if not need_xn:
        return None
    dx = _ln_bwd(dxn, x, A.ln, lnst, g if need_dx else None)
    return dx if need_dx else None


def _lin_apply(x, w_nk, st, act, residual=None, row_scale=None, want_raw=True):
    """act(x w^T + bias) [* ls] [* rs] [+ residual] under the coefficient block `st` -> (out, raw product or None): one kernel where
    the shape is dfd_gemm's, else the product and one apply pass."""
    fused = K.gemm_bias_act(x, w_nk, st, act, residual, row_scale, want_raw=want_raw)
    if fused is not None:
        return fused
    y, _, _ = K.pwconv(x, None, w_nk, None, stats=False)
    return K.bn_act_apply(y, st, act, residual, row_scale), y


def mlp_sub_fwd(x, M: MlpSub, row_scale):
    """x + [rs *] [ls *] fc2(GELU(fc1(LN(x)))) -> (out, saved).
    Not two lin_fwd calls: both layers' derived weights and coefficient blocks are made before the first product, and a block
    used on its own launches each of them, so going through lin_fwd (state, then product, per layer) would reorder launches."""
    dt = x.dtype
    derived = getattr(_derived_tls, "table", None)
    fc1, fc2 = M.fc1, M.fc2
    xn, lnst = K.layernorm_fwd(x, M.ln.gamma, M.ln.beta, 1e-5)
    w1_nk, w1_kn = _prep(fc1.w, dt, derived)
    st1 = _bn_state(None, 0, _rows(xn), fc1.bn, fc1.gamma, fc1.beta, False)
    w2_nk, w2_kn = _prep(fc2.w, dt, derived)
    st2 = _bn_state(None, 0, _rows(xn), fc2.bn, fc2.gamma, fc2.beta, False, None, None, fc2.ls)
    # fc1 + bias + GELU and fc2 + bias (+ LayerScale, DropPath row scale, skip connection) are one kernel each where the shape
    # is dfd_gemm's (the activated hidden tensor `a` and the pre-activation `h` both leave fc1's epilogue: `h` for GELU');
    # otherwise the activated tensor is materialised by one pass — as a GEMM prologue the GELU was evaluated once per
    # 128-column output tile by fc2's forward and again by its weight gradient
    a, h = _lin_apply(xn, w1_nk, st1, ACT_GELU)
    # y2 is None from the one-kernel form without LayerScale: the backward never reads it (and `out` must not stand in: a
    # Function must not save its own output)
    out, y2 = _lin_apply(a, w2_nk, st2, ACT_NONE, x, row_scale, want_raw=fc2.ls is not None)
    return out, (x, xn, lnst, h, a, st1, y2, st2, w1_kn, w2_kn)


def mlp_sub_bwd(g, saved, M: MlpSub, row_scale, need_dx: bool):
    """-> dx (None unless need_dx); the parameter gradients land on M's records.  Its own launch sequence, not lin_bwd's: with
    LayerScale fc2's mapped gradient dz2 is materialised once (affine2_apply) instead of being a GEMM prologue, and fc1's
    bn_backward runs only when its bias gradient is wanted (dz1 needs no coefficients under the identity statistic)."""
    x, xn, lnst, h, a, st1, y2, st2, w1_kn, w2_kn = saved
    ln, fc1, fc2 = M.ln, M.fc1, M.fc2
    C, hid = fc2.w.shape[0], fc1.w.shape[0]
    gb = K.scale_rows(g, row_scale) if row_scale is not None else g
    # fc2 has no BatchNorm: the backward map of its identity statistic is dz = ls * g.  Without layer scale that is g itself and
    # the bias gradient is the column sums of g (one reduction launch, its final summation in the block's batch); with it the
    # BatchNorm-shaped pair runs and the scaled gradient is materialised once (as a GEMM prologue it was evaluated once per
    # 128-column tile of the data gradient — 8 times per element at hidden 1024 — and read y2 only to multiply it by zero)
    if fc2.ls is None:
        if fc2.need_beta:
            fc2.dbeta = K.bias_grad(gb, None, _slot(fc2.beta, True, (C,)))
        dz2 = gb
    else:
        parts, n = K.bn_bwd_reduce(gb, y2, st2, None)
        dz2 = K.affine2_apply(gb, y2, bn_backward(fc2, parts, n, _rows(y2), st2, False))
    need_xn = need_dx or ln.need_bn
    if fc2.need_w:
        fc2.dw = K.pwconv_wgrad(dz2, None, a, None, _slot(fc2.w, True, (C, hid))).view(fc2.w.shape)
    if not (need_xn or fc1.need_w or fc1.need_beta):
        return None
    D, _, _ = K.pwconv(dz2, None, w2_kn, None, stats=False)
    dz1, parts, n = K.act_bn_bwd(D, h, None, None, st1, ACT_GELU)
    if fc1.need_beta:
        bn_backward(fc1, parts, n, _rows(h), st1, False)
    if fc1.need_w:
        fc1.dw = K.pwconv_wgrad(dz1, None, xn, None, _slot(fc1.w, True, (hid, C))).view(fc1.w.shape)
    if not need_xn:
        return None
    dxn, _, _ = K.pwconv(dz1, None, w1_kn, None, stats=False)
    dx = _ln_bwd(dxn, x, ln, lnst, g if need_dx else None)
    return dx if need_dx else None


# =========================================================================== HAT block
@dataclass
class HATCtx:
    heads: int
    carrier: bool                       # level 2: carrier-token stream + concatenation
    cat_src_ct: torch.Tensor | None     # int32 [nW*4]: carrier row of every (window, slot)
    cat_dst_ct: torch.Tensor | None     # int32 [nW*4]: its row in the concatenated tensor
    cat_dst_x: torch.Tensor | None      # int32 [nW*49]: row of every window token in the concatenated tensor


class HATFunction(torch.autograd.Function):
    """One hierarchical-attention block.  x: [nW, 49, 1, C] window tokens; ct: [B, 16, 1, C] carrier tokens in row-major
    image order (None without carrier tokens); then hat_inputs(...), rs_win, rs_ct.  Returns (x_out, ct_out)."""

    @staticmethod
    def forward(ctx, x, ct, cfg: HATCtx, *t):
        win, car, (rs_win, rs_ct) = cut_hat(t, None, cfg.carrier)
        nW, Tw, _, C = x.shape
        x1 = K.add_rowtable(x, win.pos.tab)
        per, kept = 0, ()
        if cfg.carrier:
            B, Tc = ct.shape[0], ct.shape[1]
            c1 = K.add_rowtable(ct, car.pos.tab)
            c2, hattn_saved = attn_sub_fwd(c1, car.attn, cfg.heads, rs_ct)
            c3, hmlp_saved = mlp_sub_fwd(c2, car.mlp, rs_ct)
            per = Tc * B // nW                                      # carrier tokens per window (4)
            xc = torch.empty((nW, Tw + per, 1, C), dtype=x.dtype, device=x.device)
            K.copy_rows(c3.view(-1, C), cfg.cat_src_ct, xc.view(-1, C), cfg.cat_dst_ct, nW * per)
            K.copy_rows(x1.view(-1, C), None, xc.view(-1, C), cfg.cat_dst_x, nW * Tw)
            kept = (*hattn_saved, *hmlp_saved)
        else:
            xc = x1
        xa, attn_saved = attn_sub_fwd(xc, win.attn, cfg.heads, rs_win)
        xm, mlp_saved = mlp_sub_fwd(xa, win.mlp, rs_win)
        if cfg.carrier:
            x_out = torch.empty_like(x)
            ct_out = torch.empty_like(ct)
            K.copy_rows(xm.view(-1, C), cfg.cat_dst_x, x_out.view(-1, C), None, nW * Tw)
            K.copy_rows(xm.view(-1, C), cfg.cat_dst_ct, ct_out.view(-1, C), cfg.cat_src_ct, nW * per)
        else:
            x_out, ct_out = xm, None
        ctx.cfg, ctx.per = cfg, per
        ctx.shapes = (tuple(x.shape), tuple(ct.shape) if ct is not None else None, x.dtype)
        # the inputs, then what the two or four sub-blocks kept; never an output (without carrier tokens x_out is mlp_sub_fwd's)
        ctx.save_for_backward(*t, *kept, *attn_saved, *mlp_saved)
        if ct_out is None:
            ctx.mark_non_differentiable()
            return x_out, None
        return x_out, ct_out

    @staticmethod
    @K.batched_sums
    def backward(ctx, gx, gct):
        cfg: HATCtx = ctx.cfg
        per = ctx.per
        x_shape, ct_shape, dt = ctx.shapes
        need_x, need_ct, _, *need = ctx.needs_input_grad
        saved = ctx.saved_tensors
        win, car, (rs_win, rs_ct) = cut_hat(saved[:len(need)], need, cfg.carrier)
        kept = iter(saved[len(need):])
        if cfg.carrier:
            hattn_saved, hmlp_saved = tuple(islice(kept, N_ATTN_SAVED)), tuple(islice(kept, N_MLP_SAVED))
        attn_saved, mlp_saved = tuple(islice(kept, N_ATTN_SAVED)), tuple(islice(kept, N_MLP_SAVED))
        nW, Tw, _, C = x_shape
        dev = gx.device
        carrier_up = cfg.carrier and (need_ct or any(getattr(r, "need_" + f) for part in _stream_slots(car) for r, f in part))
        need_x1 = need_x or win.pos.need_tab
        gx = _c(gx)
        if cfg.carrier:
            gm = torch.empty((nW, Tw + per, 1, C), dtype=dt, device=dev)
            K.copy_rows(gx.view(-1, C), None, gm.view(-1, C), cfg.cat_dst_x, nW * Tw)
            if gct is not None:
                K.copy_rows(_c(gct).view(-1, C), cfg.cat_src_ct, gm.view(-1, C), cfg.cat_dst_ct, nW * per)
            else:
                zero = torch.zeros((nW * per, C), dtype=dt, device=dev)
                K.copy_rows(zero, None, gm.view(-1, C), cfg.cat_dst_ct, nW * per)
        else:
            gm = gx
        dxa = mlp_sub_bwd(gm, mlp_saved, win.mlp, rs_win, True)
        dxc = attn_sub_bwd(dxa, attn_saved, win.attn, cfg.heads, rs_win, need_x1 or carrier_up)
        dx = dct = None
        if cfg.carrier:
            dx1 = None
            if need_x1:
                dx1 = torch.empty(x_shape, dtype=dt, device=dev)
                K.copy_rows(dxc.view(-1, C), cfg.cat_dst_x, dx1.view(-1, C), None, nW * Tw)
            if carrier_up:
                dc3 = torch.empty(ct_shape, dtype=dt, device=dev)
                K.copy_rows(dxc.view(-1, C), cfg.cat_dst_ct, dc3.view(-1, C), cfg.cat_src_ct, nW * per)
                dc2 = mlp_sub_bwd(dc3, hmlp_saved, car.mlp, rs_ct, True)
                dc1 = attn_sub_bwd(dc2, hattn_saved, car.attn, cfg.heads, rs_ct, need_ct or car.pos.need_tab)
                if car.pos.need_tab:
                    car.pos.dtab = K.rowtable_grad(dc1, ct_shape[1])
                dct = dc1 if need_ct else None
        else:
            dx1 = dxc
        if need_x1:
            if win.pos.need_tab:
                win.pos.dtab = K.rowtable_grad(dx1, Tw)
            dx = dx1 if need_x else None
        return (dx, dct, None, *hat_grads(win, car))




# =========================================================================== ConvBlock (levels 0, 1)
@dataclass
class ConvBlockCtx:
    bn1: BNRef
    bn2: BNRef
    training: bool
    counters: list | None = None


class ConvBlockFunction(torch.autograd.Function):
    """x + [rs *] [gamma *] BN(conv3x3(GELU(BN(conv3x3(x)))))  (both convolutions with bias, folded into the BNs)."""

    @staticmethod
    def forward(ctx, x, w1, b1, g1, be1, w2, b2, g2, be2, gamma, row_scale, cfg: ConvBlockCtx):
        tr = cfg.training
        N, H, W, C = x.shape
        need_bwd = any(ctx.needs_input_grad)
        w1_nk, _ = _gemm_weight(w1, x.dtype, False)
        w1_kn = _dgrad_weight(w1, x.dtype) if need_bwd else None          # [C][(flipped tap, co)]: stride-1 data gradient
        y1, parts, n = K.conv_fwd(x, None, ACT_NONE, w1_nk, 3, 1, 1, H, W, stats=tr)
        st1 = _bn_state(parts, n, N * H * W, cfg.bn1, g1, be1, tr, cfg.counters, conv_bias=b1)
        w2_nk, _ = _gemm_weight(w2, x.dtype, False)
        w2_kn = _dgrad_weight(w2, x.dtype) if need_bwd else None
        # GELU(BN(y1)) is materialised once (one streaming pass, ~45 us at level 0): as the prologue of the second convolution and
        # of its weight gradient it was evaluated on every staged tile with its halo, per output-channel group, on the
        # workgroup's critical path — +50 us and +54 us per block against the plain kernels (same bits either way)
        a1 = K.bn_act_apply(y1, st1, ACT_GELU)
        y2, parts, n = K.conv_fwd(a1, None, ACT_NONE, w2_nk, 3, 1, 1, H, W, stats=tr)
        st2 = _bn_state(parts, n, N * H * W, cfg.bn2, g2, be2, tr, cfg.counters, conv_bias=b2, ls=gamma)
        out = K.bn_act_apply(y2, st2, ACT_NONE, x, row_scale)
        ctx.cfg = cfg
        ctx.save_for_backward(x, y1, a1, y2, st1, st2, w1_kn, w2_kn, w1, b1, g1, be1, w2, b2, g2, be2, gamma, row_scale)
        return out

    @staticmethod
    @K.batched_sums
    def backward(ctx, g):
        cfg: ConvBlockCtx = ctx.cfg
        x, y1, a1, y2, st1, st2, w1_kn, w2_kn, *t = ctx.saved_tensors
        need = ctx.needs_input_grad
        c1, c2 = cut_layers(("conv1", "conv2"), t, need[1:], 0, None).values()
        c2.ls, c2.need_ls, row_scale = t[8], need[9], t[9]
        tr = cfg.training
        N, H, W, C = x.shape
        rows = N * H * W
        g = _c(g)
        gb = K.scale_rows(g, row_scale) if row_scale is not None else g
        parts, n = K.bn_bwd_reduce(gb, y2, st2, None)
        coef2 = bn_backward(c2, parts, n, rows, st2, tr)
        dz2 = K.affine2_apply(gb, y2, coef2)              # the BN-backward-mapped gradient, once for both consumers
        if c2.need_w:
            dwg = K.conv_wgrad(dz2, None, a1, None, ACT_NONE, 3, 1, 1)
            c2.dw = K.conv_wgrad_from_gemm(dwg, tuple(c2.w.shape), _slot(c2.w, True, tuple(c2.w.shape)))
        # data gradient of a stride-1 convolution = the forward convolution of the BN-backward-mapped gradient with the
        # flipped, transposed weight: no [M][9C] column matrix, no col2im
        da1, _, _ = K.conv_fwd(dz2, None, ACT_NONE, w2_kn, 3, 1, 1, H, W, stats=False)
        dz1, parts, n = K.act_bn_bwd(da1, y1, None, None, st1, ACT_GELU)
        coef1 = bn_backward(c1, parts, n, rows, st1, tr)
        dx = None
        dzm1 = K.affine2_apply(dz1, y1, coef1) if (need[0] or c1.need_w) else None
        if c1.need_w:
            dwg = K.conv_wgrad(dzm1, None, x, None, ACT_NONE, 3, 1, 1)
            c1.dw = K.conv_wgrad_from_gemm(dwg, tuple(c1.w.shape), _slot(c1.w, True, tuple(c1.w.shape)))
        if need[0]:
            dx0, _, _ = K.conv_fwd(dzm1, None, ACT_NONE, w1_kn, 3, 1, 1, H, W, stats=False)
            dx = K.add(dx0, g)
        return (dx, *c1.grads(), *c2.grads(), c2.dls, None, None)


def _dgrad_weight(w: torch.Tensor, dt: torch.dtype):
    w_nk, _ = K.prep_weights(K.conv_weight_to_dgrad_gemm(w), dt, True, False)
    return w_nk


# =========================================================================== Downsample (LayerNorm2d + conv3x3 s2)
class FVDownsampleFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ln_w, ln_b, w):
        N, H, W, C = x.shape
        need_bwd = any(ctx.needs_input_grad)
        xn, lnst = K.layernorm_fwd(x, ln_w, ln_b, 1e-6)
        w_nk, w_kn = _gemm_weight(w, x.dtype, need_bwd)
        Ho, Wo = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
        y, _, _ = K.conv_fwd(xn, None, ACT_NONE, w_nk, 3, 2, 1, Ho, Wo, stats=False)
        ctx.save_for_backward(x, xn, lnst, w_kn, ln_w, ln_b, w)
        return y

    @staticmethod
    @K.batched_sums
    def backward(ctx, g):
        x, xn, lnst, w_kn, ln_w, ln_b, w = ctx.saved_tensors
        need = ctx.needs_input_grad
        N, H, W, C = x.shape
        g = _c(g)
        dw = dx = dlw = dlb = None
        if need[3]:
            dwg = K.conv_wgrad(g, None, xn, None, ACT_NONE, 3, 2, 1)
            dw = K.conv_wgrad_from_gemm(dwg, tuple(w.shape), _slot(w, True, tuple(w.shape)))
        if need[0] or need[1] or need[2]:
            dcol, _, _ = K.pwconv(g, None, w_kn, None, stats=False)
            dxn = K.col2im(dcol, (N, H, W, C), 3, 2, 1)
            dx, dgm, dbt = K.layernorm_bwd(dxn, x, ln_w, lnst)
            dlw, dlb = _place(dgm, ln_w, need[1]), _place(dbt, ln_b, need[2])
            if not need[0]:
                dx = None
        return dx, dlw, dlb, dw


# =========================================================================== carrier-token initialiser
class TokenInitFunction(torch.autograd.Function):
    """dw3x3 (+bias) -> AvgPool2d(kernel, stride): [B, H, W, C] -> [B, h*w, 1, C] carrier tokens in row-major order."""

    @staticmethod
    def forward(ctx, x, w, b, kernel: int, stride: int):
        N, H, W, C = x.shape
        y, _, _ = K.dwconv_fwd(x, None, ACT_NONE, w, 3, 1, 1, 1, H, W, stats=False)
        p = K.avgpool_fwd(y, kernel, stride)
        out = K.add_rowtable(p, b.view(1, C))
        ctx.save_for_backward(x, w, b)
        ctx.geom = (kernel, stride, tuple(y.shape))
        return out.view(N, p.shape[1] * p.shape[2], 1, C)

    @staticmethod
    @K.batched_sums
    def backward(ctx, g):
        x, w, b = ctx.saved_tensors
        kernel, stride, yshape = ctx.geom
        need = ctx.needs_input_grad
        N, H, W, C = x.shape
        ho = (H - kernel) // stride + 1
        g4 = _c(g).view(N, ho, -1, C)
        db = _place(K.rowtable_grad(g4, 1).view(-1), b, need[2])
        dx = dw = None
        if need[0] or need[1]:
            dy = K.avgpool_bwd(g4, yshape, kernel, stride)
            if need[0]:
                dx, _, _ = K.dwconv_bwd_data(dy, None, None, w, None, None, ACT_NONE, tuple(x.shape), 3, 1, 1, 1)
            if need[1]:
                dw = K.dwconv_bwd_weight(dy, None, None, x, None, ACT_NONE, 3, 1, 1, 1, _slot(w, True, (C, 1, 3, 3)))
        return dx, dw, db, None, None


__all__ = ["ConvBlockCtx", "ConvBlockFunction", "FVDownsampleFunction", "HATCtx", "HATFunction", "TokenInitFunction"]
