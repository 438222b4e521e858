"""Fused autograd functions of the HIP engine: stem, MBConv block, classifier head, loss.

One torch.autograd.Function per network stage.  Inside a stage the tensors that an
unfused framework would write to HBM after every BatchNorm / SiLU / SE multiply never
exist: each conv kernel writes its RAW output plus per-channel partial sums, a tiny
finalize kernel turns the sums into (scale, shift, mean, rstd), and the NEXT kernel
applies normalisation + activation (+ SE gate) while it loads its operand.  Backward
re-derives activations from the saved raw tensors the same way and uses the identity
    d(conv out) = a[c]*dz + b[c]*y + c[c]
for training-mode BatchNorm, so BN-backward is also folded into the consumers.

This module also holds what the stages of all three families share (vit_functions.py and fastervit_functions.py import it):
the `Layer` record of one "conv (+bias) + BatchNorm [+ LayerScale]" layer, `cut_layers` which cuts a stage's tensor inputs
into such records, `bn_backward`, the gradient-arena look-up `_slot` and the derived-weight look-up `_prep`.

Stage arithmetic mirrors efficientnet_pytorch 0.7.1 `MBConvBlock.forward` /
timm 1.0.20 `InvertedResidual.forward` (reference call sites:
trainers/efficientnet.py:297,302; orchestration/orchestrator.py:529,590).
"""

from __future__ import annotations

import contextlib
import os
import threading
from dataclasses import dataclass

import torch

from . import kernels as K
from ._lib import ACT_NONE, ACT_SILU
from .arch import ConvGeom
from .arena import grad_dest


@dataclass
class BNRef:
    """A BatchNorm2d's buffers + hyper-parameters (its weight/bias travel as Function inputs)."""

    running_mean: torch.Tensor
    running_var: torch.Tensor
    num_batches_tracked: torch.Tensor | None
    momentum: float
    eps: float

    def params(self, weight: torch.Tensor, bias: torch.Tensor) -> K.BNParams:
        return K.BNParams(weight, bias, self.running_mean, self.running_var, self.momentum, self.eps)


def _bn_state(parts, nparts, count: int, bn: BNRef, weight, bias, training: bool, counters: list | None = None,
              conv_bias=None, ls=None) -> torch.Tensor:
    """BatchNorm coefficients of one layer.  `counters`: the list owned by the calling network's forward pass; the
    layer's num_batches_tracked is appended and the network bumps all of them with ONE launch at the end
    (kernels.DeviceRng.tick).  A stage used on its own (counters None) bumps its counter itself."""
    params = bn.params(weight, bias)
    params.conv_bias, params.ls = conv_bias, ls
    if training:
        if bn.num_batches_tracked is not None:
            if counters is not None:
                counters.append(bn.num_batches_tracked)
            else:
                bn.num_batches_tracked.add_(1)
        return K.bn_finalize(parts, nparts, count, params)
    return _bn_eval_state(params)


def _bn_eval_state(params: K.BNParams) -> torch.Tensor:
    """Eval-mode coefficient block: from the pass's batch (bn_eval_batch) where one is active, else one small launch."""
    batch = getattr(_bn_batch_tls, "batch", None)
    if batch is not None:
        return batch.request(params)
    return K.bn_eval_coeffs(params)


_bn_batch_tls = threading.local()


def eval_fused_enabled(elems: int, dtype: torch.dtype) -> bool:
    """Whether an MBConv block whose depthwise input has `elems` elements of `dtype` runs the inference form
    (MBConvFunction._forward_eval).  Measured (profiles/r02_eval_forms.md): the SiLU of a producer epilogue is
    exposed VALU time (two half-rate transcendentals per element), the same SiLU in a consumer's staging phase hides under
    its loads — so the inference form only wins where launches, not VALU, bound the block: f32 tensors up to 32 M elements
    (batch <= 64 at 224 px: -2..3 % replayed, -6 % eager); in bf16 it never does.  DFD_EVAL_FUSED=0 / 1 forces the
    training-form chain / the inference form (A/B switch of scripts/eval_small.py and of the parity test)."""
    flag = os.environ.get("DFD_EVAL_FUSED")
    if flag is not None:
        return flag != "0"
    return dtype == torch.float32 and elems <= int(os.environ.get("DFD_EVAL_FUSED_MAX_ELEMS", EVAL_FUSED_MAX_ELEMS))


EVAL_FUSED_MAX_ELEMS = 32 << 20


@contextlib.contextmanager
def bn_eval_batch(owner: dict, tag):
    """Inside the block, eval-mode BatchNorm coefficient blocks come from `owner`'s kernels.BNEvalBatch for `tag` (one per
    network and mode): recorded on the first pass, one batched launch from the second pass on."""
    batches = owner.setdefault("_bn_eval_batches", {})
    batch = batches.get(tag)
    if batch is None:
        batch = batches[tag] = K.BNEvalBatch()
    prev = getattr(_bn_batch_tls, "batch", None)
    _bn_batch_tls.batch = batch
    batch.begin()
    try:
        yield batch
    finally:
        _bn_batch_tls.batch = prev
        batch.end()


def _c(t: torch.Tensor) -> torch.Tensor:
    return t if t.is_contiguous() else t.contiguous()


def _slot(t: torch.Tensor | None, need: bool, shape):
    """Gradient-arena slot of parameter `t` if it wants a gradient and its slot is free."""
    if not need or t is None:
        return None
    return grad_dest(t.data_ptr(), shape)


def _rows(t: torch.Tensor) -> int:
    return t.numel() // t.shape[-1]


@dataclass
class Layer:
    """One "conv (+bias) + BatchNorm [+ LayerScale]" layer of a stage: its tensors, one need flag per tensor (all False in a
    forward, where only the tensors matter) and the gradients its backward produced.  A plain record: built afresh from the
    arguments in `forward` and from ctx.saved_tensors in `backward`, never kept on ctx."""

    w: torch.Tensor | None
    b: torch.Tensor | None
    gamma: torch.Tensor
    beta: torch.Tensor | None
    bn: BNRef | None = None
    ls: torch.Tensor | None = None
    need_w: bool = False
    need_b: bool = False
    need_gamma: bool = False
    need_beta: bool = False
    need_ls: bool = False
    dw: torch.Tensor | None = None
    db: torch.Tensor | None = None
    dgamma: torch.Tensor | None = None
    dbeta: torch.Tensor | None = None
    dls: torch.Tensor | None = None

    @property
    def need_bn(self) -> bool:
        """gamma and beta share one launch flag: the kernel writes both."""
        return self.need_gamma or self.need_beta

    @property
    def need_any(self) -> bool:
        return self.need_w or self.need_b or self.need_bn

    def grads(self, bias: bool = True):
        """(dw, db, dgamma, dbeta) in input order, each masked by its own flag; bias=False: without db (see cut_layers)."""
        db = (self.db if self.need_b else None,) if bias else ()
        return (self.dw if self.need_w else None, *db,
                self.dgamma if self.need_gamma else None, self.dbeta if self.need_beta else None)


def cut_layers(names, t, need, offset: int, bns, bias: bool = True) -> dict[str, Layer]:
    """{name: Layer} for the (weight, bias, bn.weight, bn.bias) quads that start at t[offset], one per name.
    need: the slice of ctx.needs_input_grad that lines up with t (None in a forward); bns: name -> BNRef, or None.
    bias=False: the stage's convolutions have no bias and its inputs are (weight, bn.weight, bn.bias) triples; Layer.b is None."""
    out, width = {}, 4 if bias else 3
    for i, nm in enumerate(names):
        o = offset + width * i
        q, flags = list(t[o: o + width]), list(need[o: o + width]) if need is not None else [False] * width
        if not bias:
            q.insert(1, None)
            flags.insert(1, False)
        out[nm] = Layer(*q, bns[nm] if bns is not None else None, None, *flags)
    return out


def bn_backward(L: Layer, parts, n, rows: int, st, training: bool):
    """The BatchNorm-backward coefficients of L from the partial sums; dgamma, dbeta, dls and the convolution-bias gradient land
    on L — in their gradient-arena slots, each claimed only when this launch really writes it."""
    C = L.gamma.numel()
    nb, want_ls, want_b = L.need_bn, L.need_ls and L.ls is not None, L.need_b and L.b is not None
    outs = (_slot(L.gamma, nb, (C,)), _slot(L.beta, nb, (C,)), _slot(L.ls, want_ls, (C,)), _slot(L.b, want_b, (C,)))
    coef, L.dgamma, L.dbeta, L.dls, L.db = K.bn_bwd_finalize(parts, n, rows, L.gamma, L.beta, L.ls, st, training, nb, want_ls,
                                                             want_b, outs)
    return coef


def _prep(w: torch.Tensor, dt: torch.dtype, derived, need_bwd: bool = True):
    """(w_nk, w_kn) of a 1x1 convolution weight [O, I, 1, 1] (or a 2-D GEMM weight) in the activation dtype.
    derived: {weight.data_ptr(): (w_nk, w_kn)} refreshed for the whole network by one batched launch per forward
    (kernels.DerivedWeights; w_nk a kernels.MxWeight with FasterViT's fp8 weights), or None: prepare this layer on the spot.
    An entry of another dtype than `dt` (a table handed on into another autocast region) is not used."""
    if derived is not None:
        hit = derived.get(w.data_ptr())
        if hit is not None and (isinstance(hit[0], K.MxWeight) or hit[0].dtype == dt):
            return hit
    return K.prep_weights(w, dt, True, need_bwd)


# =========================================================================== stem
@dataclass
class StemCtx:
    geom: ConvGeom
    bn: BNRef
    dtype: torch.dtype
    training: bool
    counters: list | None = None          # see _bn_state


class StemFunction(torch.autograd.Function):
    """conv k3 s2 (3 -> C) + BN + SiLU.  x: [N,H,W,3] f32."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, cfg: StemCtx):
        g = cfg.geom
        N, H, W, _ = x.shape
        Ho, Wo = g.out_size(H), g.out_size(W)
        y, parts, n = K.stem_conv_fwd(x, weight, cfg.dtype, g.stride, g.pad_lead, g.pad_lead, Ho, Wo, stats=cfg.training)
        st = _bn_state(parts, n, N * Ho * Wo, cfg.bn, gamma, beta, cfg.training, cfg.counters)
        out = K.bn_act_apply(y, st, ACT_SILU)
        ctx.cfg = cfg
        ctx.save_for_backward(x, y, st, weight, gamma, beta)
        return out

    @staticmethod
    def backward(ctx, g):
        cfg: StemCtx = ctx.cfg
        x, y, st, *t = ctx.saved_tensors
        L = cut_layers(("conv",), t, ctx.needs_input_grad[1:], 0, None, bias=False)["conv"]
        geom = cfg.geom
        pads = (geom.kernel, geom.stride, geom.pad_lead, geom.pad_lead)
        if L.need_w and K.stem_bwd_fused_ok(x, y, *pads):
            # dz has one consumer, the weight gradient, which recomputes it from g and y: the sums only, no dz tensor (same bits)
            g = _c(g)
            _, parts, n = K.act_bn_bwd(g, y, None, None, st, ACT_SILU, want_dz=False)
            coef = bn_backward(L, parts, n, _rows(y), st, cfg.training)
            L.dw = K.stem_bwd_fused(x, g, y, st, ACT_SILU, coef, *pads, _slot(L.w, True, tuple(L.w.shape)))
            return (None, *L.grads(bias=False), None)
        dz, parts, n = K.act_bn_bwd(_c(g), y, None, None, st, ACT_SILU)
        coef = bn_backward(L, parts, n, _rows(y), st, cfg.training)
        if L.need_w:
            L.dw = K.stem_conv_wgrad(x, dz, y, coef, geom.kernel, geom.stride, geom.pad_lead, geom.pad_lead,
                                     _slot(L.w, True, tuple(L.w.shape)))
        return (None, *L.grads(bias=False), None)


# =========================================================================== MBConv
@dataclass
class MBConvCtx:
    expand: bool
    dw: ConvGeom
    skip: bool
    bn_expand: BNRef | None
    bn_dw: BNRef
    bn_project: BNRef
    training: bool
    derived: dict | None = None           # see _prep; the squeeze-excite expand weight's entry is (None, se_w2t): _se_w2t
    counters: list | None = None          # see _bn_state
    # autograd state at the call site (inside Function.forward grad mode is always off, and needs_input_grad reflects
    # requires_grad alone): False under no_grad / inference_mode, where nothing has to be kept for a backward pass
    grad_enabled: bool = True


def _mb_layers(t, need, cfg: MBConvCtx):
    """(expand, dw, project) records and the four squeeze-excite tensors of MBConvFunction's tensor inputs `t` behind x."""
    bns = {"expand": cfg.bn_expand, "dw": cfg.bn_dw, "project": cfg.bn_project}
    Ls = cut_layers(("expand", "dw"), t, need, 0, bns, bias=False) | cut_layers(("project",), t, need, 10, bns, bias=False)
    return *Ls.values(), t[6:10]


def _se_mats(se):
    """The squeeze-excite weights [R, C, 1, 1], [C, R, 1, 1] as matrices, with their biases."""
    return se[0].reshape(se[0].shape[0], -1), se[1], se[2].reshape(se[2].shape[0], -1), se[3]


def _se_w2t(w: torch.Tensor, derived) -> torch.Tensor | None:
    """The f32 [R][C] copy of the squeeze-excite expand weight from the network's derived-weight table (see _prep; its entry
    holds no w_nk); None: kernels.se_fwd makes it."""
    hit = derived.get(w.data_ptr()) if derived is not None else None
    return hit[1] if hit is not None else None


class MBConvFunction(torch.autograd.Function):
    """[1x1 expand + BN + SiLU] -> dw kxk + BN + SiLU -> SE -> 1x1 project + BN [-> *mask + x].

    Tensor inputs (None where a block has no expand conv):
      x, w_exp, g_exp, b_exp, w_dw, g_dw, b_dw, se_w1, se_b1, se_w2, se_b2, w_proj, g_proj, b_proj, row_scale
    """

    @staticmethod
    def forward(ctx, x, w_exp, g_exp, b_exp, w_dw, g_dw, b_dw, se_w1, se_b1, se_w2, se_b2, w_proj, g_proj, b_proj,
                row_scale, cfg: MBConvCtx):
        t = (w_exp, g_exp, b_exp, w_dw, g_dw, b_dw, se_w1, se_b1, se_w2, se_b2, w_proj, g_proj, b_proj)
        exp, dw, proj, se = _mb_layers(t, None, cfg)
        tr = cfg.training
        N, H, W, Cin = x.shape
        dt = x.dtype
        geom = cfg.dw
        Ho, Wo = geom.out_size(H), geom.out_size(W)
        need_bwd = any(ctx.needs_input_grad)   # grad mode is off inside forward(); this is the autograd view
        if not tr and not (need_bwd and cfg.grad_enabled) and eval_fused_enabled(
                N * H * W * (exp.w.shape[0] if cfg.expand else Cin), dt):
            return MBConvFunction._forward_eval(x, exp, dw, proj, se, cfg, Ho, Wo)
        if cfg.expand:
            wexp_nk, wexp_kn = _prep(exp.w, dt, cfg.derived, need_bwd)
            y1, parts, n = K.pwconv(x, None, wexp_nk, None, stats=tr)
            st1 = _bn_state(parts, n, N * H * W, exp.bn, exp.gamma, exp.beta, tr, cfg.counters)
            y2, parts, n = K.dwconv_fwd(y1, st1, ACT_SILU, dw.w, geom.kernel, geom.stride, geom.pad_lead, geom.pad_lead,
                                        Ho, Wo, stats=tr)
        else:
            wexp_kn, y1, st1 = None, None, None
            y2, parts, n = K.dwconv_fwd(x, None, ACT_NONE, dw.w, geom.kernel, geom.stride, geom.pad_lead, geom.pad_lead,
                                        Ho, Wo, stats=tr)
        st2 = _bn_state(parts, n, N * Ho * Wo, dw.bn, dw.gamma, dw.beta, tr, cfg.counters)
        pooled, hpre, gate, w2t = K.se_fwd(y2, st2, ACT_SILU, *_se_mats(se), ACT_SILU, _se_w2t(se[2], cfg.derived))
        wproj_nk, wproj_kn = _prep(proj.w, dt, cfg.derived, need_bwd)
        pro = K.pro_bn_act_gate(st2, ACT_SILU, gate, Ho * Wo)
        y3, parts, n = K.pwconv(y2, pro, wproj_nk, None, stats=tr)
        st3 = _bn_state(parts, n, N * Ho * Wo, proj.bn, proj.gamma, proj.beta, tr, cfg.counters)
        out = K.bn_act_apply(y3, st3, ACT_NONE, x if cfg.skip else None, row_scale if cfg.skip else None)
        ctx.cfg = cfg
        ctx.has_rs = cfg.skip and row_scale is not None
        ctx.save_for_backward(x, y1, y2, y3, st1, st2, st3, pooled, hpre, gate, wexp_kn, wproj_kn, w2t, *t,
                              row_scale if ctx.has_rs else None)
        return out

    @staticmethod
    def _forward_eval(x, exp: Layer, dw: Layer, proj: Layer, se, cfg, Ho, Wo):
        """Inference form (running statistics, nothing kept for a backward pass): every BatchNorm is an affine map known up
        front, so each PRODUCER stores its activated output and the depthwise kernel also leaves the squeeze-excite channel
        sums — no consumer prologues, no pooling pass.  Per stage the values are those of the reference's autocast graph
        (conv -> bn -> SiLU each rounded to the activation dtype; timm InvertedResidual.forward / efficientnet_pytorch
        MBConvBlock.forward)."""
        N, H, W, Cin = x.shape
        dt = x.dtype
        geom = cfg.dw
        a1 = x
        if cfg.expand:
            wexp_nk, _ = _prep(exp.w, dt, cfg.derived, False)
            st1 = _bn_state(None, 0, N * H * W, exp.bn, exp.gamma, exp.beta, False, cfg.counters)
            a1 = K.pwconv_eval(x, wexp_nk, st1, ACT_SILU)
        st2 = _bn_state(None, 0, N * Ho * Wo, dw.bn, dw.gamma, dw.beta, False, cfg.counters)
        a2, pool_parts, _ = K.dwconv_eval(a1, dw.w, st2, ACT_SILU, geom.kernel, geom.stride, geom.pad_lead, geom.pad_lead, Ho, Wo)
        _, gate, _ = K.se_fwd_parts(pool_parts, Ho * Wo, *_se_mats(se), ACT_SILU, _se_w2t(se[2], cfg.derived))
        wproj_nk, _ = _prep(proj.w, dt, cfg.derived, False)
        pro = K.pro_bn_act_gate(K.identity_state(x.device, a2.shape[3]), ACT_NONE, gate, Ho * Wo)     # gate only
        y3, _, _ = K.pwconv(a2, pro, wproj_nk, None, stats=False)
        st3 = _bn_state(None, 0, N * Ho * Wo, proj.bn, proj.gamma, proj.beta, False, cfg.counters)
        return K.bn_act_apply(y3, st3, ACT_NONE, x if cfg.skip else None, None)

    @staticmethod
    @K.batched_sums                 # the three weight gradients' final sums: one pair of launches at the end of the block
    def backward(ctx, g):
        cfg: MBConvCtx = ctx.cfg
        x, y1, y2, y3, st1, st2, st3, pooled, hpre, gate, wexp_kn, wproj_kn, w2t, *t, row_scale = ctx.saved_tensors
        need = ctx.needs_input_grad
        exp, dw, proj, se = _mb_layers(t, need[1:], cfg)
        tr = cfg.training
        geom = cfg.dw
        N, H, W, Cin = x.shape
        _, Ho, Wo, Cmid = y2.shape
        g = _c(g)
        gb = K.scale_rows(g, row_scale) if ctx.has_rs else g
        # ---- project BN backward, folded into the two GEMMs that consume dy3
        parts, n = K.bn_bwd_reduce(gb, y3, st3, None)
        Cout, R = y3.shape[3], se[0].shape[0]
        w1 = se[0].reshape(R, -1)
        coef3 = bn_backward(proj, parts, n, N * Ho * Wo, st3, tr)
        # the BN-backward-mapped gradient [rows][Cout] is materialised once for its two GEMMs: as a prologue it is re-evaluated
        # (and y3 re-read) per 128-column tile of the Cmid-wide data gradient (B0: 13.99 -> 13.90 ms per step; same bits)
        gm3 = K.affine2_apply(gb, y3, coef3)
        D, _, _ = K.pwconv(gm3, None, wproj_kn, None, stats=False)                   # d(act*gate) [.., Cmid]
        if proj.need_w:
            pro_q = K.pro_bn_act_gate(st2, ACT_SILU, gate, Ho * Wo)
            proj.dw = K.pwconv_wgrad(gm3, None, y2, pro_q, _slot(proj.w, True, (Cout, Cmid))).view(Cout, Cmid, 1, 1)
        # ---- squeeze-excite backward
        need_se = need[7:11]
        se_outs = tuple(_slot(p, nd, shape) for p, nd, shape in zip(se, need_se, ((R, Cmid), (R,), (Cmid, R), (Cmid,))))
        # the FC weight gradients (read by the optimizer only) ride along with the next launch instead of being one of their own
        se_res = K.se_bwd(D, y2, st2, ACT_SILU, gate, hpre, pooled, w1, w2t, ACT_SILU, any(need_se), se_outs, defer_wgrad=True)
        dpooled, dw1, db1, dw2, db2 = se_res[:5]
        se_job = se_res[5]
        # ---- SiLU' and depthwise BN backward
        dz2, parts, n = K.act_bn_bwd(D, y2, gate, dpooled, st2, ACT_SILU, se_job=se_job)
        if dw1 is not None:
            dw1, dw2 = dw1.view(dw1.shape[0], -1, 1, 1), dw2.view(dw2.shape[0], -1, 1, 1)
        coef2 = bn_backward(dw, parts, n, N * Ho * Wo, st2, tr)
        dx = None
        if cfg.expand:
            dz1, parts, n = K.dwconv_bwd_data(dz2, y2, coef2, dw.w, y1, st1, ACT_SILU, y1.shape, geom.kernel,
                                              geom.stride, geom.pad_lead, geom.pad_lead)
            coef1 = bn_backward(exp, parts, n, N * H * W, st1, tr)
            pro_dy1 = K.pro_affine2(y1, coef1)
            # blocks 1-3: data and weight gradient of the expand layer from ONE pass over (dz1, y1), the widest tensors of the
            # network (csrc/dfd_pwtnw.hip, DG) — bit-identical to the two kernels below
            both = K.pwconv_bwd_fused(dz1, y1, coef1, x, wexp_kn, g if cfg.skip else None, _slot(exp.w, True, (Cmid, Cin))) \
                if (need[0] and exp.need_w and K.pwconv_bwd_fused_ok(dz1, x)) else None
            if dw.need_w:
                dw.dw = K.dwconv_bwd_weight(dz2, y2, coef2, y1, st1, ACT_SILU, geom.kernel, geom.stride,
                                            geom.pad_lead, geom.pad_lead, _slot(dw.w, True, tuple(dw.w.shape)))
            if exp.need_w and both is None:
                exp.dw = K.pwconv_wgrad(dz1, pro_dy1, x, None, _slot(exp.w, True, (Cmid, Cin))).view(Cmid, Cin, 1, 1)
            if both is not None:
                dx, exp.dw = both[0], both[1].view(Cmid, Cin, 1, 1)
            elif need[0]:
                dx, _, _ = K.pwconv(dz1, pro_dy1, wexp_kn, g if cfg.skip else None, stats=False)
        else:
            if dw.need_w:
                dw.dw = K.dwconv_bwd_weight(dz2, y2, coef2, x, None, ACT_NONE, geom.kernel, geom.stride,
                                            geom.pad_lead, geom.pad_lead, _slot(dw.w, True, tuple(dw.w.shape)))
            if need[0]:
                dx, _, _ = K.dwconv_bwd_data(dz2, y2, coef2, dw.w, None, None, ACT_NONE, tuple(x.shape), geom.kernel,
                                             geom.stride, geom.pad_lead, geom.pad_lead)
                if cfg.skip:
                    dx = K.add(dx, g)
        return (dx, *exp.grads(bias=False), *dw.grads(bias=False), dw1, db1, dw2, db2, *proj.grads(bias=False), None, None)


# =========================================================================== head
@dataclass
class HeadCtx:
    bn: BNRef
    dropout: float
    training: bool
    derived: dict | None = None           # see _prep
    counters: list | None = None          # see _bn_state


class HeadFunction(torch.autograd.Function):
    """1x1 conv + BN + SiLU -> global average pool -> dropout -> Linear.  Returns f32 logits."""

    @staticmethod
    def forward(ctx, x, w_head, gamma, beta, w_fc, b_fc, drop_u, cfg: HeadCtx):
        N, H, W, Cin = x.shape
        need_bwd = any(ctx.needs_input_grad)
        w_nk, w_kn = _prep(w_head, x.dtype, cfg.derived, need_bwd)
        y, parts, n = K.pwconv(x, None, w_nk, None, stats=cfg.training)
        st = _bn_state(parts, n, N * H * W, cfg.bn, gamma, beta, cfg.training, cfg.counters)
        pooled = K.pool_act(y, st, ACT_SILU)
        feat = K.dropout(pooled, drop_u, cfg.dropout) if drop_u is not None else pooled
        logits = K.linear_fwd(feat, w_fc, b_fc)
        ctx.cfg = cfg
        ctx.save_for_backward(x, y, st, feat, w_kn, w_head, gamma, beta, w_fc, b_fc, drop_u)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        cfg: HeadCtx = ctx.cfg
        x, y, st, feat, w_kn, *t, w_fc, b_fc, drop_u = ctx.saved_tensors
        need = ctx.needs_input_grad
        head = cut_layers(("head",), t, need[1:], 0, None, bias=False)["head"]
        need_wfc, need_bfc = need[4], need[5] and b_fc is not None
        Chead, Cin = y.shape[3], x.shape[3]
        backbone = need[0] or head.need_any
        J = w_fc.shape[0]
        # K.linear_bwd writes a bias gradient only next to the weight gradient: a classifier whose bias alone is trained asks for
        # both (the weight gradient goes to a temporary and is dropped)
        dfeat, dw_fc, db_fc = K.linear_bwd(_c(dlogits.float()), feat, w_fc, backbone, need_wfc or need_bfc, need_bfc,
                                           _slot(w_fc, need_wfc, (J, Chead)), _slot(b_fc, need_bfc, (J,)))
        dx = None
        if backbone:
            dpooled = K.dropout(dfeat, drop_u, cfg.dropout) if drop_u is not None else dfeat
            dz, parts, n = K.act_bn_bwd(None, y, None, dpooled, st, ACT_SILU)
            coef = bn_backward(head, parts, n, _rows(y), st, cfg.training)
            pro = K.pro_affine2(y, coef)
            if need[0]:
                dx, _, _ = K.pwconv(dz, pro, w_kn, None, stats=False)
            if head.need_w:
                head.dw = K.pwconv_wgrad(dz, pro, x, None, _slot(head.w, True, (Chead, Cin))).view(Chead, Cin, 1, 1)
        return dx, *head.grads(bias=False), dw_fc if need_wfc else None, db_fc, None, None

# =========================================================================== hooked head (Grad-CAM)
class HeadConvFunction(torch.autograd.Function):
    """The head's 1x1 convolution alone (raw output, NHWC): used when forward hooks sit on the head-conv
    module, so that its OUTPUT exists as an autograd tensor (web_ui.py:96-114 attaches Grad-CAM there)."""

    @staticmethod
    def forward(ctx, x, w_head):
        w_nk, w_kn = K.prep_weights(w_head, x.dtype, True, True)
        y, _, _ = K.pwconv(x, None, w_nk, None, stats=False)
        ctx.save_for_backward(x, w_kn)
        return y

    @staticmethod
    def backward(ctx, g):
        x, w_kn = ctx.saved_tensors
        g = _c(g)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx, _, _ = K.pwconv(g, None, w_kn, None, stats=False)
        if ctx.needs_input_grad[1]:
            dw = K.pwconv_wgrad(g, None, x, None).view(g.shape[3], x.shape[3], 1, 1)
        return dx, dw


class HeadTailEvalFunction(torch.autograd.Function):
    """Eval-mode BN + SiLU -> global average pool -> Linear on the raw head-conv output.  Differentiable
    with respect to that activation only (the Grad-CAM use): parameters get no gradient here."""

    @staticmethod
    def forward(ctx, y, w_fc, b_fc, bn: BNRef, gamma, beta):
        st = _bn_eval_state(bn.params(gamma, beta))
        pooled = K.pool_act(y, st, ACT_SILU)
        logits = K.linear_fwd(pooled, w_fc, b_fc)
        ctx.save_for_backward(y, st, pooled, w_fc)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        y, st, pooled, w_fc = ctx.saved_tensors
        dy = None
        if ctx.needs_input_grad[0]:
            dpooled, _, _ = K.linear_bwd(_c(dlogits.float()), pooled, w_fc, True, False, False, None, None)
            dz, _, _ = K.act_bn_bwd(None, y, None, dpooled, st, ACT_SILU)          # d loss / d (BN output)
            C = y.shape[3]
            coef = torch.empty((3, C), dtype=torch.float32, device=y.device)        # eval BN: dy = scale * dz
            coef[0].copy_(st[0])
            coef[1:].zero_()
            dy = K.affine2_apply(dz, y, coef)
        return dy, None, None, None, None, None



# =========================================================================== loss
class CrossEntropyFunction(torch.autograd.Function):
    """Mean label-smoothed cross entropy of f32 logits (trainers/efficientnet.py:412).  Like torch's, it takes class
    indices (int64 [N]) or class probabilities (floating [N, J], what mix.BatchMixer produces)."""

    @staticmethod
    def forward(ctx, logits, targets, label_smoothing: float):
        if targets.is_floating_point():
            if targets.shape != logits.shape:
                raise ValueError(f"probability targets must have the logits' shape {tuple(logits.shape)}, got {tuple(targets.shape)}")
            loss, dlogits = K.ce_loss_soft(_c(logits), _c(targets.float()), label_smoothing, 1.0, ctx.needs_input_grad[0])
        else:
            loss, dlogits = K.ce_loss(_c(logits), targets, label_smoothing, 1.0, ctx.needs_input_grad[0])
        ctx.save_for_backward(dlogits)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        (dlogits,) = ctx.saved_tensors
        return K.axpby(dlogits, None, 1.0, 0.0, a_dev=gloss.reshape(1).float()), None, None


class WeightedCrossEntropyFunction(torch.autograd.Function):
    """CrossEntropyFunction with per-class weights (f32 [J] or None) and the focal factor (1 - p)^gamma, through dfd_ce_loss_w.
    The mean is torch's: over the targets' weights with class indices, over N with probabilities.  The weights get no gradient."""

    @staticmethod
    def forward(ctx, logits, targets, label_smoothing: float, focal_gamma: float, class_weight):
        if targets.is_floating_point():
            if targets.shape != logits.shape:
                raise ValueError(f"probability targets must have the logits' shape {tuple(logits.shape)}, got {tuple(targets.shape)}")
            targets = _c(targets.float())
        loss, dlogits = K.ce_loss_w(_c(logits), targets, label_smoothing, focal_gamma, class_weight, 1.0, ctx.needs_input_grad[0])
        ctx.save_for_backward(dlogits)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        (dlogits,) = ctx.saved_tensors
        return K.axpby(dlogits, None, 1.0, 0.0, a_dev=gloss.reshape(1).float()), None, None, None, None


__all__ = ["BNRef", "CrossEntropyFunction", "HeadConvFunction", "HeadCtx", "HeadFunction", "HeadTailEvalFunction", "Layer", "MBConvCtx",
           "MBConvFunction", "StemCtx", "StemFunction", "WeightedCrossEntropyFunction", "bn_backward", "cut_layers"]
