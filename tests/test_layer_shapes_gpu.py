"""The depthwise, stem and squeeze-excite kernels at every layer geometry of the configurations the reference runs
(tests/_layer_shapes.py): EfficientNet-B0 (timm) at 224 / 160 px, B3 (efficientnet_pytorch, TF-SAME padding frozen at 300 px)
at 224 / 160 / 300 px, EfficientFormerV2-S0 / S1 / S2 at 224 / 160 px.

The depthwise planners pick tile shapes, occupancy classes, the paired-output instance and the XCD remap from each layer's
real map size and padding, so a wrong edge tile shows up at one geometry only; the network-level tests would absorb it into
their bf16 bounds.  Here every geometry is compared, whole tensor against whole tensor, with the CPU oracle
(oracle/ops_ref.py) at N = 2 and the tolerances of tests/test_ops_gpu.py.  Each test loops over all geometries and reports
every mismatch at once.  The drift guard records what the built models hand these kernels and holds the list to it.
"""

from __future__ import annotations

import zlib

import pytest
import torch

from oracle import ops_ref as R
from tests import _layer_shapes as S
from tests.test_ops_gpu import dev, gen, rand_state, sum_parts, tol

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
N = 2
STEMS, DWS, SES = S.all_geometries()


def _k():
    from deepfakedetection_amd import kernels

    return kernels


def _err(got: torch.Tensor, want: torch.Tensor) -> float:
    got, want = got.detach().float().cpu(), want.detach().float().cpu()
    if got.shape != want.shape:
        return float("inf")
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-6)


class Report:
    """Collects every mismatch of a loop over geometries (test_ops_gpu.close's measure: max |error| / max |reference|)."""

    def __init__(self) -> None:
        self.bad: list[str] = []
        self.checked = 0

    def close(self, got, want, rel: float, what: str, geom) -> None:
        self.checked += 1
        err = _err(got, want)
        if not err <= rel:
            self.bad.append(f"{geom}: {what}: max err {err:.3e} > {rel:.1e}")

    def fail(self, what: str, geom, exc: Exception) -> None:
        self.bad.append(f"{geom}: {what}: {type(exc).__name__}: {exc}")

    def done(self) -> None:
        assert self.checked > 0
        assert not self.bad, f"{len(self.bad)} of {self.checked} checks failed:\n" + "\n".join(self.bad)


def _seed(g, salt: int) -> int:
    return (zlib.crc32(repr(tuple(g)).encode()) + salt) % (1 << 31)       # (hash() of a str changes from run to run)


def test_depthwise_forward_at_every_layer_geometry():
    """bf16 forward with the model's prologue and statistics, and raw without statistics; the vector-unit kernels (dfd_tune key 0
    = 0) everywhere and the matrix-core form (key 0 = 9: every shape it serves) wherever C % 16 == 0, against one oracle."""
    K = _k()
    lib = K._L()
    rep = Report()
    try:
        for g in DWS:
            H, W, C, k, s, pt, pl, Ho, Wo = g.geom
            act = S.ACTS[g.pro]
            x = gen((N, H, W, C), _seed(g, 1), BF)
            w = gen((C, 1, k, k), _seed(g, 2), torch.float32, 0.3)
            st = rand_state(C, _seed(g, 3))
            want = R.dwconv_fwd(x.float(), st if g.pro else None, act, w, k, s, pt, pl, Ho, Wo, BF)
            want_raw = R.dwconv_fwd(x.float(), None, 0, w, k, s, pt, pl, Ho, Wo, BF) if g.pro else want
            dx, dw, dst = dev(x), dev(w), dev(st)
            forms = [("vector-unit", 0)] + ([("matrix-core", 9)] if C % 16 == 0 else [])
            for form, mode in forms:
                assert lib.dfd_tune(0, mode) == 0
                try:
                    y, parts, n = K.dwconv_fwd(dx, dst if g.pro else None, act, dw, k, s, pt, pl, Ho, Wo, stats=g.stats)
                    sums = sum_parts(parts, n, C) if g.stats else None
                    y2, _, _ = K.dwconv_fwd(dx, None, 0, dw, k, s, pt, pl, Ho, Wo, stats=False)
                except RuntimeError as exc:
                    rep.fail(f"{form} forward", g, exc)
                    continue
                rep.close(y, want, tol(BF), f"{form} forward y", g)
                if g.stats:
                    rep.close(sums, R.stats_sums(y.float().cpu()), 1e-3, f"{form} forward statistics", g)
                rep.close(y2, want_raw, tol(BF), f"{form} forward raw", g)
    finally:
        lib.dfd_tune(0, 1)
    rep.done()


def test_depthwise_backward_at_every_layer_geometry():
    """bf16 data and weight gradient as the model calls them: the BN-backward map (dz, y, coef) where the layer has statistics,
    the data gradient's BN + act epilogue (with its statistics) and the weight gradient's BN + act prologue where it has them."""
    K = _k()
    rep = Report()
    for g in DWS:
        H, W, C, k, s, pt, pl, Ho, Wo = g.geom
        xin = gen((N, H, W, C), _seed(g, 4), BF)
        dz = gen((N, Ho, Wo, C), _seed(g, 5), BF)
        yraw = gen((N, Ho, Wo, C), _seed(g, 6), BF)
        w = gen((C, 1, k, k), _seed(g, 7), torch.float32, 0.3)
        st = rand_state(C, _seed(g, 8))
        gc = torch.Generator().manual_seed(_seed(g, 9))
        coef = torch.stack([0.5 + torch.rand(C, generator=gc), torch.randn(C, generator=gc) * 0.1, torch.randn(C, generator=gc) * 0.05])
        dy = R.rnd(coef[0] * dz.float() + coef[1] * yraw.float() + coef[2], BF) if g.stats else dz.float()
        xact = R.rnd(R.act_fwd(st[0] * xin.float() + st[1], S.ACTS[g.pro]), BF) if g.pro else xin.float()
        da, want_dw = R.dwconv_bwd(dy, xact, w, k, s, pt, pl, BF)
        z = st[0] * xin.float() + st[1]
        want_dzin = R.rnd(da * R.act_grad(z, S.ACTS[g.epi]), BF) if g.epi else R.rnd(da, BF)
        m = (dev(yraw), dev(coef)) if g.stats else (None, None)
        try:
            dzin, parts, n = K.dwconv_bwd_data(dev(dz), *m, dev(w), dev(xin) if g.epi else None, dev(st) if g.epi else None,
                                               S.ACTS[g.epi], (N, H, W, C), k, s, pt, pl)
            sums = sum_parts(parts, n, C) if g.epi else None
            got_dw = K.dwconv_bwd_weight(dev(dz), *m, dev(xin), dev(st) if g.pro else None, S.ACTS[g.pro], k, s, pt, pl)
        except RuntimeError as exc:
            rep.fail("backward", g, exc)
            continue
        rep.close(dzin, want_dzin, tol(BF), "data gradient", g)
        if g.epi:
            got = dzin.float().cpu()
            xhat = (xin.float() - st[2]) * st[3]
            want_sums = torch.stack([got.reshape(-1, C).double().sum(0), (got * xhat).reshape(-1, C).double().sum(0)]).float()
            rep.close(sums, want_sums, 2e-3, "data-gradient statistics", g)
        rep.close(got_dw, want_dw, 5e-3, "weight gradient", g)
    rep.done()


def test_depthwise_eval_form_at_every_layer_geometry():
    """The f32 inference form (dwconv_eval: conv -> BN -> SiLU stored activated, per-(tile, image) channel sums for the
    squeeze-excite) at every EfficientNet depthwise geometry."""
    K = _k()
    rep = Report()
    rd = torch.float32
    for g in [g for g in DWS if g.eval]:
        H, W, C, k, s, pt, pl, Ho, Wo = g.geom
        x = gen((N, H, W, C), _seed(g, 10), rd)
        w = gen((C, 1, k, k), _seed(g, 11), rd, 0.3)
        st = rand_state(C, _seed(g, 12))
        raw = R.dwconv_fwd(x, None, 0, w, k, s, pt, pl, Ho, Wo, rd)
        want = R.act_fwd(raw * st[0] + st[1], R.ACT_SILU)
        try:
            a, parts, tiles = K.dwconv_eval(dev(x), dev(w), dev(st), R.ACT_SILU, k, s, pt, pl, Ho, Wo)
        except (RuntimeError, ValueError) as exc:
            rep.fail("eval form", g, exc)
            continue
        rep.close(a, want, tol(rd), "eval-form output", g)
        if parts.shape != (tiles, N, C):
            rep.bad.append(f"{g}: eval-form channel sums have shape {tuple(parts.shape)}, not {(tiles, N, C)}")
            continue
        rep.close(parts.double().sum(0), a.double().sum((1, 2)), 1e-5, "eval-form channel sums", g)
    rep.done()


def test_stem_at_every_layer_geometry():
    """stem_conv_fwd (with statistics) and stem_conv_wgrad (with the BN-backward map), bf16 and f32, at each input size and
    padding: B3's frozen (0, 1), the symmetric 1 of timm B0 and of the EfficientFormerV2 stem."""
    K = _k()
    rep = Report()
    for g in STEMS:
        H, W, Co, k, s, pt, pl, Ho, Wo = g
        x = gen((N, H, W, 3), _seed(g, 13), torch.float32)
        w = gen((Co, 3, k, k), _seed(g, 14), torch.float32, 0.3)
        for rd in (BF, torch.float32):
            dz = gen((N, Ho, Wo, Co), _seed(g, 15), rd)
            yraw = gen((N, Ho, Wo, Co), _seed(g, 16), rd)
            coef = rand_state(Co, _seed(g, 17))[:3].contiguous()
            dy = R.rnd(coef[0] * dz.float() + coef[1] * yraw.float() + coef[2], rd)
            try:
                y, parts, n = K.stem_conv_fwd(dev(x), dev(w), rd, s, pt, pl, Ho, Wo)
                sums = sum_parts(parts, n, Co)
                got_dw = K.stem_conv_wgrad(dev(x), dev(dz), dev(yraw), dev(coef), k, s, pt, pl)
            except RuntimeError as exc:
                rep.fail(f"stem {rd}", g, exc)
                continue
            rep.close(y, R.stem_conv_fwd(x, w, s, pt, pl, Ho, Wo, rd), tol(rd), f"stem forward {rd}", g)
            rep.close(sums, R.stats_sums(y.float().cpu()), 1e-3, f"stem statistics {rd}", g)
            rep.close(got_dw, R.stem_conv_wgrad(x, dy, k, s, pt, pl, rd), 5e-3 if rd == BF else 2e-4, f"stem weight gradient {rd}", g)
    rep.done()


def test_squeeze_excite_at_every_layer_geometry():
    """bf16 pool_act, se_fwd and se_bwd (and its deferred form, the FC weight gradients riding on the next act_bn_bwd launch,
    as the training step runs it) at every (H*W, C, SE width)."""
    K = _k()
    rep = Report()
    for g in SES:
        H, W, C, Rr = g
        gg = torch.Generator().manual_seed(_seed(g, 18))
        y = gen((N, H, W, C), _seed(g, 19), BF)
        D = gen((N, H, W, C), _seed(g, 20), BF)
        st = torch.zeros((4, C))
        st[0] = torch.rand(C, generator=gg) + 0.5
        st[1] = torch.randn(C, generator=gg) * 0.1
        st[3] = 1.0
        w1 = torch.randn((Rr, C), generator=gg) * C ** -0.5
        b1 = torch.randn(Rr, generator=gg) * 0.1
        w2 = torch.randn((C, Rr), generator=gg) * Rr ** -0.5
        b2 = torch.randn(C, generator=gg) * 0.1
        a = R.rnd(R.act_fwd(st[0] * y.float() + st[1], R.ACT_SILU), BF)
        want_pooled = a.double().mean((1, 2)).float()
        dy, dD, dst, dw1, db1, dw2, db2 = dev(y), dev(D), dev(st), dev(w1), dev(b1), dev(w2), dev(b2)
        try:
            pooled0 = K.pool_act(dy, dst, R.ACT_SILU)
            pooled, hpre, gate, w2t = K.se_fwd(dy, dst, R.ACT_SILU, dw1, db1, dw2, db2, R.ACT_SILU)
            got = K.se_bwd(dD, dy, dst, R.ACT_SILU, gate, hpre, pooled, dw1, w2t, R.ACT_SILU)
            later = K.se_bwd(dD, dy, dst, R.ACT_SILU, gate, hpre, pooled, dw1, w2t, R.ACT_SILU, defer_wgrad=True)
            K.act_bn_bwd(dD, dy, gate, later[0], dst, R.ACT_SILU, se_job=later[5])
            later = [t.clone() for t in later[:5]]
        except RuntimeError as exc:
            rep.fail("squeeze-excite", g, exc)
            continue
        rep.close(pooled0, want_pooled, 1e-3, "pool_act", g)
        rep.close(pooled, want_pooled, 1e-3, "se_fwd pooled", g)
        # the FC layers from the kernel's own pooled vector: their check is not blurred by the pooling's rounding
        pr = pooled.cpu().clone().requires_grad_(True)
        params = [t.clone().requires_grad_(True) for t in (w1, b1, w2, b2)]
        want_hpre, want_gate = R.se_fc(pr, *params, R.ACT_SILU)
        rep.close(hpre, want_hpre, 1e-4, "se_fwd hpre", g)
        rep.close(gate, want_gate, 1e-4, "se_fwd gate", g)
        if not torch.equal(w2t.cpu(), w2.t()):
            rep.bad.append(f"{g}: se_fwd w2t is not the transpose of w2")
        dgate = (a.double() * D.double()).sum((1, 2)).float()
        want_gate.backward(dgate)
        for t, ref, name in zip(got, [pr.grad] + [p.grad for p in params], ("dpooled", "dw1", "db1", "dw2", "db2")):
            rep.close(t, ref, 2e-3, f"se_bwd {name}", g)
        for t, ref, name in zip(later, got, ("dpooled", "dw1", "db1", "dw2", "db2")):
            if not torch.equal(t, ref):
                rep.bad.append(f"{g}: deferred se_bwd {name} differs from the launch of its own")
    rep.done()


# ---- drift guard: what the models issue is what the list holds
def _act(code: int, state) -> str | None:
    if state is None:
        return None
    return {v: k for k, v in S.ACTS.items()}[code]


def _rec_fwd(x, in_state, in_act, w, k, stride, pad_top, pad_left, Ho, Wo, stats=True):
    _, H, W, C = x.shape
    return ("fwd", (H, W, C, k, stride, pad_top, pad_left, Ho, Wo), _act(in_act, in_state), bool(stats))


def _rec_bwd_data(dz, y, coef, w, xin, in_state, in_act, in_shape, k, stride, pad_top, pad_left):
    _, H, W, C = in_shape
    return ("bwd_data", (H, W, C, k, stride, pad_top, pad_left, dz.shape[1], dz.shape[2]), _act(in_act, xin), coef is not None)


def _rec_bwd_weight(dz, y, coef, xin, in_state, in_act, k, stride, pad_top, pad_left, out=None):
    _, H, W, C = xin.shape
    return ("bwd_weight", (H, W, C, k, stride, pad_top, pad_left, dz.shape[1], dz.shape[2]), _act(in_act, in_state), coef is not None)


def _rec_eval(x, w, out_state, out_act, k, stride, pad_top, pad_left, Ho, Wo):
    _, H, W, C = x.shape
    return ("eval", (H, W, C, k, stride, pad_top, pad_left, Ho, Wo))


def _rec_stem_fwd(x, w, out_dtype, stride, pad_top, pad_left, Ho, Wo, stats=True):
    _, H, W, _ = x.shape
    return ("stem", S.Stem(H, W, w.shape[0], w.shape[2], stride, pad_top, pad_left, Ho, Wo))


def _rec_stem_wgrad(x, dz, y, coef, k, stride, pad_top, pad_left, out=None):
    _, H, W, _ = x.shape
    return ("stem", S.Stem(H, W, dz.shape[3], k, stride, pad_top, pad_left, dz.shape[1], dz.shape[2]))


def _rec_se(y, state, act_in, w1, *rest, **kw):
    _, H, W, C = y.shape
    return ("se", S.Se(H, W, C, w1.shape[0]))


def _rec_se_bwd(D, y, state, act_in, gate, hpre, pooled, w1, *rest, **kw):
    return _rec_se(y, state, act_in, w1)


_RECORDERS = {"dwconv_fwd": _rec_fwd, "dwconv_bwd_data": _rec_bwd_data, "dwconv_bwd_weight": _rec_bwd_weight, "dwconv_eval": _rec_eval,
              "stem_conv_fwd": _rec_stem_fwd, "stem_conv_wgrad": _rec_stem_wgrad, "se_fwd": _rec_se, "se_bwd": _rec_se_bwd}


def _expected(name: str) -> set:
    stems, dws, ses = S.config_geometries(name)
    want = {("stem", g) for g in stems} | {("se", g) for g in ses}
    for g in dws:
        want |= {("fwd", g.geom, g.pro, g.stats), ("bwd_data", g.geom, g.epi, g.stats), ("bwd_weight", g.geom, g.pro, g.stats)}
        if g.eval:
            want.add(("eval", g.geom))
    return want


@pytest.mark.parametrize("name", list(S.CONFIGS))
def test_layer_list_matches_what_the_model_issues(name, monkeypatch):
    """One bf16 training step (forward + backward) at N = 2, and for EfficientNet an f32 eval forward (the inference form),
    with recorders around the depthwise, stem and squeeze-excite entry points: the calls they see are exactly the list's."""
    from deepfakedetection_amd import kernels as K

    family, variant, flavour, size = S.CONFIGS[name]
    seen: set = set()

    def wrap(fn, rec):
        def inner(*args, **kwargs):
            seen.add(rec(*args, **kwargs))
            return fn(*args, **kwargs)

        return inner

    torch.manual_seed(5)
    if family == "efficientnet":
        from deepfakedetection_amd.efficientnet import HipEfficientNet

        net = HipEfficientNet(variant, flavour, 2)
    else:
        from deepfakedetection_amd.efficientformer_v2 import HipEfficientFormerV2

        net = HipEfficientFormerV2(variant, 2, size)
    net = net.cuda().train()
    x = torch.randn(N, 3, size, size, device="cuda").contiguous(memory_format=torch.channels_last)
    for fname, rec in _RECORDERS.items():
        monkeypatch.setattr(K, fname, wrap(getattr(K, fname), rec))
    with torch.autocast("cuda", dtype=BF):
        out = net(x)
    out.float().square().sum().backward()
    if family == "efficientnet":
        with torch.inference_mode():
            net.eval()(x)
    torch.cuda.synchronize()
    want = _expected(name)
    assert seen - want == set(), f"{name}: the model issues kernel calls the layer list does not hold: {sorted(seen - want, key=str)}"
    assert want - seen == set(), f"{name}: the layer list holds calls the model does not issue: {sorted(want - seen, key=str)}"
