"""The class-weighted and focal cross entropy on the device (dfd_ce_loss_w, ABI 147): the kernel against the float64 reference of
tests/_wloss_ref.py on the shapes, logit regimes and targets of tests/test_head_gpu.py, then the loss module, a captured training
step and the orchestrated trainer.

The tolerances are test_head_gpu's for the two plain cross entropies, under the same close(): 1e-5 on the loss, 2e-4 on dlogits.
Where the denominator sum_n w[t_n] is 0, both sides are NaN; that is asserted and nothing else is compared.  Every comparison
prints its measured error first (pytest -s shows them)."""

from __future__ import annotations

import dataclasses
import functools
import math
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml
from PIL import Image

from deepfakedetection_amd import kernels as K
from tests import _wloss_ref as W
from tests.test_head_gpu import CE_SHAPES, REGIMES, ce_logits, hard_targets, measured, same_bits, soft_targets
from tests.test_ops_gpu import dev

pytestmark = pytest.mark.gpu

EPS = (0.0, 0.1)
GRAD_SCALES = (1.0, 0.25, 128.0)
INF = float("inf")


def class_weights(J: int) -> torch.Tensor:
    """f32 [J] in [0.25, 4]; with more than two classes one weight is exactly 0 (class 1, which hard_targets' first and last rows
    never name, so that the denominator stays positive)."""
    w = torch.rand(J, generator=torch.Generator().manual_seed(8100 + J)) * 3.75 + 0.25
    if J > 2:
        w[1] = 0.0
    return w


def target_sets(N: int, J: int):
    """[(name, targets)]: test_head_gpu's index targets (class 0 and class J - 1 among them) and its probability rows (sums 1, 0.5, 0)."""
    out = [(f"indices {i}", t) for i, t in enumerate(hard_targets(N, J))]
    return out + [(f"probabilities {s}", soft_targets(N, J, s)) for s in range(3 if N < 3 else 1)]


@functools.lru_cache(maxsize=None)
def reference(shape, regime: str, which: int, eps: float, gamma: float, weighted: bool):
    """(loss, dlogits) in float64: computed once per case, shared by the tests, never written to."""
    N, J = shape
    _, tg = target_sets(N, J)[which]
    return W.loss_and_grad(ce_logits(shape, regime), tg, class_weights(J) if weighted else None, eps, gamma)


def check_case(shape, regime: str, which: int, eps: float, gamma: float, weighted: bool) -> None:
    """One (logits, targets, eps, gamma, weights): loss and dlogits at every gradient scale, and the loss alone."""
    N, J = shape
    name, tg = target_sets(N, J)[which]
    w = class_weights(J) if weighted else None
    want, dwant = reference(shape, regime, which, eps, gamma, weighted)
    lgd, tgd, wd = dev(ce_logits(shape, regime)), dev(tg), None if w is None else dev(w)
    what = f"wce {shape} {regime} {name} eps={eps} gamma={gamma} weights={weighted}"
    alone, none = K.ce_loss_w(lgd, tgd, eps, gamma, wd, 1.0, False)
    assert none is None
    for gs in GRAD_SCALES:
        loss, dl = K.ce_loss_w(lgd, tgd, eps, gamma, wd, gs, True)
        if math.isnan(float(want)):                             # the targets carry no weight: torch's mean is 0 / 0
            print(f"[wloss] {what}: the denominator is 0, loss {float(loss)!r}")
            assert math.isnan(float(loss)) and math.isnan(float(alone)), (float(loss), float(alone))
            continue
        measured(loss.reshape(1), want.reshape(1), 1e-5, f"{what} gs={gs}: loss")
        measured(dl, dwant * gs, 2e-4, f"{what} gs={gs}: dlogits")
        same_bits(alone.reshape(1), loss.reshape(1), f"{what} gs={gs}: loss without and with the gradient")
        if J == 1 and gamma > 0:
            assert float(loss) == 0.0 and int(torch.count_nonzero(dl)) == 0, f"{what}: one class has loss 0 and no gradient"


# ------------------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("shape", CE_SHAPES)
def test_weighted_cross_entropy(shape, regime):
    """gamma = 0 under drawn class weights: torch's cross_entropy(weight=, label_smoothing=) (tests/test_wloss_cpu.py pins the
    reference to it), index and probability targets."""
    for which in range(len(target_sets(*shape))):
        for eps in EPS:
            check_case(shape, regime, which, eps, 0.0, True)


@pytest.mark.parametrize("gamma", [0.5, 2.0])
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("shape", CE_SHAPES)
def test_focal_cross_entropy(shape, regime, gamma):
    """The focal factor (1 - p)^gamma through exp2 / log2 (0.5) and through the product (2), with unit and with drawn weights.
    At one class p = 1: the loss is 0 and so is every gradient."""
    for which in range(len(target_sets(*shape))):
        for eps in EPS:
            for weighted in (False, True):
                check_case(shape, regime, which, eps, gamma, weighted)


@pytest.mark.parametrize("shape", [s for s in CE_SHAPES if s[1] > 1])
def test_minus_infinity_off_the_target_without_smoothing(shape):
    """eps = 0, gamma = 2 and one -inf logit per row at a class that is not the target (the construction of test_head_gpu's
    test_ce_minus_infinity_off_the_target_without_smoothing): that class has q = 0, its term is 0 and not 0 * inf."""
    N, J = shape
    lg = ce_logits(shape, "normal").clone()
    for ti, tg in enumerate(hard_targets(N, J)):
        hole = (tg + 1 + torch.arange(N) % (J - 1)) % J          # 1 .. J - 1 classes behind the target: never the target
        assert not bool((hole == tg).any())
        lh = lg.clone()
        lh[torch.arange(N), hole] = -INF
        for w in (None, class_weights(J)):
            want, dwant = W.loss_and_grad(lh, tg, w, 0.0, 2.0)
            assert bool(torch.isfinite(want)) and bool(torch.isfinite(dwant).all()), "the reference itself"
            loss, dl = K.ce_loss_w(dev(lh), dev(tg), 0.0, 2.0, None if w is None else dev(w), 1.0, True)
            what = f"wce {shape} -inf targets {ti} weights={w is not None}"
            assert bool(torch.isfinite(loss).item()) and bool(torch.isfinite(dl).all()), f"{what}: loss {float(loss)!r}"
            measured(loss.reshape(1), want.reshape(1), 1e-5, f"{what}: loss")
            measured(dl, dwant, 2e-4, f"{what}: dlogits")
            at = dl.cpu()[torch.arange(N), hole]
            assert int(torch.count_nonzero(at)) == 0 and int(torch.count_nonzero(dwant[torch.arange(N), hole])) == 0


@pytest.mark.parametrize("gamma", [0.0, 2.0])
@pytest.mark.parametrize("shape", [(7, 3), (257, 2), (300, 257)])
def test_scaling_the_weights(shape, gamma):
    """Every weight times 4, a power of two, so that every product and sum scales without rounding.  Index targets: the
    denominator scales with the rows and nothing changes, bit for bit.  Probability targets: the denominator is N, so the loss and
    dlogits are 4 times what they were, exactly."""
    N, J = shape
    lgd = dev(ce_logits(shape, "normal"))
    w = class_weights(J)
    for name, tg in target_sets(N, J):
        tgd = dev(tg)
        for eps in EPS:
            loss1, dl1 = K.ce_loss_w(lgd, tgd, eps, gamma, dev(w), 0.25, True)
            loss4, dl4 = K.ce_loss_w(lgd, tgd, eps, gamma, dev(w * 4), 0.25, True)
            assert bool(torch.isfinite(loss1)) and int(torch.count_nonzero(dl1)) > 0
            factor = 4.0 if tg.is_floating_point() else 1.0
            what = f"wce {shape} {name} eps={eps} gamma={gamma}: weights times 4"
            same_bits(loss4.reshape(1), (loss1 * factor).reshape(1), f"{what}, loss")
            same_bits(dl4, dl1 * factor, f"{what}, dlogits")


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("shape", CE_SHAPES)
def test_unit_weights_without_focusing_agree_with_the_plain_kernels(shape, regime):
    """No weights (NULL) and a vector of ones, gamma = 0: what dfd_ce_loss / dfd_ce_loss_soft compute, within the tolerances both
    are held to against float64.  (Not the same bits: the new kernel sums the exponentials beside the maximum on their own.)"""
    N, J = shape
    lgd = dev(ce_logits(shape, regime))
    ones = torch.ones(J, device="cuda")
    for name, tg in target_sets(N, J):
        tgd = dev(tg)
        plain = K.ce_loss_soft if tg.is_floating_point() else K.ce_loss
        for eps in EPS:
            want, dwant = plain(lgd, tgd, eps, 0.25, True)
            for wd in (None, ones):
                loss, dl = K.ce_loss_w(lgd, tgd, eps, 0.0, wd, 0.25, True)
                what = f"wce {shape} {regime} {name} eps={eps} ones={wd is not None} against the plain kernel"
                measured(loss.reshape(1), want.reshape(1), 1e-5, f"{what}: loss")
                measured(dl, dwant, 2e-4, f"{what}: dlogits")


@pytest.mark.parametrize("shape", [(257, 2), (300, 257)])
def test_two_calls_give_the_same_bits_inside_nan_filled_buffers(shape):
    """No atomics: a second call repeats the first bit for bit.  row_loss and dlogits are interior slices of NaN-filled buffers:
    every element inside is overwritten (nothing stays NaN), nothing outside is."""
    N, J = shape
    lgd, wd = dev(ce_logits(shape, "normal")), dev(class_weights(J))
    pad = 64
    for name, tg in target_sets(N, J):
        tgd = dev(tg)
        runs = []
        for _ in range(2):
            rows_buf = torch.full((N + 2 * pad,), float("nan"), device="cuda")
            dl_buf = torch.full((N * J + 2 * pad,), float("nan"), device="cuda")
            rows, dl = rows_buf[pad: pad + N], dl_buf[pad: pad + N * J].view(N, J)
            loss, got = K.ce_loss_w(lgd, tgd, 0.1, 2.0, wd, 1.0, True, row_loss=rows, dlogits=dl)
            assert got is dl
            assert bool(torch.isfinite(rows).all()) and bool(torch.isfinite(dl).all()) and bool(torch.isfinite(loss)), name
            for buf, n in ((rows_buf, N), (dl_buf, N * J)):
                assert bool(torch.isnan(buf[:pad]).all()) and bool(torch.isnan(buf[pad + n:]).all()), f"{name}: a write outside the slice"
            runs.append((loss.clone(), rows.clone(), dl.clone()))
        for a, b, what in zip(runs[0], runs[1], ("loss", "row_loss", "dlogits")):
            same_bits(a.reshape(-1), b.reshape(-1), f"wce {shape} {name}: {what} of two calls")
        # the rows are what the loss sums: index targets divide by the targets' weights, probability targets by N
        D = float(N) if tg.is_floating_point() else float(class_weights(J).double()[tg].sum())
        measured(runs[0][0].reshape(1), (runs[0][1].double().sum() / D).reshape(1), 1e-5, f"wce {shape} {name}: loss against its rows")


@pytest.mark.parametrize("gamma", [0.0, 2.0])
def test_targets_without_weight_give_nan_like_torch(gamma):
    """Index targets that all name classes of weight 0: torch's mean is 0 / 0.  Both sides are NaN and nothing else is compared;
    probability targets divide by N and stay finite under the same weights."""
    N, J = 7, 3
    lg = ce_logits((N, J), "normal")
    tg = torch.tensor([0, 1, 0, 0, 1, 1, 0])
    w = torch.tensor([0.0, 0.0, 1.5])
    assert math.isnan(float(torch.nn.functional.cross_entropy(lg.double(), tg, weight=w.double(), label_smoothing=0.1)))
    assert math.isnan(float(W.loss(lg.double(), tg, w, 0.1, gamma)))
    for want_grad in (False, True):
        loss, _ = K.ce_loss_w(dev(lg), dev(tg), 0.1, gamma, dev(w), 1.0, want_grad)
        assert math.isnan(float(loss)), float(loss)
    soft = soft_targets(N, J, 0)
    want, dwant = W.loss_and_grad(lg, soft, w, 0.1, gamma)
    loss, dl = K.ce_loss_w(dev(lg), dev(soft), 0.1, gamma, dev(w), 1.0, True)
    measured(loss.reshape(1), want.reshape(1), 1e-5, f"wce gamma={gamma} two weightless classes, probability targets: loss")
    measured(dl, dwant, 2e-4, f"wce gamma={gamma} two weightless classes, probability targets: dlogits")


def test_front_end_refuses_misshapen_arguments():
    lg, tg = torch.zeros(4, 3, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")
    for bad in (lambda: K.ce_loss_w(lg, tg, 0.1, -1.0), lambda: K.ce_loss_w(lg, tg, 1.0, 0.0), lambda: K.ce_loss_w(lg, tg[:3], 0.1, 0.0),
                lambda: K.ce_loss_w(lg, tg, 0.1, 0.0, torch.ones(2, device="cuda")), lambda: K.ce_loss_w(lg, lg[:, :2].contiguous(), 0.1, 0.0),
                lambda: K.ce_loss_w(lg, tg, 0.1, 0.0, None, 1.0, True, dlogits=torch.zeros(4, 2, device="cuda"))):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------------------------------ the module
def _spy(monkeypatch, name: str) -> list:
    calls = []
    real = getattr(K, name)
    monkeypatch.setattr(K, name, lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def test_plain_module_keeps_the_plain_kernel_bit_for_bit(monkeypatch):
    from deepfakedetection_amd.optim import HipCrossEntropyLoss

    g = torch.Generator().manual_seed(6)
    logits = (torch.randn(64, 10, generator=g) * 2).cuda()
    y = torch.randint(0, 10, (64,), generator=g).cuda()
    want_loss, want_d = K.ce_loss(logits, y, 0.1, 1.0, True)
    calls = _spy(monkeypatch, "ce_loss_w")
    ld = logits.clone().requires_grad_(True)
    loss = HipCrossEntropyLoss(0.1)(ld, y)
    loss.backward()
    assert not calls
    same_bits(loss.reshape(1), want_loss.reshape(1), "module loss")
    same_bits(ld.grad, want_d, "module gradient")
    probs = torch.softmax(torch.randn(64, 10, generator=g), 1).cuda()
    soft_loss = HipCrossEntropyLoss(0.1, weight=None, focal_gamma=0.0)(ld, probs)
    assert not calls
    same_bits(soft_loss.reshape(1), K.ce_loss_soft(logits, probs, 0.1, 1.0, False)[0].reshape(1), "module loss, probability targets")


@pytest.mark.parametrize("gamma", [0.0, 2.0])
def test_weighted_module_backward_and_probability_targets(monkeypatch, gamma):
    """Through autograd from a leaf: d (3 * loss) / d logits against the reference, with class indices and with Mixup's rows."""
    from deepfakedetection_amd.mix import BatchMixer
    from deepfakedetection_amd.optim import HipCrossEntropyLoss

    g = torch.Generator().manual_seed(9)
    N, J = 32, 2
    logits = torch.randn(N, J, generator=g) * 2
    y = torch.randint(0, J, (N,), generator=g)
    w = torch.tensor([2.5, 0.625])
    crit = HipCrossEntropyLoss(0.1, weight=w.tolist(), focal_gamma=gamma)
    assert crit.weight.device.type == "cpu"
    crit = crit.cuda()
    where = crit.weight.data_ptr()
    calls = _spy(monkeypatch, "ce_loss_w")
    torch.manual_seed(4)
    _, mixed = BatchMixer(0.8, 0.0, mode="elem", num_classes=J)(torch.randn(N, 3, 8, 8).cuda(), y.cuda())
    assert mixed.dtype == torch.float32 and mixed.shape == (N, J) and float((mixed - mixed.round()).abs().max()) > 0.01
    for name, tg in (("indices", y), ("mixed rows", mixed.cpu())):
        ld = logits.cuda().requires_grad_(True)
        loss = crit(ld, tg.cuda())
        (loss * 3.0).backward()
        want, dwant = W.loss_and_grad(logits, tg, w, 0.1, gamma)
        measured(loss.reshape(1), want.reshape(1), 1e-5, f"weighted module gamma={gamma} {name}: loss")
        measured(ld.grad, dwant * 3.0, 2e-4, f"weighted module gamma={gamma} {name}: gradient")
    assert len(calls) == 2 and crit.weight.data_ptr() == where
    with pytest.raises(ValueError, match="class weights"):
        crit(torch.zeros(4, 3, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda"))
    lazy = HipCrossEntropyLoss(0.1, weight=w.tolist())          # nobody moved it: the buffer follows the logits at its first use
    same_bits(lazy(logits.cuda(), y.cuda()).reshape(1), HipCrossEntropyLoss(0.1, weight=w.tolist()).cuda()(logits.cuda(), y.cuda()).reshape(1),
              "a criterion moved at its first use")
    assert lazy.weight.is_cuda


# ------------------------------------------------------------------------------------------------------------------ the captured step
def test_graphed_step_with_weights_and_focusing_is_bitwise_the_eager_step():
    """EfficientNet-B0, batch 8 at 64 x 64, weight = [2.5, 0.625] and gamma = 2 (the pattern of tests/test_train_gpu.py's
    test_graphed_step_is_bitwise_the_eager_step): three optimizer steps leave bit-identical parameters and statistics.  The weights
    are a buffer at a fixed address, so `criterion.weight.copy_(new)` reaches the next replay: its loss is the eager loss under
    the new weights, and not the loss under the old ones."""
    from deepfakedetection_amd.efficientnet import HipEfficientNet
    from deepfakedetection_amd.graph_step import GraphedTrainStep
    from deepfakedetection_amd.optim import HipAdamW, HipCrossEntropyLoss

    g = torch.Generator().manual_seed(3)
    batches = [(torch.randn(8, 3, 64, 64, generator=g).cuda(), torch.randint(0, 2, (8,), generator=g).cuda()) for _ in range(4)]
    assert all(0 < int(y.sum()) < 8 for _, y in batches)

    def run(graph: bool, swap: bool):
        torch.manual_seed(11)
        model = HipEfficientNet("b0", "timm", 2).cuda().train()
        opt = HipAdamW(model.parameters(), lr=1e-3, weight_decay=5e-2)
        crit = HipCrossEntropyLoss(0.1, weight=[2.5, 0.625], focal_gamma=2.0).cuda()
        step = GraphedTrainStep(model, crit, opt, accum_steps=1)
        if not graph:
            step.failed = True                                  # the object's own eager path
        losses = []
        for x, y in batches[:3]:
            losses.append(step.micro_batch(x, y, first=True, last=True).clone())
            step.optimizer_step()
        torch.cuda.synchronize()
        state = {k: v.clone() for k, v in model.state_dict().items()}
        if swap:
            crit.weight.copy_(torch.tensor([0.625, 2.5]))
        after = step.micro_batch(*batches[3], first=True, last=True).clone()
        torch.cuda.synchronize()
        return state, torch.stack(losses).cpu(), after.cpu(), step

    s_e, l_e, a_e, step_e = run(False, True)
    s_g, l_g, a_g, step_g = run(True, True)
    _, _, a_old, _ = run(False, False)
    assert step_e.replays == 0
    assert not step_g.failed and step_g.replays == 3, step_g.replays        # step 1 eager (first sight), then every micro-batch replayed
    assert torch.equal(l_e, l_g), (l_e, l_g)
    for name in s_e:
        assert torch.equal(s_e[name], s_g[name]), name
    print(f"[wloss] replayed loss under the new weights {float(a_g):.6f}, eager {float(a_e):.6f}, under the old weights {float(a_old):.6f}")
    assert torch.equal(a_e, a_g) and not torch.equal(a_old, a_g)


# ------------------------------------------------------------------------------------------------------------------ the trainer
def _folder(root: Path, counts: dict, size: int) -> None:
    rng = np.random.default_rng(0)
    for split, per_class in counts.items():
        for ci, (name, n) in enumerate(per_class.items()):
            (root / split / name).mkdir(parents=True)
            for i in range(n):
                arr = (rng.random((size, size + 8, 3)) * 255).astype(np.uint8)
                arr[..., ci % 3] //= 2
                Image.fromarray(arr).save(root / split / name / f"{i}.png")


@pytest.mark.parametrize("model_name,on", [("efficientnet_b0", True), ("efficientnet_b0", False), ("efficientformerv2_s0", True)])
def test_orchestrated_training_with_class_weights_focusing_and_balanced_sampling(tmp_path, monkeypatch, model_name, on):
    """training.class_weights: balanced + focal_gamma: 2 + balanced_sampling on a 12 + 4 picture folder (the pattern of
    tests/test_mix_gpu.py's trainer test): the training criterion carries n / (J n_j) = (0.6667, 2.0) and gamma 2, the evaluation
    criterion carries neither, dfd_ce_loss_w runs and the training loaders draw balanced epochs.  With the three keys absent none
    of that happens: one plain criterion serves both, K.ce_loss_w is never called and the loaders shuffle uniformly."""
    from deepfakedetection_amd.dp import BalancedShardedSampler
    from deepfakedetection_amd.optim import HipCrossEntropyLoss
    from deepfakedetection_amd.orchestration.orchestrator import orchestrate
    from deepfakedetection_amd.trainers import _engine as mod

    monkeypatch.chdir(tmp_path)
    for var in ("CLASS_WEIGHTS", "FOCAL_GAMMA", "BALANCED_SAMPLING"):
        monkeypatch.delenv(var, raising=False)
    img = 64
    _folder(tmp_path / "data", {"train": {"fake": 12, "real": 4}, "val": {"fake": 4, "real": 4}}, img + 8)
    calls = _spy(monkeypatch, "ce_loss_w")
    made, used, samplers, evals = [], [], [], []
    real_make, real_epoch, real_eval = mod._make_criterion_and_optimizer, mod.train_one_epoch, mod.evaluate

    def make(use_cuda, *a, **k):
        crit, make_opt = real_make(use_cuda, *a, **k)
        made.append((crit, bool(a or k)))
        crit.register_forward_hook(lambda m, args, out: used.append((m, torch.is_grad_enabled(), out.detach())))
        return crit, make_opt

    def spy_epoch(model, dl, opt, scaler, criterion, *a, **k):
        samplers.append((dl.sampler, criterion))
        return real_epoch(model, dl, opt, scaler, criterion, *a, **k)

    def rising_eval(model, *a, **k):                             # every evaluation a little better: a deterministic best epoch
        res = real_eval(model, *a, **k)
        evals.append((a[3] if len(a) > 3 else k.get("criterion"), res))
        return dataclasses.replace(res, acc=0.1 * len(evals))

    monkeypatch.setattr(mod, "_make_criterion_and_optimizer", make)
    monkeypatch.setattr(mod, "train_one_epoch", spy_epoch)
    monkeypatch.setattr(mod, "evaluate", rising_eval)
    training = {"epochs": 1, "batch_size": 8, "ft_batch_size": 8, "accum_steps": 1, "num_workers": 0, "resume": "auto",
                "pretrained": False, "img_size": img}
    if on:
        training.update(class_weights="balanced", focal_gamma=2, balanced_sampling=True)
    base = {"seed": 1, "device": "cuda", "data": {"root": str(tmp_path / "data"), "train_split": "train", "val_split": "val",
                                                  "test_split": "val", "num_classes": 2, "img_size": img}}
    path = tmp_path / "runs.yaml"
    path.write_text(yaml.safe_dump({**base, "models": {model_name: {"output_dir": str(tmp_path / "runs" / model_name), "training": training}}}))
    orchestrate(path, mode="training")

    reports_loss = model_name.startswith("efficientnet")
    assert len(samplers) == 2                                    # warm-up and one fine-tune epoch
    train_crits = {id(c) for _, c in samplers}
    assert len(train_crits) == 1
    train_crit = samplers[0][1]
    assert isinstance(train_crit, HipCrossEntropyLoss) and train_crit.label_smoothing == 0.1
    train_losses = torch.stack([out.float().cpu() for m, grad, out in used if grad])
    assert len(train_losses) >= 4 and bool(torch.isfinite(train_losses).all()), train_losses       # 16 draws / 8 per phase
    assert all(m is train_crit for m, grad, _ in used if grad)
    eval_crits = [c for c, _ in evals]
    assert len(evals) == 2 and all((c is not None) == reports_loss for c in eval_crits)
    if on:
        assert [float(v) for v in train_crit.weight.cpu()] == pytest.approx([16 / 24, 2.0], rel=1e-6) and train_crit.focal_gamma == 2.0
        assert train_crit.weight.is_cuda and len(calls) >= 4
        assert all(isinstance(s, BalancedShardedSampler) for s, _ in samplers)
        assert [flag for _, flag in made] == [True] + [False] * reports_loss     # the training criterion, then the plain one for val_loss
        for c in eval_crits:
            if reports_loss:
                assert isinstance(c, HipCrossEntropyLoss) and c is not train_crit
                assert c.weight is None and c.focal_gamma == 0.0 and c.label_smoothing == 0.1
        assert all(m is not train_crit for m, grad, _ in used if not grad)
    else:
        assert train_crit.weight is None and train_crit.focal_gamma == 0.0
        assert not calls and [flag for _, flag in made] == [False]
        assert not any(isinstance(s, BalancedShardedSampler) for s, _ in samplers)
        assert all(c is train_crit for c in eval_crits if c is not None)
    if reports_loss:
        assert all(res.loss is not None and math.isfinite(res.loss) for _, res in evals)
    run = sorted((tmp_path / "runs" / model_name).iterdir())[0]
    ckpt = torch.load(run / "checkpoints" / "latest.ckpt", map_location="cpu")
    assert ckpt["epoch"] == 1 and all(bool(torch.isfinite(v).all()) for v in ckpt["model"].values() if v.is_floating_point())
    banner = (run / "logs" / "train.log").read_text() if (run / "logs" / "train.log").is_file() else ""
    if banner:
        assert ("focal_gamma=2" in banner) == on
