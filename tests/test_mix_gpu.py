"""Mixup / CutMix on the MI355X: dfd_mix_batch against the CPU restatement bit for bit, dfd_ce_loss_soft against torch's
cross entropy with probability targets in float64, the untouched integer-target path, one mixed f32 training step of B0
against the oracle, the mixer in front of the replayed training-step graph, and the orchestrated train -> inference path
with `mixup_alpha` / `cutmix_alpha`, on and off."""

from __future__ import annotations

import dataclasses
import json
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

from deepfakedetection_amd import kernels as K
from deepfakedetection_amd.mix import BatchMixer
from tests import _mix_ref as R
from tests.test_model_gpu import assert_grads_match, make_pair, oracle_batch, ref_backward, rel_err
from tests.test_ops_gpu import close
from tests.test_plumbing_cpu import _make_dataset

pytestmark = pytest.mark.gpu


def _bits(a: torch.Tensor) -> np.ndarray:
    return np.ascontiguousarray(a.detach().cpu().contiguous().numpy()).view(np.uint8)


def _device_batch(x: torch.Tensor, layout: str, shift: int = 0) -> torch.Tensor:
    """`x` (CPU, NCHW) on the device in the memory layout asked for, `shift` floats off 16-byte alignment."""
    N, C, H, W = x.shape
    store = torch.empty(x.numel() + shift, dtype=torch.float32, device="cuda")
    if layout == "nhwc":
        view = store[shift:].view(N, H, W, C).permute(0, 3, 1, 2)
        assert view.is_contiguous(memory_format=torch.channels_last)
    else:
        view = store[shift:].view(N, C, H, W)
    view.copy_(x.cuda())
    assert view.data_ptr() % 16 == 4 * shift
    return view


def _job_tables(N: int, H: int, W: int) -> list[list[list[int]]]:
    """Job tables for a batch of N: all three modes; boxes that are empty, one pixel wide or high, touching each border and
    the whole picture; pairs whose two jobs differ (mixup against cutmix, two different overlapping boxes)."""
    whole, empty = (0, H, 0, W), (5, 5, 3, 3)
    thin, flat = (3, H - 4, 7, 8), (H // 2, H // 2 + 1, 0, W)                 # one pixel wide / one pixel high
    tl, br = (0, H // 3, 0, W // 2), (H // 2, H, W // 3, W)                  # top + left borders / bottom + right borders
    left, right = (2, H - 2, 0, 5), (1, H - 1, W - 5, W)
    box = lambda b: R.job(R.CUTMIX, 1 - (b[1] - b[0]) * (b[3] - b[2]) / (H * W), b)      # noqa: E731
    if N == 2:
        return [[box(tl), box(br)],                                         # two different boxes that overlap
                [R.job(R.MIXUP, 0.3), box(thin)],
                [R.job(R.KEEP), R.job(R.KEEP)]]
    if N == 7:
        return [[R.job(R.MIXUP, 0.25), box(left), R.job(R.KEEP), R.job(R.KEEP), box(flat), R.job(R.MIXUP, 0.9), box(whole)],
                [box(right), box(empty), box(tl), R.job(R.KEEP), box(tl), R.job(R.KEEP), box(right)]]
    assert N == 8
    return [[R.job(R.MIXUP, 0.3), box(whole), box(empty), box(thin), R.job(R.KEEP), box(tl), box(br), R.job(R.MIXUP, 0.8)],
            [box(br)] * 8,                                                   # batch mode: every pair swaps one box
            [R.job(R.MIXUP, 0.5)] * 8,
            [box(left), box(right), box(flat), R.job(R.MIXUP, 1e-3), box(tl), box(left), box(right), box(left)]]


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("H,W", [(37, 29), (20, 24)])        # 3 * 37 * 29 is odd: partners differ in alignment (float by float)
@pytest.mark.parametrize("N", [2, 7, 8])
@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
def test_mix_kernel_equals_the_cpu_restatement_bit_for_bit(layout, N, H, W, shift):
    g = torch.Generator().manual_seed(100 * N + H)
    J = 3
    for t, jobs in enumerate(_job_tables(N, H, W)):
        x = torch.randn(N, 3, H, W, generator=g) * 3.0
        labels = torch.randint(0, J, (N,), generator=g)
        if t % 2 == 0:
            labels[N - 1] = labels[0]                        # equal labels in a pair: the two shares add up
        else:
            labels[N - 1] = (labels[0] + 1) % J
        table = R.table(jobs)
        want_x, want_y = R.ref_mix(x, labels, table, J)
        xd = _device_batch(x, layout, shift)
        y = K.mix_batch(xd, labels.cuda(), table, J)
        torch.cuda.synchronize()
        assert y.dtype == torch.float32 and tuple(y.shape) == (N, J)
        assert np.array_equal(_bits(y), _bits(want_y)), (t, y.cpu(), want_y)
        got = xd.cpu().contiguous()
        diff = (got.view(torch.int32) != want_x.view(torch.int32)).nonzero()
        assert diff.numel() == 0, (t, len(diff), diff[:8].tolist())


def test_mix_kernel_at_full_size_in_elem_mode():
    """N = 256 at 224 x 224, channels_last, a table from BatchMixer's elem mode with both kinds of job and some keeps."""
    N, H, W, J = 256, 224, 224, 2
    torch.manual_seed(17)
    table = BatchMixer(0.8, 1.0, prob=0.9, mode="elem", num_classes=J).sample(N, H, W)
    assert set(table[:, 0].tolist()) == {R.KEEP, R.MIXUP, R.CUTMIX}
    g = torch.Generator().manual_seed(4)
    x = torch.randn(N, 3, H, W, generator=g)
    labels = torch.randint(0, J, (N,), generator=g)
    want_x, want_y = R.ref_mix(x, labels, table, J)
    xd = x.cuda().contiguous(memory_format=torch.channels_last)
    y = K.mix_batch(xd, labels.cuda(), table.pin_memory(), J)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(y), _bits(want_y))
    assert torch.equal(xd.cpu().contiguous().view(torch.int32), want_x.view(torch.int32))


def test_mix_wrapper_checks():
    x = torch.zeros(4, 3, 8, 8, device="cuda")
    labels = torch.zeros(4, dtype=torch.int64)
    ok = R.table([R.job(R.KEEP)] * 4)
    with pytest.raises(ValueError, match="leaves the"):
        K.mix_batch(x, labels.cuda(), R.table([R.job(R.CUTMIX, 0.5, (0, 9, 0, 8))] * 4), 2)
    with pytest.raises(ValueError, match="label"):
        K.mix_batch(x, torch.tensor([0, 1, 2, 0]), ok, 2)                     # host labels are checked
    with pytest.raises(ValueError):
        K.mix_batch(x.half(), labels.cuda(), ok, 2)
    with pytest.raises(ValueError):
        K.mix_batch(x[:, :, ::2], labels.cuda(), R.table([R.job(R.KEEP)] * 4), 2)       # not dense
    y = K.mix_batch(x, labels, ok, 2)                                         # host labels are uploaded
    assert y.cpu().tolist() == [[1.0, 0.0]] * 4


def test_batch_mixer_on_the_device_follows_its_table():
    mixer = BatchMixer(0.8, 1.0, mode="pair", num_classes=2)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(8, 3, 37, 29, generator=g)
    labels = torch.randint(0, 2, (8,), generator=g)
    torch.manual_seed(3)
    table = mixer.sample(8, 37, 29)
    want_x, want_y = R.ref_mix(x, labels, table, 2)
    torch.manual_seed(3)
    xd = x.cuda().contiguous(memory_format=torch.channels_last)
    out, y = mixer(xd, labels.cuda())
    assert out is xd and y.dtype == torch.float32 and tuple(y.shape) == (8, 2)
    assert torch.equal(y.cpu(), want_y) and torch.equal(xd.cpu().contiguous(), want_x)
    keep = BatchMixer(0.8, 1.0, prob=0.0, num_classes=2)
    before = xd.clone()
    _, y = keep(xd, labels.cuda())                           # a batch that drew `keep` still returns dense targets
    assert torch.equal(xd, before) and torch.equal(y.cpu(), torch.nn.functional.one_hot(labels, 2).float())


# ------------------------------------------------------------------ the loss
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("N", [1, 32, 256])
@pytest.mark.parametrize("J", [2, 10, 1000])
def test_soft_cross_entropy_against_torch_in_float64(J, N, eps):
    """Tolerance: `close` of tests/test_ops_gpu.py at 1e-5, the project's figure for the hard-label loss and the softmax."""
    g = torch.Generator().manual_seed(1000 * J + N)
    logits = torch.randn(N, J, generator=g) * 3.0
    probs = torch.softmax(torch.randn(N, J, generator=g) * 2.0, 1)
    probs[0] *= 0.6                                         # a row that does not sum to one
    if N > 2:
        probs[2] = torch.nn.functional.one_hot(torch.tensor(1), J).float()
    ref = logits.double().requires_grad_(True)
    want = torch.nn.functional.cross_entropy(ref, probs.double(), label_smoothing=eps)
    want.backward()
    loss, dlogits = K.ce_loss_soft(logits.cuda(), probs.cuda(), eps, 1.0, True)
    print(f"[soft ce] J={J} N={N} eps={eps}: loss err {abs(float(loss) - float(want.detach())) / max(abs(float(want.detach())), 1e-6):.3e}, "
          f"dlogits err {float((dlogits.cpu().double() - ref.grad).abs().max()) / max(float(ref.grad.abs().max()), 1e-6):.3e}")
    close(loss.reshape(1), want.detach().reshape(1), 1e-5, "soft ce loss")
    close(dlogits, ref.grad, 1e-5, "soft ce dlogits")
    loss2, none = K.ce_loss_soft(logits.cuda(), probs.cuda(), eps, 1.0, False)
    assert none is None and torch.equal(loss2, loss)
    _, scaled = K.ce_loss_soft(logits.cuda(), probs.cuda(), eps, 0.5, True)
    close(scaled, 0.5 * ref.grad, 1e-5, "soft ce dlogits, grad_scale 0.5")


def test_loss_module_dispatches_on_the_target_type():
    from deepfakedetection_amd.optim import HipCrossEntropyLoss

    g = torch.Generator().manual_seed(2)
    crit = HipCrossEntropyLoss(0.1)
    logits = torch.randn(32, 10, generator=g)
    probs = torch.softmax(torch.randn(32, 10, generator=g), 1)
    ld = logits.cuda().requires_grad_(True)
    loss = crit(ld, probs.cuda())
    (loss * 3.0).backward()
    ref = logits.double().requires_grad_(True)
    want = torch.nn.functional.cross_entropy(ref, probs.double(), label_smoothing=0.1)
    (want * 3.0).backward()
    close(loss.reshape(1), want.detach().reshape(1), 1e-5, "module loss")
    close(ld.grad, ref.grad, 1e-5, "module grad")
    with pytest.raises(ValueError, match="shape"):
        crit(ld, probs.cuda()[:, :5])
    with pytest.raises(ValueError, match="shape"):
        crit(ld, probs.cuda()[:, 0].contiguous())


def test_integer_targets_keep_the_hard_label_kernel_bit_for_bit(monkeypatch):
    from deepfakedetection_amd.optim import HipCrossEntropyLoss

    g = torch.Generator().manual_seed(6)
    logits = (torch.randn(64, 10, generator=g) * 2).cuda()
    y = torch.randint(0, 10, (64,), generator=g).cuda()
    want_loss, want_d = K.ce_loss(logits, y, 0.1, 1.0, True)
    soft_calls = []
    real = K.ce_loss_soft
    monkeypatch.setattr(K, "ce_loss_soft", lambda *a, **k: (soft_calls.append(1), real(*a, **k))[1])
    ld = logits.clone().requires_grad_(True)
    loss = HipCrossEntropyLoss(0.1)(ld, y)
    loss.backward()
    assert not soft_calls
    assert np.array_equal(_bits(loss), _bits(want_loss)) and np.array_equal(_bits(ld.grad), _bits(want_d))


# ------------------------------------------------------------------ the training step
def test_mixed_train_step_f32_against_the_oracle():
    """test_train_step_f32's first case (B0, timm flavour, 96 x 96, N = 8) with the batch mixed on the device in elem mode, both
    kinds of job in it, against the oracle fed the CPU-mixed pictures and F.cross_entropy on the CPU-mixed targets.  Same
    bounds: logits 1e-3, loss 1e-4, gradients through assert_grads_match."""
    from deepfakedetection_amd.optim import HipCrossEntropyLoss

    ref, hip = make_pair("b0", "timm", 2)
    ref.train(); hip.train()
    N, size = 8, 96
    x, labels, masks, u = oracle_batch(ref, "timm", N, size, seed=2)
    labels[0], labels[7] = 0, 1                              # a pair with different labels: a wrong partner shows in the targets
    torch.manual_seed(8)
    mixer = BatchMixer(0.8, 1.0, mode="elem", num_classes=2)
    table = mixer.sample(N, size, size)
    modes = table[:, 0].tolist()
    assert R.MIXUP in modes and R.CUTMIX in modes, modes
    assert any(modes[i] != modes[N - 1 - i] for i in range(N // 2)), modes
    x_mixed, y_mixed = R.ref_mix(x, labels, table, 2)
    assert not torch.equal(x_mixed, x) and float((y_mixed - y_mixed.round()).abs().max()) > 0.01
    ref_logits, ref_loss = ref_backward(ref, (x_mixed, y_mixed, masks, u))

    torch.manual_seed(8)                                     # the mixer draws the same table again
    xd = x.cuda().to(memory_format=torch.channels_last)
    xd, yd = mixer(xd, labels.cuda())
    assert torch.equal(yd.cpu(), y_mixed)
    logits = hip(xd, [None if m is None else m.cuda() for m in masks], u.cuda())
    loss = HipCrossEntropyLoss(0.1)(logits, yd)
    loss.backward()
    print(f"[mixed step] logits rel {rel_err(logits, ref_logits):.3e}, loss {float(loss.detach()):.6f} vs {float(ref_loss):.6f}")
    assert rel_err(logits, ref_logits) <= 1e-3
    assert abs(float(loss) - float(ref_loss)) <= 1e-4 * max(1.0, abs(float(ref_loss)))
    assert_grads_match(hip, {n: p.grad for n, p in ref.named_parameters()}, "b0 timm mixed")


def _b0(seed: int):
    from deepfakedetection_amd.efficientnet import HipEfficientNet

    torch.manual_seed(seed)
    return HipEfficientNet("b0", "timm", 2).cuda()


@pytest.mark.parametrize("accum", [1, 2])
def test_graph_replay_behind_the_mixer_equals_eager(accum):
    """The mixer runs outside the captured step; its dense float targets travel through GraphedTrainStep's static buffers."""
    from deepfakedetection_amd.graph_step import GraphedTrainStep
    from deepfakedetection_amd.optim import HipAdamW, HipCrossEntropyLoss

    cycles = 3
    g = torch.Generator().manual_seed(3)
    batches = [(torch.randn(16, 3, 64, 64, generator=g), torch.randint(0, 2, (16,), generator=g)) for _ in range(accum * cycles)]

    def run(graph: bool):
        model = _b0(11).train()
        opt = HipAdamW(model.parameters(), lr=1e-3, weight_decay=5e-2)
        step = GraphedTrainStep(model, HipCrossEntropyLoss(0.1), opt, accum_steps=accum)
        if not graph:
            step.failed = True
        mixer = BatchMixer(0.8, 1.0, mode="elem", num_classes=2)
        torch.manual_seed(21)                                # the same tables in both runs
        targets = []
        for i, (x, y) in enumerate(batches):
            xd, yd = mixer(x.cuda().contiguous(memory_format=torch.channels_last), y.cuda())
            targets.append(yd.cpu())
            step.micro_batch(xd, yd, first=i % accum == 0, last=(i + 1) % accum == 0)
            if (i + 1) % accum == 0:
                step.optimizer_step()
        torch.cuda.synchronize()
        return model, step, targets

    m_e, step_e, t_e = run(False)
    m_g, step_g, t_g = run(True)
    assert step_e.replays == 0
    assert not step_g.failed and step_g.replays > 0 and step_g.replays == (cycles - 1) * accum, step_g.replays
    assert all(torch.equal(a, b) for a, b in zip(t_e, t_g))
    assert any(float((t - t.round()).abs().max()) > 0.01 for t in t_g), "no batch was mixed"
    for (name, a), (_, b) in zip(m_e.state_dict().items(), m_g.state_dict().items()):
        assert torch.equal(a, b), name


# ------------------------------------------------------------------ the orchestrated path
def _spies(monkeypatch):
    """Counts of K.mix_batch / K.ce_loss_soft calls, and what every criterion the trainers build receives."""
    from deepfakedetection_amd.trainers import _engine

    calls = {"mix_batch": 0, "ce_loss_soft": 0}
    for name in calls:
        real = getattr(K, name)

        def spy(*a, _real=real, _name=name, **k):
            calls[_name] += 1
            return _real(*a, **k)

        monkeypatch.setattr(K, name, spy)
    seen = []                                                # (grad enabled, target dtype, target shape, logits shape, loss)
    real_make = _engine._make_criterion_and_optimizer

    def make(use_cuda):
        crit, make_opt = real_make(use_cuda)
        crit.register_forward_hook(lambda m, args, out: seen.append(
            (torch.is_grad_enabled(), args[1].dtype, tuple(args[1].shape), tuple(args[0].shape), out.detach())))
        return crit, make_opt

    monkeypatch.setattr(_engine, "_make_criterion_and_optimizer", make)
    return calls, seen


def _train_yaml(tmp_path: Path, model_name: str, img: int, training: dict, tag: str = "runs"):
    base = {"seed": 1, "device": "cuda",
            "data": {"root": str(tmp_path / "data"), "train_split": "train", "val_split": "val", "test_split": "test",
                     "num_classes": 2, "img_size": img}}
    out_dir = str(tmp_path / tag / model_name)
    path = tmp_path / f"{tag}.yaml"
    path.write_text(yaml.safe_dump({**base, "models": {model_name: {"output_dir": out_dir, "training": training}}}))
    return base, out_dir, path


@pytest.mark.parametrize("model_name,img", [("efficientnet_b0", 64), ("efficientformerv2_s0", 64)])
def test_orchestrated_training_with_mixing_and_inference(tmp_path, monkeypatch, model_name, img):
    """training.mixup_alpha / cutmix_alpha end to end: the criterion gets float [N, J] targets while training and int64 [N]
    targets while evaluating, every training loss is finite, checkpoint and best-weights file are written and served.  (The
    accuracy on 16 random pictures decides nothing: every evaluation is reported a little better than the one before, so
    that each epoch is the best so far and the best-weights file is written deterministically.)"""
    from deepfakedetection_amd.orchestration.orchestrator import orchestrate
    from deepfakedetection_amd.trainers import _engine as mod      # where run() looks its loops up, for every trainer

    monkeypatch.chdir(tmp_path)
    vit = not model_name.startswith("efficientnet")
    real_eval = mod.evaluate
    evals = []

    def rising_eval(model, *a, **k):
        res = real_eval(model, *a, **k)
        evals.append(res.acc)
        return dataclasses.replace(res, acc=0.1 * len(evals))

    monkeypatch.setattr(mod, "evaluate", rising_eval)
    calls, seen = _spies(monkeypatch)
    epoch_losses = []
    real_epoch = mod.train_one_epoch

    def spy_epoch(*a, **k):
        assert k.get("mixer") is not None                    # warm-up and fine-tune both mix
        done = real_epoch(*a, **k)
        epoch_losses.append(done.loss)
        return done

    monkeypatch.setattr(mod, "train_one_epoch", spy_epoch)
    _make_dataset(tmp_path / "data", classes=("fake", "real"), per_class=8, size=img + 8)
    training = {"epochs": 2, "batch_size": 8, "ft_batch_size": 8, "accum_steps": 2, "num_workers": 0, "resume": "auto",
                "pretrained": False, "img_size": img, "mixup_alpha": 0.8, "cutmix_alpha": 1.0, "mix_mode": "elem"}
    base, out_dir, path = _train_yaml(tmp_path, model_name, img, training)
    orchestrate(path, mode="training")
    train_calls = [s for s in seen if s[0]]
    eval_calls = [s for s in seen if not s[0]]
    assert calls["mix_batch"] >= 6 and calls["ce_loss_soft"] >= 1, calls     # 16 images / 8: two batches per phase, three phases
    assert train_calls and all(dt == torch.float32 and shape == lshape and shape[1] == 2 for _, dt, shape, lshape, _ in train_calls)
    assert all(dt == torch.int64 and len(shape) == 1 for _, dt, shape, _, _ in eval_calls)
    if not vit:                                              # the EfficientNet trainer reports a validation loss
        assert eval_calls
        assert len(epoch_losses) == 3 and all(np.isfinite(v) for v in epoch_losses), epoch_losses
    losses = torch.stack([out.float().cpu() for *_, out in train_calls])
    assert bool(torch.isfinite(losses).all()), losses
    run = sorted(Path(out_dir).iterdir())[0]
    ckpt = torch.load(run / "checkpoints" / "latest.ckpt", map_location="cpu")
    assert ckpt["epoch"] == 2 and ckpt["best_epoch"] == 2 and len(evals) == 3
    assert all(bool(torch.isfinite(v).all()) for v in ckpt["model"].values() if v.is_floating_point())
    weights_name = "EfficientFormerV2_S1.pth" if vit else "EfficientNetModel.pth"
    assert (run / weights_name).is_file()
    infer = {**base, "models": {model_name: {"output_dir": out_dir, "inference": {
        "weights": str(run / weights_name), "split": "test", "batch_size": 16, "num_workers": 0, "img_size": img}}}}
    path2 = tmp_path / "infer.yaml"
    path2.write_text(yaml.safe_dump(infer))
    orchestrate(path2, mode="inference")
    run2 = sorted(Path(out_dir).iterdir())[-1]
    row = json.loads((run2 / "logs" / "metrics.jsonl").read_text().splitlines()[0])
    assert row["model"] == model_name and 0.0 <= row["accuracy"] <= 1.0


def test_off_means_off(tmp_path, monkeypatch):
    """No mixing key, and both alphas 0: the same weights bit for bit, and neither run launches dfd_mix_batch or
    dfd_ce_loss_soft or hands the criterion anything but int64 [N] targets."""
    from deepfakedetection_amd.orchestration.orchestrator import orchestrate

    monkeypatch.chdir(tmp_path)
    calls, seen = _spies(monkeypatch)
    _make_dataset(tmp_path / "data", classes=("fake", "real"), per_class=8, size=72)
    plain = {"epochs": 1, "batch_size": 8, "ft_batch_size": 8, "accum_steps": 2, "num_workers": 0, "resume": "auto",
             "pretrained": False, "img_size": 64}
    models = []
    for tag, extra in (("absent", {}), ("zero", {"mixup_alpha": 0.0, "cutmix_alpha": 0.0})):
        _, out_dir, path = _train_yaml(tmp_path, "efficientnet_b0", 64, {**plain, **extra}, tag=tag)
        orchestrate(path, mode="training")
        run = sorted(Path(out_dir).iterdir())[0]
        models.append(torch.load(run / "checkpoints" / "latest.ckpt", map_location="cpu")["model"])
    assert calls == {"mix_batch": 0, "ce_loss_soft": 0}
    assert seen and all(dt == torch.int64 and len(shape) == 1 for _, dt, shape, _, _ in seen)
    assert set(models[0]) == set(models[1])
    for name, a in models[0].items():
        assert torch.equal(a, models[1][name]), name
