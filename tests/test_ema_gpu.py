"""Weight EMA on the MI355X: dfd_ema_update against a numpy f32 restatement, ema.ModelEma over HipAdamW cycles, the
EMA update inside the replayed training-step graph, the shadow's graphed eval forward, the orchestrated train ->
resume -> inference path with `ema_decay`, and data parallel."""

from __future__ import annotations

import dataclasses
import datetime
import json
import os
import socket
import traceback
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import yaml

from deepfakedetection_amd import kernels as K
from deepfakedetection_amd._lib import EMA_COPY, EMA_LERP
from deepfakedetection_amd.ema import ModelEma, weight_at
from tests.test_plumbing_cpu import _make_dataset

pytestmark = pytest.mark.gpu

_F32 = np.float32


def _lerp_ref(dst: np.ndarray, src: np.ndarray, w: float) -> np.ndarray:
    """dst + w * (src - dst), three f32 roundings in this order (numpy never fuses)."""
    d = (src - dst).astype(_F32)
    t = (_F32(w) * d).astype(_F32)
    return (dst + t).astype(_F32)


def _bits(a) -> np.ndarray:
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("w", [0.0, 1.0, 2 / 11, 1e-4])
def test_kernel_is_the_numpy_f32_lerp_bit_for_bit(w):
    rng = np.random.default_rng(7)
    dev = torch.device("cuda")
    sizes = (1, 3, 4095, 4096, 4097, 1_000_003)
    rows, cases = [], []
    for shift in (0, 1):                                   # shift 1: rows one float off 16-byte alignment (scalar path)
        for n in sizes:
            s_host = (rng.standard_normal(n + shift) * rng.choice([1e-3, 1.0, 1e3])).astype(_F32)
            d_host = (rng.standard_normal(n + shift)).astype(_F32)
            s, d = torch.from_numpy(s_host).to(dev), torch.from_numpy(d_host).to(dev)
            for off in range(0, n, 4096):
                rows.append([s.data_ptr() + 4 * (shift + off), d.data_ptr() + 4 * (shift + off), min(4096, n - off), EMA_LERP])
            cases.append((s, d, s_host, d_host, shift))
    ints = []
    for n in (1, 5, 4097):                                 # integer buffers: 8-byte words copied unchanged
        src = torch.from_numpy(rng.integers(-2**62, 2**62, n)).to(dev)
        dst = torch.zeros_like(src)
        for off in range(0, n, 4096):
            rows.append([src.data_ptr() + 8 * off, dst.data_ptr() + 8 * off, min(4096, n - off), EMA_COPY])
        ints.append((src, dst))
    table = torch.tensor(rows, dtype=torch.int64, device=dev)
    wd = torch.tensor([w], dtype=torch.float32, device=dev)
    K.ema_update(table, wd)
    torch.cuda.synchronize()
    for s, d, s_host, d_host, shift in cases:
        want = d_host.copy()
        want[shift:] = _lerp_ref(d_host[shift:], s_host[shift:], w)
        assert np.array_equal(_bits(d), _bits(want)), (s.numel() - shift, shift, w)
        assert np.array_equal(_bits(s), _bits(s_host))
    for src, dst in ints:
        assert torch.equal(src, dst)


def _b0(seed: int):
    from deepfakedetection_amd.efficientnet import HipEfficientNet

    torch.manual_seed(seed)
    return HipEfficientNet("b0", "timm", 2).cuda()


def _batches(n: int, bs: int = 32, size: int = 64, seed: int = 3):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(bs, 3, size, size, generator=g).cuda(), torch.randint(0, 2, (bs,), generator=g).cuda()) for _ in range(n)]


def _snapshot(module) -> dict:
    return {k: v.detach().cpu().numpy().copy() for k, v in module.state_dict().items()}


def test_model_ema_follows_adamw_cycles_bit_for_bit():
    """Five HipAdamW cycles at accum_steps = 2 with part of the network frozen; after every cycle the shadow equals the numpy
    restatement over snapshots of the model's state dict: frozen and trainable parameters, running statistics (lerped) and
    num_batches_tracked (copied)."""
    from deepfakedetection_amd.optim import HipAdamW, HipCrossEntropyLoss

    model = _b0(1).train()
    frozen = [p for n, p in model.named_parameters() if n.startswith(("conv_stem", "bn1.", "blocks.0"))]
    assert frozen
    for p in frozen:
        p.requires_grad_(False)
    ema = ModelEma(model, _b0(2), decay=0.9999)
    assert ema.module is not model and not any(p.requires_grad for p in ema.module.parameters())
    want = _snapshot(model)
    assert all(np.array_equal(_bits(v), _bits(want[k])) for k, v in ema.module.state_dict().items())     # a copy to start
    opt = HipAdamW([p for p in model.parameters() if p.requires_grad], lr=1e-3, weight_decay=5e-2)
    crit = HipCrossEntropyLoss(0.1)
    batches = _batches(10)
    for cycle in range(5):
        opt.zero_grad(set_to_none=True)
        for x, y in batches[2 * cycle: 2 * cycle + 2]:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss = crit(model(x), y) / 2
            loss.backward()
        opt.step()
        ema.step()
        torch.cuda.synchronize()
        src = _snapshot(model)
        w = weight_at(cycle + 1, 0.9999)
        want = {k: (_lerp_ref(want[k], v, w) if v.dtype == np.float32 else v.copy()) for k, v in src.items()}
        got = ema.module.state_dict()
        for k, v in want.items():
            assert np.array_equal(_bits(got[k]), _bits(v)), (cycle, k)
    assert ema.updates == 5
    nbt = [k for k in want if k.endswith("num_batches_tracked")]
    assert nbt and int(got[nbt[0]]) == 10
    moved = [k for k in want if want[k].dtype == np.float32 and not np.array_equal(want[k], src[k])]
    assert moved, "the EMA never differed from the model"


def test_graph_replay_with_ema_equals_eager():
    """GraphedTrainStep(ema=...) captures the EMA update with AdamW; its weight changes on every replay (warm-up on), so equal
    results show that the replayed launch reads it from device memory."""
    from deepfakedetection_amd.graph_step import GraphedTrainStep
    from deepfakedetection_amd.optim import HipAdamW, HipCrossEntropyLoss

    accum, cycles = 2, 5
    batches = _batches(accum * cycles)

    def run(graph: bool):
        model = _b0(11).train()
        ema = ModelEma(model, _b0(12), decay=0.9999, warmup=True)
        opt = HipAdamW(model.parameters(), lr=1e-3, weight_decay=5e-2)
        step = GraphedTrainStep(model, HipCrossEntropyLoss(0.1), opt, accum_steps=accum, ema=ema)
        if not graph:
            step.failed = True
        for i, (x, y) in enumerate(batches):
            step.micro_batch(x, y, first=i % accum == 0, last=(i + 1) % accum == 0)
            if (i + 1) % accum == 0:
                step.optimizer_step()
        torch.cuda.synchronize()
        return model, ema, step

    m_e, ema_e, _ = run(False)
    m_g, ema_g, step = run(True)
    assert not step.failed and step.step_graph is not None and step.replays == (cycles - 1) * accum, step.replays
    assert ema_e.updates == ema_g.updates == cycles
    for (name, a), (_, b) in zip(m_e.state_dict().items(), m_g.state_dict().items()):
        assert torch.equal(a, b), name
    for (name, a), (_, b) in zip(ema_e.module.state_dict().items(), ema_g.module.state_dict().items()):
        assert torch.equal(a, b), f"EMA {name}"
    diff = [n for (n, a), (_, b) in zip(m_g.state_dict().items(), ema_g.module.state_dict().items())
            if a.is_floating_point() and not torch.equal(a, b)]
    assert diff, "the EMA equals the model"


@pytest.mark.parametrize("graph_step", ["1", "0"])
def test_shadow_eval_forward_follows_in_place_updates(monkeypatch, graph_step):
    from deepfakedetection_amd.optim import HipAdamW, HipCrossEntropyLoss
    from deepfakedetection_amd.trainers.efficientnet import eval_forward

    monkeypatch.setenv("GRAPH_STEP", graph_step)
    model = _b0(21).train()
    ema = ModelEma(model, _b0(22), decay=0.99)
    opt = HipAdamW(model.parameters(), lr=1e-2, weight_decay=5e-2)
    crit = HipCrossEntropyLoss(0.1)
    (x, _), = _batches(1, bs=8, seed=5)
    fwd = eval_forward(ema.module, "cuda")
    assert (fwd is not ema.module) == (graph_step == "1")
    for x_t, y_t in _batches(3, bs=8, seed=6):
        ema.module.eval()
        with torch.inference_mode():
            for _ in range(2):                           # first sight eager, then captured (GRAPH_STEP on)
                fwd(x)
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            crit(model(x_t), y_t).backward()
        opt.step()
        ema.step()
        with torch.inference_mode():
            got = fwd(x).clone()
        fresh = _b0(23)
        fresh.load_state_dict(ema.module.state_dict())
        fresh.eval()
        with torch.inference_mode():
            want = fresh(x)
        torch.cuda.synchronize()
        assert torch.equal(got, want)
    if graph_step == "1":
        assert fwd.replays >= 3


def _is_shadow(model) -> bool:
    return not any(p.requires_grad for p in model.parameters())


@pytest.mark.parametrize("model_name,img", [("efficientnet_b0", 64), ("efficientformerv2_s0", 64)])
def test_orchestrated_training_with_ema_resume_and_inference(tmp_path, monkeypatch, model_name, img):
    """training.ema_decay end to end: checkpoints carry model_ema / model_ema_updates, the best-weights file is the EMA
    state dict when the EMA accuracy selects the epoch (the shadow's accuracy is reported as 1.0 here so that the epoch is
    selected deterministically), inference serves it, and a resumed run restores the EMA and continues its count."""
    from deepfakedetection_amd.orchestration.orchestrator import RunPaths, orchestrate, run_training_job
    from deepfakedetection_amd.trainers import _engine as mod      # where run() looks its loops up, for every trainer

    monkeypatch.chdir(tmp_path)
    vit = not model_name.startswith("efficientnet")
    real_eval = mod.evaluate
    shadow_evals = []

    def fake_eval(model, *a, **k):
        res = real_eval(model, *a, **k)
        if _is_shadow(model):
            shadow_evals.append(res.acc)
            return dataclasses.replace(res, acc=1.0)
        return res

    monkeypatch.setattr(mod, "evaluate", fake_eval)
    restored = []
    real_restore = mod.restore_model_ema

    def spy_restore(ema, state):
        real_restore(ema, state)
        if ema is not None and state is not None:
            restored.append(({k: v.detach().cpu().clone() for k, v in ema.module.state_dict().items()}, ema.updates))

    monkeypatch.setattr(mod, "restore_model_ema", spy_restore)

    _make_dataset(tmp_path / "data", classes=("fake", "real"), per_class=8, size=img + 8)
    base = {"seed": 1, "device": "cuda",
            "data": {"root": str(tmp_path / "data"), "train_split": "train", "val_split": "val", "test_split": "test",
                     "num_classes": 2, "img_size": img}}
    out_dir = str(tmp_path / "runs" / model_name)
    training = {"epochs": 1, "batch_size": 8, "ft_batch_size": 8, "accum_steps": 2, "num_workers": 0, "resume": "auto",
                "pretrained": False, "img_size": img, "ema_decay": 0.999}
    path = tmp_path / "train.yaml"
    path.write_text(yaml.safe_dump({**base, "models": {model_name: {"output_dir": out_dir, "training": training}}}))
    orchestrate(path, mode="training")
    assert len(shadow_evals) == 1
    run = sorted(Path(out_dir).iterdir())[0]
    ckpt = torch.load(run / "checkpoints" / "latest.ckpt", map_location="cpu")
    assert ckpt["epoch"] == 1 and ckpt["best_epoch"] == 1 and ckpt["best_val_acc"] == 1.0
    updates1 = ckpt["model_ema_updates"]
    assert updates1 == (2 if vit else 1)                     # 16 images: 2 steps of 8, or 1 cycle of 2 x 8
    assert set(ckpt["model_ema"]) == set(ckpt["model"])
    assert any(not torch.equal(ckpt["model_ema"][k], ckpt["model"][k]) for k in ckpt["model"] if ckpt["model"][k].is_floating_point())
    weights_name = "EfficientFormerV2_S1.pth" if vit else "EfficientNetModel.pth"
    best = torch.load(run / weights_name, map_location="cpu")
    assert set(best) == set(ckpt["model_ema"]) and all(torch.equal(best[k], ckpt["model_ema"][k]) for k in best)
    assert "EMA" in (run / "logs" / "train.log").read_text()

    # resume from epoch 1 for epoch 2 in the same run directory
    model_cfg = {"name": model_name, "output_dir": out_dir, "training": {**training, "epochs": 2}}
    run_training_job({**base, "models": {model_name: model_cfg}}, model_cfg,
                     RunPaths(run, run / "checkpoints", run / "logs", run / "plots"))
    assert len(restored) == 1
    sd, n = restored[0]
    assert n == updates1 and all(torch.equal(sd[k], ckpt["model_ema"][k]) for k in sd)
    ckpt2 = torch.load(run / "checkpoints" / "latest.ckpt", map_location="cpu")
    assert ckpt2["epoch"] == 2 and ckpt2["model_ema_updates"] == 2 * updates1

    infer = {**base, "models": {model_name: {"output_dir": out_dir, "inference": {
        "weights": str(run / weights_name), "split": "test", "batch_size": 16, "num_workers": 0, "img_size": img}}}}
    path2 = tmp_path / "infer.yaml"
    path2.write_text(yaml.safe_dump(infer))
    orchestrate(path2, mode="inference")
    run2 = sorted(Path(out_dir).iterdir())[-1]
    row = json.loads((run2 / "logs" / "metrics.jsonl").read_text().splitlines()[0])
    assert row["model"] == model_name and 0.0 <= row["accuracy"] <= 1.0


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _dp_worker(rank: int, world: int, port: int) -> None:
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      HSA_ENABLE_IPC_MODE_LEGACY="0", GRAPH_STEP="1")
    from deepfakedetection_amd.dp import GradAllReducer, broadcast_module_state
    from deepfakedetection_amd.efficientnet import HipEfficientNet
    from deepfakedetection_amd.optim import HipAdamW, HipCrossEntropyLoss
    from deepfakedetection_amd.trainers.efficientnet import make_stepper

    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=180))
    try:
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        torch.manual_seed(10 + rank)                                 # different init: broadcast must fix it
        model = HipEfficientNet("b0", "timm", 2).to(dev).train()
        broadcast_module_state(model)
        ema = ModelEma(model, HipEfficientNet("b0", "timm", 2).to(dev), decay=0.999)
        opt = HipAdamW(model.parameters(), lr=1e-3, weight_decay=1e-2, grad_scale=1.0 / world)
        red = GradAllReducer(model.parameters(), bucket_bytes=2 << 20, arena=opt.arena)
        red.attach()
        step = make_stepper(model, HipCrossEntropyLoss(0.1), opt, accum_steps=1, use_cuda=True, world=world, reducer=red, ema=ema)
        assert step is not None and step.ema is ema
        g = torch.Generator().manual_seed(70 + rank)                 # each rank its own shard
        for _ in range(3):
            x = torch.randn(8, 3, 64, 64, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
            y = torch.randint(0, 2, (8,), generator=g).to(dev)
            step.micro_batch(x, y, first=True, last=True)
            step.optimizer_step()
        torch.cuda.synchronize()
        red.detach()
        assert ema.updates == 3 and step.step_graph is not None
        flat = torch.cat([p.detach().flatten() for p in ema.module.parameters()])
        parts = [torch.zeros_like(flat) for _ in range(world)]
        dist.all_gather(parts, flat)
        assert torch.equal(parts[0], parts[1]), "EMA parameters differ across ranks"
    except BaseException:
        traceback.print_exc()
        os._exit(1)
    dist.destroy_process_group()


def test_two_ranks_keep_equal_ema_parameters():
    mp.spawn(_dp_worker, args=(2, _free_port()), nprocs=2, join=True)
