"""BASELINE.json configs[0] — the reference's CPU-runnable plumbing case: the whole
registry / YAML / env-var / trainer / checkpoint / inference surface end to end on CPU with
a tiny generated ImageFolder.  The HIP engine cannot (and must not) run on CPU, so the
model is a plug-in stub registered through the public registry hook; everything around it
is the product code.
"""

from __future__ import annotations

import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml
from PIL import Image
from torch import nn

from deepfakedetection_amd.orchestration import model_registry as reg
from deepfakedetection_amd.orchestration.orchestrator import orchestrate


class TinyNet(nn.Module):
    """Stand-in classifier with the head naming the trainers' freeze mask looks for."""

    def __init__(self, num_classes: int) -> None:
        super().__init__()
        self.conv_stem = nn.Conv2d(3, 8, 3, stride=2, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(8)
        self.classifier = nn.Linear(8, num_classes)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.classifier(torch.relu(self.bn1(self.conv_stem(x))).mean((2, 3)))


def _make_dataset(root: Path, classes=("cat", "dog", "eel"), per_class=6, size=40) -> None:
    rng = np.random.default_rng(0)
    for split in ("train", "val", "test"):
        for ci, name in enumerate(classes):
            folder = root / split / name
            folder.mkdir(parents=True)
            for i in range(per_class):
                arr = (rng.random((size, size + 8, 3)) * 255).astype(np.uint8)
                arr[..., ci % 3] //= 2
                mode_l = (i == 0)
                Image.fromarray(arr[..., 0] if mode_l else arr).save(folder / f"{i}.png")   # one grayscale: ensure_rgb path


@pytest.fixture()
def workspace(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    _make_dataset(tmp_path / "data")
    reg.register_model_spec(reg.ModelSpec("tinynet_stub", "deepfakedetection_amd.trainers.efficientnet", "tinynet_stub", 32,
                                          lambda _name, nc: TinyNet(nc)))
    return tmp_path


def _config(tmp_path: Path, **model_block) -> Path:
    cfg = {
        "seed": 1, "device": "cpu",
        "data": {"root": str(tmp_path / "data"), "train_split": "train", "val_split": "val", "test_split": "test",
                 "num_classes": 3, "img_size": 32},
        "models": {"tinynet_stub": {"output_dir": str(tmp_path / "runs" / "tiny"), **model_block}},
        "selection": ["tinynet_stub"],
    }
    path = tmp_path / "cfg.yaml"
    path.write_text(yaml.safe_dump(cfg))
    return path


def test_training_then_inference_end_to_end(workspace):
    tmp = workspace
    cfg = _config(tmp, training={"epochs": 2, "batch_size": 6, "num_workers": 0, "resume": "auto", "accum_steps": 2,
                                 "ft_batch_size": 4, "pretrained": False},
                  transforms={"train": {"train_random_resized_crop": False, "train_center_crop": True, "train_random_rotation": True,
                                        "train_color_jitter": True, "train_random_erasing": True},
                              "eval": {"val_resize": True}})
    orchestrate(cfg, mode="training")
    runs = sorted((tmp / "runs" / "tiny").iterdir())
    assert len(runs) == 1
    run = runs[0]
    for rel in ("checkpoints/latest.ckpt", "checkpoints/best.ckpt", "EfficientNetModel.pth", "logs/train.log", "config_snapshot.yaml"):
        assert (run / rel).exists(), rel
    ckpt = torch.load(run / "checkpoints" / "latest.ckpt")
    assert ckpt["epoch"] == 2 and ckpt["warmup_done"] is True and "optimizer" in ckpt and "scheduler" in ckpt
    assert set(torch.load(run / "EfficientNetModel.pth")) == set(TinyNet(3).state_dict())
    log = (run / "logs" / "train.log").read_text()
    assert "Warmup (head only)" in log and "Fine-tune" in log and "val_acc=" in log and "img/s" not in log.split("Data")[0]
    snap = yaml.safe_load((run / "config_snapshot.yaml").read_text())
    assert snap["model"]["name"] == "tinynet_stub" and snap["global"]["seed"] == 1

    weights = run / "EfficientNetModel.pth"
    cfg2 = _config(tmp, inference={"weights": str(weights), "split": "test", "batch_size": 5, "num_workers": 0, "img_size": 32})
    orchestrate(cfg2, mode="inference")
    run2 = sorted((tmp / "runs" / "tiny").iterdir())[-1]
    rows = [json.loads(line) for line in (run2 / "logs" / "metrics.jsonl").read_text().splitlines()]
    assert rows[0]["model"] == "tinynet_stub" and rows[0]["split"] == "test" and 0.0 <= rows[0]["accuracy"] <= 1.0
    assert np.array(rows[0]["confusion_matrix"]).sum() == 18
    assert (run2 / "logs" / "inference.log").exists()


class TinyHeadNet(nn.Module):
    """Stub with the names the EfficientFormerV2 / FasterViT freeze masks look for (`head`, `stages.3`)."""

    def __init__(self, num_classes: int) -> None:
        super().__init__()
        self.stem = nn.Conv2d(3, 8, 3, stride=2, padding=1)
        self.stages = nn.Sequential(*[nn.Conv2d(8, 8, 1) for _ in range(4)])
        self.norm = nn.BatchNorm2d(8)
        self.head = nn.Linear(8, num_classes)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.head(self.norm(torch.relu(self.stages(self.stem(x)))).mean((2, 3)))


@pytest.mark.parametrize("trainer,weights,img_arg", [("efficientformer_v2", "EfficientFormerV2_S1.pth", True),
                                                     ("fastervit", "FasterVitModel.pth", False)])
def test_other_two_trainers_end_to_end_on_cpu(workspace, trainer, weights, img_arg):
    """trainers/efficientformer_v2.py and trainers/fastervit.py counterparts (shared engine) through the orchestrator:
    warm-up on the head, the reference's fine-tune subsets, file names, throughput.jsonl."""
    built = {}

    def builder(_name, nc, img_size=None):
        built["img_size"] = img_size
        return TinyHeadNet(nc)

    if not img_arg:
        two_arg = builder
        builder = lambda name, nc: two_arg(name, nc)  # noqa: E731  (FasterViT's builder takes no img_size)
    name = f"stub_{trainer}"
    reg.register_model_spec(reg.ModelSpec(name, f"deepfakedetection_amd.trainers.{trainer}", name, 32, builder))
    cfg = yaml.safe_load(_config(workspace, training={"epochs": 1, "batch_size": 6, "num_workers": 0, "pretrained": False}).read_text())
    cfg["models"] = {name: {**cfg["models"]["tinynet_stub"], "output_dir": str(workspace / "runs" / name)}}
    cfg["selection"] = [name]
    path = workspace / f"{trainer}.yaml"
    path.write_text(yaml.safe_dump(cfg))
    orchestrate(path, mode="training")
    run = sorted((workspace / "runs" / name).iterdir())[0]
    ckpt = torch.load(run / "checkpoints" / "latest.ckpt")
    assert ckpt["epoch"] == 1 and ckpt["warmup_done"] is True
    log = (run / "logs" / "train.log").read_text()
    assert "Warmup (head only)" in log and "val_acc=" in log
    rows = [json.loads(line) for line in (run / "logs" / "throughput.jsonl").read_text().splitlines()]
    assert [r["phase"] for r in rows] == ["warmup", "fine-tune"] and rows[0]["images"] == 18
    n_state = len(ckpt["optimizer"]["state"])
    if trainer == "efficientformer_v2":
        assert built["img_size"] == 32                        # timm.create_model(..., img_size=img_size) in the reference
        assert n_state == 4                                   # stages.3.{weight,bias} + head.{weight,bias}
        assert "Fine-tune" not in log                         # BATCH_SIZE batches, no accumulation
    else:
        assert n_state == len(list(TinyHeadNet(3).parameters())) and rows[1]["batch_size"] == 32 and rows[1]["accum_steps"] == 4
        assert "Fine-tune" in log and "accum_steps=4" in log
    assert (run / "checkpoints" / "best.ckpt").exists() == (run / weights).exists()


_STUBS = {"efficientnet": lambda _name, nc: TinyNet(nc), "efficientformer_v2": lambda _name, nc, img_size=None: TinyHeadNet(nc),
          "fastervit": lambda _name, nc: TinyHeadNet(nc)}
_NUM, _ACC, _LR = r"\d+\.\d{4}", r"\d\.\d{4}", r"\d\.\d{2}e[-+]\d{2}"
# what may follow a console record in train.log: the head of another one (nothing else belongs to the record before it)
_NEXT = r"(?= (?:Fine-tune:|epoch \d+ |new best |Early stopping|warmup \| loss=|train \| loss=|Best weights saved))"


def _train_stub(workspace: Path, trainer: str, **training) -> str:
    """Seeded CPU training of trainers/<trainer>.py on its stub; the whitespace-normalised logs/train.log (rich wraps long
    lines at the log's width)."""
    name = f"stub_{trainer}"
    reg.register_model_spec(reg.ModelSpec(name, f"deepfakedetection_amd.trainers.{trainer}", name, 32, _STUBS[trainer]))
    cfg = yaml.safe_load(_config(workspace, training={"batch_size": 6, "num_workers": 0, "pretrained": False, **training}).read_text())
    cfg["models"] = {name: {**cfg["models"]["tinynet_stub"], "output_dir": str(workspace / "runs" / name)}}
    cfg["selection"] = [name]
    path = workspace / f"{trainer}.yaml"
    path.write_text(yaml.safe_dump(cfg))
    orchestrate(path, mode="training")
    run = sorted((workspace / "runs" / name).iterdir())[0]
    return " ".join((run / "logs" / "train.log").read_text().split())


def _records(log: str, pattern: str) -> list[str]:
    """Console records of `log` that match `pattern` as a whole: from the start of a word to the head of the next record."""
    return re.findall(r"(?<![^ ])" + pattern + _NEXT, log)


@pytest.mark.parametrize("trainer", ["efficientnet", "efficientformer_v2", "fastervit"])
def test_console_lines_per_trainer(workspace, trainer):
    """The warm-up, fine-tune and epoch lines of each trainer keep the reference's shapes through the one engine."""
    log = _train_stub(workspace, trainer, epochs=2)
    counts = r" \(\d+/18\)"
    if trainer == "efficientnet":
        warm = rf"warmup \| val_acc={_ACC} \| val_loss={_NUM}{counts}"
        epoch = rf"epoch \d \| train_loss={_NUM} \| val_loss={_NUM} \| val_acc={_ACC}{counts} \| lr={_LR}"
    elif trainer == "efficientformer_v2":
        warm, epoch = rf"warmup \| val_acc={_ACC}", rf"epoch \d \| val_acc={_ACC}"
    else:
        warm, epoch = rf"warmup \| val_acc={_ACC}", rf"epoch \d \| val_acc={_ACC}{counts} \| lr={_LR}"
    assert len(_records(log, warm)) == 1, log
    assert len(_records(log, epoch)) == 2, log
    if trainer == "efficientformer_v2":
        assert "Fine-tune" not in log
    else:
        assert "Fine-tune: bs=32, accum_steps=4 (effective ≈ 128)" in log


def test_specs_carry_the_reference_constants():
    """One table over the three SPECs; and trainers/efficientnet.py owns no loop: its main / evaluate / train_one_epoch are
    the engine's."""
    import inspect

    from deepfakedetection_amd.trainers import _engine, efficientformer_v2, efficientnet, fastervit

    unfreeze = ("stages.3", "blocks.3", "layer4", "bneck", "features.6", "classifier", "head")
    #        warm-up keys            fine-tune   ft batch, accum, from env   early  zg1st  img    weights file               epochs  batch
    table = {
        efficientnet: (("_fc", "classifier"), None, (32, 4, True), True, False, False, "EfficientNetModel.pth", 25, 64),
        efficientformer_v2: (("classifier", "head"), unfreeze, (None, 1, False), False, True, True, "EfficientFormerV2_S1.pth", 5, 128),
        fastervit: (("head",), None, (32, 4, False), True, False, False, "FasterVitModel.pth", 25, 64),
    }
    for mod, (warm, ft, (ft_bs, ft_accum, ft_env), early, zg_first, img, weights, epochs, batch) in table.items():
        s = mod.SPEC
        assert isinstance(s, _engine.TrainerSpec)
        assert (s.warmup_keys, s.unfreeze_keys) == (warm, ft), mod.__name__
        assert (s.ft_batch_size, s.ft_accum_steps, s.ft_from_env) == (ft_bs, ft_accum, ft_env), mod.__name__
        assert (s.early_stop, s.zero_grad_first, s.pass_img_size) == (early, zg_first, img), mod.__name__
        assert (s.best_weights_name, s.default_epochs, s.default_batch_size) == (weights, epochs, batch), mod.__name__
        assert s.report_loss == (mod is efficientnet) and (s.transform_kwargs is None) == (mod is efficientnet)
        assert mod.evaluate is _engine.evaluate and mod.train_one_epoch is _engine.train_one_epoch
        source = inspect.getsource(mod)
        assert "def train_one_epoch" not in source and "def evaluate" not in source and "device_batches(" not in source
        assert inspect.getsource(mod.main).split(":", 1)[1].strip() == "run(SPEC)" and mod.run is _engine.run


class _StubEma:
    """What run() touches on an ema.ModelEma, for CPU modules (the product's EMA is a HIP kernel and refuses them)."""

    def __init__(self, model: nn.Module, build, device: str, settings) -> None:
        self.model, self.module, self.decay, self.updates = model, build().to(device), settings.decay, 0
        self.module.load_state_dict(model.state_dict())
        for p in self.module.parameters():
            p.requires_grad = False

    def step(self) -> None:
        self.updates += 1
        with torch.no_grad():
            for shadow, p in zip(self.module.parameters(), self.model.parameters()):
                shadow.lerp_(p, 1.0 - self.decay)


@pytest.mark.parametrize("trainer", ["efficientnet", "fastervit"])
def test_ema_console_line_per_trainer(workspace, monkeypatch, trainer):
    from deepfakedetection_amd.trainers import _engine

    monkeypatch.setattr(_engine, "make_model_ema", _StubEma)
    log = _train_stub(workspace, trainer, epochs=1, ema_decay=0.9)
    val_loss = rf"val_loss={_NUM} \| " if trainer == "efficientnet" else ""
    assert len(_records(log, rf"epoch 1 EMA \| {val_loss}val_acc={_ACC} \(\d+/18\) \| updates=\d+")) == 1, log
    assert ("EMA | val_loss=" in log) == (trainer == "efficientnet")


def test_reference_train_yaml_fails_loudly_for_the_engine_that_is_not_built(workspace):
    """config/train.yaml of the reference selects all three models.  A registered model without a HIP engine must
    stop with the registry's message — not with ModuleNotFoundError from a dangling trainer path (round-1 review)."""
    import importlib

    for key in ("efficientnet_b3", "efficientformerv2_s1", "faster_vit_2_224"):
        spec = reg.get_model_spec(key)
        assert hasattr(importlib.import_module(spec.train_module), "main")
    cfg = yaml.safe_load(_config(workspace, training={"epochs": 1, "batch_size": 6, "num_workers": 0, "pretrained": False}).read_text())
    # every model of the reference's YAMLs now has an engine; a name under a registered prefix without one still
    # stops with the registry's message
    name = "faster_vit_4_21k_224"
    cfg["models"] = {name: dict(cfg["models"]["tinynet_stub"])}
    cfg["selection"] = [name]
    path = workspace / "fv.yaml"
    path.write_text(yaml.safe_dump(cfg))
    with pytest.raises(NotImplementedError, match="registered but its MI355X engine is not built"):
        orchestrate(path, mode="training")
    for key, cls in (("faster_vit_2_224", "HipFasterViT"), ("faster_vit_0_224", "HipFasterViT"), ("efficientformerv2_s1", "HipEfficientFormerV2")):
        assert type(reg.get_model_spec(key).builder(key, 2)).__name__ == cls


def test_class_count_mismatch_exits(workspace):
    cfg = yaml.safe_load(_config(workspace, training={"epochs": 1, "batch_size": 4, "num_workers": 0}).read_text())
    cfg["data"]["num_classes"] = 2
    path = workspace / "bad.yaml"
    path.write_text(yaml.safe_dump(cfg))
    with pytest.raises(SystemExit) as err:
        orchestrate(path, mode="training")
    assert err.value.code == 1


def test_missing_dataset_exits(workspace):
    cfg = yaml.safe_load(_config(workspace, training={"epochs": 1, "batch_size": 4, "num_workers": 0}).read_text())
    cfg["data"]["root"] = str(workspace / "nowhere")
    path = workspace / "bad2.yaml"
    path.write_text(yaml.safe_dump(cfg))
    with pytest.raises(SystemExit):
        orchestrate(path, mode="training")


def test_hip_model_refuses_cpu_input():
    """The product model has no CPU path: a CPU tensor raises instead of falling back."""
    model = reg.get_model_spec("efficientnet_b0").builder("efficientnet_b0", 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model(torch.zeros(1, 3, 32, 32))


def test_gpu_input_tail_sampler_and_uint8_pipeline():
    """Host side of the GPU input tail: the train/val pipelines end in uint8 HWC tensors, the tail samples
    flips and erase boxes with RandomErasing's rules (box strictly inside the image, height 0 = none)."""
    import torch
    from PIL import Image

    from deepfakedetection_amd import data as D
    from deepfakedetection_amd.trainers.efficientnet import build_transforms

    train_t, val_t, train_tail, val_tail = build_transforms(96, gpu_tail=True)
    img = Image.fromarray((torch.rand(120, 100, 3) * 255).to(torch.uint8).numpy())
    for t in (train_t, val_t):
        out = t(img)
        assert out.dtype == torch.uint8 and tuple(out.shape) == (96, 96, 3)
    assert val_tail.flip_p == 0 and val_tail.erase_p == 0 and train_tail.flip_p == 0.5
    torch.manual_seed(0)
    tail = D.GpuInputTail([0.5] * 3, [0.25] * 3, flip_p=0.5, erase_p=0.5)
    flip, erase = tail.sample(200, 64, 48)
    assert flip.dtype == torch.uint8 and 60 <= int(flip.sum()) <= 140
    assert erase.dtype == torch.int32 and tuple(erase.shape) == (200, 4)
    on = erase[:, 2] > 0
    assert 60 <= int(on.sum()) <= 140
    e = erase[on]
    assert bool(((e[:, 0] >= 0) & (e[:, 1] >= 0) & (e[:, 0] + e[:, 2] <= 64) & (e[:, 1] + e[:, 3] <= 48)).all())
    assert bool((e[:, 2] < 64).all()) and bool((e[:, 3] < 48).all())
    area = (e[:, 2] * e[:, 3]).float() / (64 * 48)
    assert float(area.min()) > 0.01 and float(area.max()) < 0.40


def test_hip_adamw_state_dict_round_trips_into_torch_adamw():
    """HipAdamW shares ONE step counter per group internally; the checkpoint must still carry an
    independent `step` per parameter, or torch.optim.AdamW (the reference's optimizer, trainers/efficientnet.py:487-491)
    advances the shared tensor once per parameter after a resume."""
    import pickle

    import torch

    from deepfakedetection_amd.optim import HipAdamW

    params = [torch.nn.Parameter(torch.randn(3, 2)) for _ in range(5)]
    opt = HipAdamW(params, lr=1e-3)
    for _ in range(3):
        opt.prepare_step()                      # host side of a step: counters + hyper-parameters (no kernel)
    sd = pickle.loads(pickle.dumps(opt.state_dict()))
    steps = [st["step"] for st in sd["state"].values()]
    assert len(steps) == 5 and all(float(s) == 3.0 for s in steps)
    assert len({id(s) for s in steps}) == 5, "per-parameter step tensors must not alias"
    ref = torch.optim.AdamW(params, lr=1e-3)
    ref.load_state_dict(sd)
    for p in params:
        p.grad = torch.ones_like(p)
    ref.step()
    assert all(float(ref.state[p]["step"]) == 4.0 for p in params)
    # and back: HipAdamW re-shares the loaded counters
    opt2 = HipAdamW(params, lr=1e-3)
    opt2.load_state_dict(ref.state_dict())
    opt2.prepare_step()
    assert all(float(opt2.state[p]["step"]) == 5.0 for p in params)


def test_rccl_log_summary_never_raises_and_picks_the_decisions(tmp_path):
    """bench.py --gpus N records what RCCL chose (config.rccl): the summariser must cope with any log, or none."""
    from deepfakedetection_amd.dp import rccl_log_summary

    log = tmp_path / "rccl.log"
    log.write_text("h:1:1 [0] NCCL INFO RCCL version 2.22.3\nh:1:1 [0] NCCL INFO Channel 00/32 : 0 1 2 3 4 5 6 7\nnoise\n"
                   "h:1:1 [0] NCCL INFO Trees [0] 1/-1/-1->0->-1\nh:1:1 [0] NCCL INFO Channel 00/32 : 0 1 2 3 4 5 6 7\n")
    got = rccl_log_summary(str(log))
    assert got["log_lines"] == 5 and got["selected"] == ["RCCL version 2.22.3", "Channel 00/32 : 0 1 2 3 4 5 6 7", "Trees [0] 1/-1/-1->0->-1"]
    assert "note" in rccl_log_summary(str(tmp_path / "missing.log"))
    assert rccl_log_summary(None) is None


def test_default_224_training_pipeline_qualifies_for_the_device_path(monkeypatch):
    """the reference's default toggles at 224 pixels switch rotation AND colour jitter on
    (reference trainers/efficientnet.py:134-135); with training.gpu_resize the whole training pipeline must still move to the
    device (workers decode + plan only, GpuInputTail rotates / jitters), and fall back to PIL for pictures too large for the kernel."""
    from deepfakedetection_amd import data as D
    from deepfakedetection_amd.trainers.efficientnet import build_transforms

    monkeypatch.delenv("TRANSFORMS", raising=False)
    train, val, train_tail, val_tail = build_transforms(224, gpu_tail=True, gpu_resize=True)
    assert isinstance(train.ops[-1], D.PlanGeometry) and train.ops[-1].mode == "rrc"
    assert not any(isinstance(op, (D.RandomRotation, D.ColorJitter)) for op in train.ops)
    assert train_tail.augments and train_tail.rotate_degrees == 10.0 and train_tail.jitter == (0.2, 0.2, 0.2, 0.05)
    assert train_tail.flip_p == 0.5 and train_tail.erase_p == 0.5 and not val_tail.augments
    big_train, _, big_tail, _ = build_transforms(300, gpu_tail=True, gpu_resize=True)
    assert any(isinstance(op, D.RandomRotation) for op in big_train.ops) and any(isinstance(op, D.ColorJitter) for op in big_train.ops)
    assert not big_tail.augments
    # the sampler: one 16-int job per picture, rotation plan + permutation + factors inside their ranges
    import torch

    torch.manual_seed(0)
    jobs = train_tail.sample_augment(64, 224, 224)
    assert jobs.shape == (64, 16) and jobs.dtype == torch.int32
    f = jobs.view(torch.float32)
    assert set(jobs[:, 0].tolist()) <= {0, 1} and (jobs[:, 15] == 15).all()
    assert all(sorted(row) == [0, 1, 2, 3] for row in jobs[:, 7:11].tolist())
    for col in (11, 12, 13):
        assert float(f[:, col].min()) >= 0.8 and float(f[:, col].max()) <= 1.2
    dh = jobs[:, 14]
    assert ((dh <= 13) | (dh >= 243)).all()                     # |0.05 * 255| = 12.75 -> shifts of at most 13 either way, modulo 256


def test_rotate_plan_is_the_oracles():
    import numpy as np

    from deepfakedetection_amd import data as D
    from oracle import image_ref as IR

    rng = np.random.default_rng(3)
    for _ in range(200):
        w, h = int(rng.integers(1, 400)), int(rng.integers(1, 400))
        a = float(rng.uniform(-400, 400)) if rng.random() < 0.8 else float(rng.choice([0, 90, 180, 270, -90, 360, 450]))
        assert D.rotate_plan(w, h, a) == IR.rotate_plan(w, h, a)
        assert D.rotate_plan(h, h, a) == IR.rotate_plan(h, h, a)


def test_bench_plain_run_leaves_the_side_measurements_to_full():
    """bench.py: a plain run is the headline alone; --full turns on the rest, and the extra-model children ask for it."""
    import bench

    plain = bench.parse(["--gpus", "1", "--steps", "3", "--warmup", "2"])
    assert plain.full is False and (plain.steps, plain.warmup) == (3, 2)
    full = bench.parse(["--full"])
    assert full.full is True and full.eval_steps > 0 and full.profile_steps > 0 and full.extra_models
    cmd = bench.extra_model_cmd("efficientformerv2_s1", full)
    assert "--full" in cmd and cmd[cmd.index("--extra-models") + 1] == "" and cmd[cmd.index("--eval-steps") + 1] == "0"


_STAGE_LAYOUTS = [
    # (stage, layer names in the order the Function's docstring lists their weight / bias / bn.weight / bn.bias quads, index of the
    #  first quad among the tensor inputs, tensor inputs in all)
    ("ConvStemFunction", ("conv",), 0, 4),
    ("DenseConvBNFunction", ("conv",), 0, 4),
    ("ConvMlpFunction", ("fc1", "dw", "fc2"), 0, 14),                                            # ..., ls, row_scale
    ("AttentionFunction", ("q", "k", "v", "v_local", "proj"), 0, 27),                            # ..., 4 talking-head, table, ls, row_scale
    ("AttentionFunction stride 2", ("stride_conv", "q", "k", "v", "v_local", "proj"), 0, 31),
    ("DownsampleFunction", ("conv",), 0, 4),
    ("DownsampleFunction attention", ("q_proj", "k", "v", "v_local", "proj"), 6, 27),            # conv quad, q.local.weight, .bias first
    ("ConvBlockFunction", ("conv1", "conv2"), 0, 10),                                            # ..., gamma, row_scale
]
_TRIPLE_LAYOUTS = [
    # the EfficientNet stages: no convolution bias, so weight / bn.weight / bn.bias triples.  A row per run of adjacent triples
    ("StemFunction", ("conv",), 0, 3),
    ("MBConvFunction", ("expand", "dw"), 0, 14),                  # expand at 0, dw at 3, four squeeze-excite tensors at 6 ...
    ("MBConvFunction project", ("project",), 10, 14),             # ... project at 10, row_scale last
    ("HeadFunction", ("head",), 0, 5),                            # ..., classifier weight, bias
]
_ALL_LAYOUTS = [(*row, True) for row in _STAGE_LAYOUTS] + [(*row, False) for row in _TRIPLE_LAYOUTS]


@pytest.mark.parametrize("stage,names,offset,total,bias", _ALL_LAYOUTS, ids=[s[0] for s in _ALL_LAYOUTS])
def test_layer_records_are_cut_in_the_stages_input_order(stage, names, offset, total, bias):
    """cut_layers on labelled dummies: every name gets its four (without a convolution bias: three) tensors and their need flags at
    its place in the stage's input order, and Layer.grads() masks each gradient by its own flag."""
    from deepfakedetection_amd import functions as Fn
    from deepfakedetection_amd import vit_functions as V
    from deepfakedetection_amd.fastervit_functions import ConvBlockFunction  # noqa: F401  (the layouts above name it)

    assert V.cut_layers is Fn.cut_layers and V.Layer is Fn.Layer            # one record type, whichever module names it
    if "Attention" in stage:
        assert names == (V._ATT_ORDER if "stride" in stage else V._ATT_ORDER[1:])
    if stage == "DownsampleFunction attention":
        assert names == V._DS_ORDER
    width = 4 if bias else 3
    fields = ("w", "b", "gamma", "beta") if bias else ("w", "gamma", "beta")
    t = tuple(torch.tensor(float(i)) for i in range(total))
    need = tuple((i * 7 + i // 4) % 3 != 0 for i in range(total))             # no period of 3 or 4: every layer gets its own pattern
    bns = {nm: object() for nm in names}
    layers = V.cut_layers(names, t, need, offset, bns, bias=bias)
    assert tuple(layers) == tuple(names)
    for i, nm in enumerate(names):
        L, o = layers[nm], offset + width * i
        assert [float(getattr(L, f)) for f in fields] == list(range(o, o + width)), nm
        assert tuple(getattr(L, "need_" + f) for f in fields) == need[o:o + width], nm
        assert bias or (L.b is None and L.need_b is False)
        assert L.bn is bns[nm] and L.ls is None and L.need_ls is False
        assert L.need_bn == (need[o + width - 2] or need[o + width - 1])
        assert L.grads(bias) == (None,) * width                                # nothing produced yet
        L.dw, L.db, L.dgamma, L.dbeta = "dw", "db", "dgamma", "dbeta"
        assert L.grads(bias) == tuple("d" + f if flag else None for f, flag in zip(fields, need[o:o + width])), nm
    forward = V.cut_layers(names, t, None, offset, None, bias=bias)            # a forward: tensors only, every flag False
    for i, nm in enumerate(names):
        L = forward[nm]
        assert float(L.w) == offset + width * i and L.bn is None
        assert not (L.need_w or L.need_b or L.need_gamma or L.need_beta or L.need_ls or L.need_any)


def test_mbconv_layers_sit_where_the_block_passes_them():
    """functions._mb_layers on MBConvFunction's 13 tensor inputs behind x: expand, dw, project and the four squeeze-excite tensors."""
    from deepfakedetection_amd import functions as Fn

    t = tuple(torch.tensor(float(i)) for i in range(13))
    cfg = Fn.MBConvCtx(True, None, False, "bn_expand", "bn_dw", "bn_project", True)
    exp, dw, proj, se = Fn._mb_layers(t, None, cfg)
    assert [float(L.w) for L in (exp, dw, proj)] == [0, 3, 10] and [float(v) for v in se] == [6, 7, 8, 9]
    assert (exp.bn, dw.bn, proj.bn) == ("bn_expand", "bn_dw", "bn_project")


# HATFunction's tensor inputs behind (x, ct, cfg), written out by hand from its input list (fastervit_functions.hat_slots states the
# order for the code): per token stream the position table, the attention sub-block and the MLP sub-block, then the LayerScales of
# both streams, then the two DropPath row scales.  A LayerNorm is a Layer of gamma and beta alone; a Linear layer the Layer of an
# identity statistic: its bias is `beta`.
_HAT_STREAM = ("pos.tab", "attn.ln.gamma", "attn.ln.beta", "attn.qkv.w", "attn.qkv.beta", "attn.proj.w", "attn.proj.beta", "attn.bias.tab",
               "mlp.ln.gamma", "mlp.ln.beta", "mlp.fc1.w", "mlp.fc1.beta", "mlp.fc2.w", "mlp.fc2.beta")
_HAT_SCALES = ("attn.proj.ls", "mlp.fc2.ls")


def _hat_paths(carrier: bool) -> list:
    streams = ("win", "car") if carrier else ("win",)
    return [(s, p) for s in streams for p in _HAT_STREAM] + [(s, p) for s in streams for p in _HAT_SCALES]


def _hat_field(streams: dict, stream: str, path: str):
    """(record, field name) at `path` of the stream."""
    *records, field = path.split(".")
    rec = streams[stream]
    for name in records:
        rec = getattr(rec, name)
    return rec, field


@pytest.mark.parametrize("layer_scale", [True, False], ids=["layer_scale", "no_layer_scale"])
@pytest.mark.parametrize("carrier", [True, False], ids=["carrier", "plain"])
def test_hat_records_are_cut_and_flattened_in_the_blocks_input_order(carrier, layer_scale):
    """cut_hat on labelled dummies: every record field holds the input at its place and that input's need flag (None LayerScales:
    ls None, need_ls False; need=None: every flag False); hat_inputs gives the inputs back; hat_grads returns one gradient per
    tensor input, input i's where its flag is set and None elsewhere."""
    from deepfakedetection_amd import fastervit_functions as FV

    paths = _hat_paths(carrier)
    total = len(paths) + 2
    assert total == (34 if carrier else 18)
    t = [torch.full((2,), float(i)) for i in range(total)]
    if not layer_scale:
        for i, (_, p) in enumerate(paths):
            if p.endswith(".ls"):
                t[i] = None
    need = tuple((i * 7 + i // 4) % 3 != 0 and t[i] is not None for i in range(total))      # no period: every input its own pattern
    win, car, scales = FV.cut_hat(t, need, carrier)
    streams = {"win": win, "car": car}
    assert (car is not None) == carrier and scales[0] is t[-2] and scales[1] is t[-1]
    for i, (s, p) in enumerate(paths):
        rec, f = _hat_field(streams, s, p)
        assert getattr(rec, f) is t[i], (i, s, p)
        assert getattr(rec, "need_" + f) is need[i], (i, s, p)
        assert getattr(rec, "d" + f) is None
        setattr(rec, "d" + f, f"d{i}")
    for st in streams.values():
        if st is not None:
            for L in (st.attn.qkv, st.attn.proj, st.mlp.fc1, st.mlp.fc2):            # Linear layers: no convolution bias, identity statistic
                assert L.b is None and not L.need_b and not L.need_gamma and L.bn.eps == 0.0 and float(L.gamma.sum()) == 2.0
            for L in (st.attn.qkv, st.mlp.fc1):
                assert L.ls is None and L.need_ls is False
            if not layer_scale:
                assert st.attn.proj.ls is None and st.mlp.fc2.ls is None and not (st.attn.proj.need_ls or st.mlp.fc2.need_ls)
    assert all(a is b for a, b in zip(FV.hat_inputs(win, car, *scales), t)) and len(FV.hat_inputs(win, car, *scales)) == total
    grads = FV.hat_grads(win, car)
    assert len(grads) == total
    assert grads == [f"d{i}" if need[i] else None for i in range(total - 2)] + [None, None]
    fwd_win, fwd_car, _ = FV.cut_hat(t, None, carrier)                                # a forward: tensors only, every flag False
    fwd = {"win": fwd_win, "car": fwd_car}
    for i, (s, p) in enumerate(paths):
        rec, f = _hat_field(fwd, s, p)
        assert getattr(rec, f) is t[i] and getattr(rec, "need_" + f) is False


@pytest.mark.parametrize("carrier", [True, False], ids=["carrier", "plain"])
def test_hat_module_hands_its_tensors_to_the_function_in_that_order(monkeypatch, carrier):
    """HipHAT.forward with HATFunction.apply replaced by a recorder: cutting what it passed gives every record the module's own
    parameter, LayerScale and coordinate table."""
    from deepfakedetection_amd import fastervit_functions as FV
    from deepfakedetection_amd.fastervit import HipHAT

    blk = HipHAT(dim=64, heads=2, sr_ratio=2 if carrier else 1, drop_path=0.0, layer_scale=1e-5, index=0)
    seen = []
    monkeypatch.setattr(FV.HATFunction, "apply", staticmethod(lambda *a: seen.append(a) or (a[0], a[1])))
    jobs, _ = blk.coord_jobs()
    assert [j.kind for j in jobs] == ["pos", "cpb"] * (2 if carrier else 1)
    tables = [torch.full((1,), float(i)) for i in range(len(jobs))]                    # in coord_jobs' order
    x, ct = torch.zeros(4, 49, 1, 64), (torch.zeros(1, 16, 1, 64) if carrier else None)
    maps = (1, 2, 3) if carrier else None
    blk(x, ct, maps, None, tables)
    (gx, gct, cfg, *t), = seen
    assert gx is x and gct is ct and cfg.carrier == carrier and cfg.heads == 2
    assert (cfg.cat_src_ct, cfg.cat_dst_ct, cfg.cat_dst_x) == (maps if carrier else (None, None, None))
    assert len(t) == (34 if carrier else 18)
    win, car, scales = FV.cut_hat(t, None, carrier)
    assert scales == (None, None)
    assert win.pos.tab is tables[0] and win.attn.bias.tab is tables[1]
    assert win.attn.ln.gamma is blk.norm1.weight and win.attn.ln.beta is blk.norm1.bias and win.attn.ln.w is None
    assert win.attn.qkv.w is blk.attn.qkv.weight and win.attn.qkv.beta is blk.attn.qkv.bias
    assert win.attn.proj.w is blk.attn.proj.weight and win.attn.proj.beta is blk.attn.proj.bias and win.attn.proj.ls is blk.gamma3
    assert win.mlp.ln.gamma is blk.norm2.weight and win.mlp.ln.beta is blk.norm2.bias
    assert win.mlp.fc1.w is blk.mlp.fc1.weight and win.mlp.fc1.beta is blk.mlp.fc1.bias
    assert win.mlp.fc2.w is blk.mlp.fc2.weight and win.mlp.fc2.beta is blk.mlp.fc2.bias and win.mlp.fc2.ls is blk.gamma4
    if carrier:
        assert car.pos.tab is tables[2] and car.attn.bias.tab is tables[3]
        assert car.attn.ln.gamma is blk.hat_norm1.weight and car.attn.ln.beta is blk.hat_norm1.bias
        assert car.attn.qkv.w is blk.hat_attn.qkv.weight and car.attn.proj.w is blk.hat_attn.proj.weight
        assert car.attn.proj.ls is blk.gamma1 and car.mlp.fc2.ls is blk.gamma2
        assert car.mlp.ln.gamma is blk.hat_norm2.weight and car.mlp.ln.beta is blk.hat_norm2.bias
        assert car.mlp.fc1.w is blk.hat_mlp.fc1.weight and car.mlp.fc2.beta is blk.hat_mlp.fc2.bias
    else:
        assert car is None
