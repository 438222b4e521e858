"""Throughput of the drop-in trainer loop (`trainers._engine.train_one_epoch`, with the EfficientNet trainer's loss sum),
eager dispatch vs hipGraph replay.

    python scripts/bench_trainer.py [--model efficientnet_b0] [--steps 60] [--ema DECAY] [--cases 32x4,256x1]
                                    [--mixup A] [--cutmix A] [--mix-mode batch|pair|elem]

Runs the real loop body on synthetic pinned batches (so the loader's H2D copy is in, PIL decode is not) at the
reference's fine-tune configuration (micro-batch 32 x 4 accumulation steps, trainers/efficientnet.py:84-86) and at
batch 256 x 1, once with GRAPH_STEP off and once on, and prints one JSON line per case.  Numbers quoted in DESIGN.md.
--ema DECAY adds the weight EMA (ema.ModelEma, one dfd_ema_update launch per optimizer step) to the loop.
--mixup A / --cutmix A add Mixup / CutMix (mix.BatchMixer, one dfd_mix_batch launch per micro-batch, probability targets).
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch  # noqa: E402
from rich.progress import Progress  # noqa: E402


class FakeLoader:
    """The attributes train_one_epoch touches on a DataLoader, over pre-pinned synthetic batches."""

    def __init__(self, batch: int, size: int, steps: int, classes: int) -> None:
        g = torch.Generator().manual_seed(1)
        self.batches = [(torch.randn(batch, 3, size, size, generator=g).pin_memory(), torch.randint(0, classes, (batch,), generator=g))
                        for _ in range(4)]
        self.batch_size, self.steps = batch, steps
        self.dataset = range(batch * steps)
        self.sampler = None

    def __len__(self) -> int:
        return self.steps

    def __iter__(self):
        for i in range(self.steps):
            yield self.batches[i % 4]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="efficientnet_b0")
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--ema", type=float, default=0.0, help="weight EMA decay (0: off)")
    ap.add_argument("--mixup", type=float, default=0.0, help="Mixup alpha (0: off)")
    ap.add_argument("--cutmix", type=float, default=0.0, help="CutMix alpha (0: off)")
    ap.add_argument("--mix-mode", default="batch", choices=("batch", "pair", "elem"))
    ap.add_argument("--cases", default="32x4,256x1", help="micro-batch x accumulation steps, comma separated")
    args = ap.parse_args()
    from deepfakedetection_amd.ema import ModelEma
    from deepfakedetection_amd.graph_step import GraphedTrainStep
    from deepfakedetection_amd.mix import BatchMixer
    from deepfakedetection_amd.optim import HipAdamW, HipCrossEntropyLoss
    from deepfakedetection_amd.orchestration.model_registry import get_model_spec
    from deepfakedetection_amd.trainers._engine import train_one_epoch

    cases = [tuple(int(v) for v in c.split("x")) for c in args.cases.split(",")]
    for batch, accum in cases:
        for graph in (False, True):
            torch.manual_seed(0)
            build = get_model_spec(args.model).builder
            model = build(args.model, 2).cuda()
            ema = ModelEma(model, build(args.model, 2).cuda(), decay=args.ema) if args.ema else None
            mixer = (BatchMixer(args.mixup, args.cutmix, mode=args.mix_mode, num_classes=2)
                     if args.mixup or args.cutmix else None)
            opt = HipAdamW(model.parameters(), lr=1e-4, weight_decay=5e-2)
            crit = HipCrossEntropyLoss(0.1)
            scaler = torch.amp.GradScaler(enabled=False)
            stepper = GraphedTrainStep(model, crit, opt, accum_steps=accum, ema=ema) if graph else None
            steps = args.steps * accum
            with Progress(disable=True) as progress:
                warm = FakeLoader(batch, args.size, 3 * accum, 2)
                train_one_epoch(model, warm, opt, scaler, crit, "cuda", use_cuda_amp=True, progress=progress,
                                task=progress.add_task("w", total=len(warm)), accum_steps=accum, stepper=stepper, ema=ema,
                                mixer=mixer, with_loss=True)
                dl = FakeLoader(batch, args.size, steps, 2)
                done = train_one_epoch(model, dl, opt, scaler, crit, "cuda", use_cuda_amp=True, progress=progress,
                                       task=progress.add_task("t", total=len(dl)), accum_steps=accum, stepper=stepper, ema=ema,
                                       mixer=mixer, with_loss=True)
            stats, loss = done.stats, done.loss
            print(json.dumps({"model": args.model, "micro_batch": batch, "accum_steps": accum, "ema": args.ema,
                              "mixup": args.mixup, "cutmix": args.cutmix,
                              "requested": "hipgraph" if graph else "eager",
                              "launch": stats["launch"], "images_per_sec": round(stats["images_per_sec"], 1),
                              "ms_per_micro_batch": round(1e3 * stats["seconds"] / steps, 3), "mean_loss": round(loss, 4)}), flush=True)
            del model, opt, stepper, ema
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
