"""Cost of gradient clipping (HipAdamW max_grad_norm) in the replayed training step at a training batch's size.

    python scripts/bench_clip.py [--models efficientnet_b0,efficientformerv2_s1,faster_vit_0_224] [--batch 256] [--size 224]
                                 [--limit 1.0] [--mode norm|value] [--steps 20] [--opt-replays 200] [--rounds 5]
                                 [--variants off,on] [--tag TEXT] [--out FILE]

Per model, one GraphedTrainStep with clipping off and one with it on (their own model instances, same seed), both warmed up
until the step graphs replay.  Then `--rounds` rounds, the variants alternating inside a round, each timing

  step_ms      `--steps` full replayed steps (prepare_step + forward/backward graph + optimizer-step graph), host clock around
               work that ends in a device synchronise;
  opt_step_us  `--opt-replays` replays of the optimizer-step graph alone (AdamW, with clipping the sum of squares and the
               finish in front of it), device events.

One JSON line per (model, variant): the median over the rounds and the spread (min, max) the rounds themselves show, so that
a difference can be held against the run-to-run noise of the same code on the same box.  The `on` line also carries the
difference to `off` in microseconds and in per cent of the step.  `--variants off` runs on a tree without the feature too
(for the comparison with the commit before it); `--out` appends the lines to a file (profiles/clip_step.jsonl).
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path
from time import perf_counter

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch  # noqa: E402


def build_variant(name: str, clip: bool, args):
    from deepfakedetection_amd.graph_step import GraphedTrainStep
    from deepfakedetection_amd.optim import HipAdamW, HipCrossEntropyLoss
    from deepfakedetection_amd.orchestration.model_registry import get_model_spec

    torch.manual_seed(0)
    model = get_model_spec(name).builder(name, 2).cuda().train()
    model.to(memory_format=torch.channels_last)
    extra = {"max_grad_norm": args.limit, "clip_mode": args.mode} if clip else {}
    opt = HipAdamW(model.parameters(), lr=1e-5, weight_decay=5e-2, **extra)
    step = GraphedTrainStep(model, HipCrossEntropyLoss(0.1), opt, accum_steps=1)
    return model, opt, step


def one_step(step, x, y) -> None:
    step.micro_batch(x, y, first=True, last=True)
    step.optimizer_step()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="efficientnet_b0,efficientformerv2_s1,faster_vit_0_224")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--limit", type=float, default=1.0)
    ap.add_argument("--mode", default="norm", choices=("norm", "value"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--opt-replays", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--variants", default="off,on")
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_clip.py measures on the GPU only")
    variants = [v for v in args.variants.split(",") if v]
    assert variants and set(variants) <= {"off", "on"}, variants
    lines = []
    for name in args.models.split(","):
        g = torch.Generator().manual_seed(1)
        x = torch.randn(args.batch, 3, args.size, args.size, generator=g).cuda().contiguous(memory_format=torch.channels_last)
        y = torch.randint(0, 2, (args.batch,), generator=g).cuda()
        built = {v: build_variant(name, v == "on", args) for v in variants}
        for _, _, step in built.values():
            for _ in range(5):                                  # eager cycle, capture, replays
                one_step(step, x, y)
            torch.cuda.synchronize()
            if step.failed or step.step_graph is None:
                raise SystemExit(f"{name}: the training step did not capture; nothing to measure")
        times = {v: {"step_ms": [], "opt_step_us": []} for v in variants}
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(args.rounds):
            for v in variants:
                _, opt, step = built[v]
                one_step(step, x, y)
                torch.cuda.synchronize()
                t0 = perf_counter()
                for _ in range(args.steps):
                    one_step(step, x, y)
                torch.cuda.synchronize()
                times[v]["step_ms"].append(1e3 * (perf_counter() - t0) / args.steps)
                step.step_graph.replay()
                start.record()
                for _ in range(args.opt_replays):
                    step.step_graph.replay()
                stop.record()
                torch.cuda.synchronize()
                times[v]["opt_step_us"].append(1e3 * start.elapsed_time(stop) / args.opt_replays)
        params = sum(p.numel() for p in built[variants[0]][0].parameters())
        for v in variants:
            _, opt, _ = built[v]
            rec = {"model": name, "clip": v, "batch": args.batch, "size": args.size, "rounds": args.rounds,
                   "steps_per_round": args.steps, "opt_replays_per_round": args.opt_replays, "gradient_bytes": 4 * params}
            if args.tag:
                rec["tag"] = args.tag
            if v == "on":
                rec.update(limit=args.limit, mode=args.mode)
                stats = opt.clip_stats()
                rec.update(grad_norm_mean=stats["grad_norm_mean"], skipped_steps=stats["skipped_steps"])
            for key, vals in times[v].items():
                digits = 4 if key == "step_ms" else 2
                rec[key] = round(statistics.median(vals), digits)
                rec[key + "_min"], rec[key + "_max"] = round(min(vals), digits), round(max(vals), digits)
            if v == "on" and "off" in times:
                off = times["off"]
                d_opt = statistics.median(times["on"]["opt_step_us"]) - statistics.median(off["opt_step_us"])
                d_step = 1e3 * (statistics.median(times["on"]["step_ms"]) - statistics.median(off["step_ms"]))
                rec.update(opt_step_extra_us=round(d_opt, 2), step_extra_us=round(d_step, 1),
                           opt_step_extra_pct_of_step=round(100.0 * d_opt / (1e3 * statistics.median(off["step_ms"])), 3))
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
        del built
        torch.cuda.empty_cache()
    if args.out:
        path = Path(args.out)
        path.parent.mkdir(parents=True, exist_ok=True)
        with path.open("a", encoding="utf-8") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
