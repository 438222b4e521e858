"""Cost of the class-weighted / focal cross entropy (dfd_ce_loss_w, ABI 147): the entry point against dfd_ce_loss, and the
replayed training step with and without `class_weights: balanced` + `focal_gamma: 2`.

    python scripts/bench_loss.py [--shapes 256x2,32x2] [--replays 500] [--model efficientnet_b0] [--batch 256] [--size 224]
                                 [--steps 20] [--rounds 5] [--skip-step] [--tag TEXT] [--out profiles/weighted_loss.jsonl]

Kernel part, per (N, J): dfd_ce_loss and three forms of dfd_ce_loss_w (weights alone; weights + gamma 2; gamma 2.5, the exp2 / log2
path) on the same logits and class indices, with the gradient, each captured in a hipGraph of its own and timed over `--replays`
replays with device events; the median of `--rounds` rounds, the variants alternating inside a round.

Step part: one GraphedTrainStep with HipCrossEntropyLoss(0.1) and one with HipCrossEntropyLoss(0.1, weight=balanced weights of a
1:4 split, focal_gamma=2) on their own model instances (same seed), `--steps` replayed steps per round by the host clock around
work that ends in a device synchronise; the median and the spread of the rounds, so that the difference can be held against the
run-to-run noise of the same code.  One JSON line per measurement; `--out` appends them to a file."""

from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path
from time import perf_counter

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch  # noqa: E402


def captured(fn) -> torch.cuda.CUDAGraph:
    """`fn` warmed up on a side stream, then captured."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph


def bench_kernels(args, lines: list) -> None:
    from deepfakedetection_amd import kernels as K

    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for shape in args.shapes.split(","):
        N, J = (int(v) for v in shape.split("x"))
        g = torch.Generator().manual_seed(1)
        logits = torch.randn(N, J, generator=g).cuda()
        y = torch.randint(0, J, (N,), generator=g).cuda()
        w = (torch.rand(J, generator=g) * 3.75 + 0.25).cuda()
        variants = {
            "ce_loss": lambda: K.ce_loss(logits, y, 0.1, 1.0, True),
            "ce_loss_w weights": lambda: K.ce_loss_w(logits, y, 0.1, 0.0, w, 1.0, True),
            "ce_loss_w weights gamma 2": lambda: K.ce_loss_w(logits, y, 0.1, 2.0, w, 1.0, True),
            "ce_loss_w gamma 2.5": lambda: K.ce_loss_w(logits, y, 0.1, 2.5, None, 1.0, True),
        }
        graphs = {name: captured(fn) for name, fn in variants.items()}
        times = {name: [] for name in variants}
        for _ in range(args.rounds):
            for name, graph in graphs.items():
                graph.replay()
                start.record()
                for _ in range(args.replays):
                    graph.replay()
                stop.record()
                torch.cuda.synchronize()
                times[name].append(1e3 * start.elapsed_time(stop) / args.replays)
        base = statistics.median(times["ce_loss"])
        for name, vals in times.items():
            rec = {"what": "kernel", "variant": name, "N": N, "J": J, "replays": args.replays, "rounds": args.rounds,
                   "replay_us": round(statistics.median(vals), 2), "replay_us_min": round(min(vals), 2),
                   "replay_us_max": round(max(vals), 2), "extra_us": round(statistics.median(vals) - base, 2)}
            if args.tag:
                rec["tag"] = args.tag
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)


def bench_step(args, lines: list) -> None:
    from deepfakedetection_amd.graph_step import GraphedTrainStep
    from deepfakedetection_amd.optim import HipAdamW, HipCrossEntropyLoss
    from deepfakedetection_amd.orchestration.model_registry import get_model_spec
    from deepfakedetection_amd.trainers._engine import balanced_class_weights

    g = torch.Generator().manual_seed(1)
    x = torch.randn(args.batch, 3, args.size, args.size, generator=g).cuda().contiguous(memory_format=torch.channels_last)
    y = (torch.rand(args.batch, generator=g) < 0.8).long().cuda()            # a 1:4 split
    weights = balanced_class_weights((1, 4))

    def build(on: bool):
        torch.manual_seed(0)
        model = get_model_spec(args.model).builder(args.model, 2).cuda().train()
        model.to(memory_format=torch.channels_last)
        opt = HipAdamW(model.parameters(), lr=1e-5, weight_decay=5e-2)
        crit = HipCrossEntropyLoss(0.1, weight=weights, focal_gamma=2.0).cuda() if on else HipCrossEntropyLoss(0.1)
        return GraphedTrainStep(model, crit, opt, accum_steps=1)

    def one_step(step) -> None:
        step.micro_batch(x, y, first=True, last=True)
        step.optimizer_step()

    built = {"off": build(False), "on": build(True)}
    for step in built.values():
        for _ in range(5):                                      # eager cycle, capture, replays
            one_step(step)
        torch.cuda.synchronize()
        if step.failed or step.step_graph is None:
            raise SystemExit(f"{args.model}: the training step did not capture; nothing to measure")
    times = {v: [] for v in built}
    for _ in range(args.rounds):
        for v, step in built.items():
            one_step(step)
            torch.cuda.synchronize()
            t0 = perf_counter()
            for _ in range(args.steps):
                one_step(step)
            torch.cuda.synchronize()
            times[v].append(1e3 * (perf_counter() - t0) / args.steps)
    for v, vals in times.items():
        rec = {"what": "step", "model": args.model, "weighted_focal": v, "batch": args.batch, "size": args.size,
               "rounds": args.rounds, "steps_per_round": args.steps, "step_ms": round(statistics.median(vals), 4),
               "step_ms_min": round(min(vals), 4), "step_ms_max": round(max(vals), 4)}
        if v == "on":
            rec.update(class_weights=[round(w, 4) for w in weights], focal_gamma=2.0,
                       step_extra_us=round(1e3 * (statistics.median(vals) - statistics.median(times["off"])), 1))
        if args.tag:
            rec["tag"] = args.tag
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x2,32x2")
    ap.add_argument("--replays", type=int, default=500)
    ap.add_argument("--model", default="efficientnet_b0")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_loss.py measures on the GPU only")
    lines: list = []
    bench_kernels(args, lines)
    if not args.skip_step:
        bench_step(args, lines)
    if args.out:
        path = Path(args.out)
        path.parent.mkdir(parents=True, exist_ok=True)
        with path.open("a", encoding="utf-8") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
