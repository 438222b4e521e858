"""Cost of the Gaussian-blur augmentation (data.RandomBlur / kernels.blur_u8) at a training batch's size.

    python scripts/bench_blur.py [--batch 256] [--size 224] [--sigma 3] [--replays 200] [--rounds 5] [--workers 16]
                                 [--loop-steps 40] [--parts host,kernel,tail,loop] [--tag TEXT] [--out FILE]

One JSON line per part; `--out` appends them to a file (profiles/blur_aug.jsonl).

  host     the batch's pictures through D.RandomBlur(1.0, (sigma, sigma)) in `--workers` forked processes (and in one), host
           clock; runs first, before this process opens the device, so that the fork is clean.
  kernel   dfd_blur_u8 on the same pictures, every picture at `--sigma`: `--replays` replays of a captured graph holding its one
           launch, device events, per round; and the same number of plain launches.  bytes_min is what the launch must move
           (read 3 and write 3 bytes per pixel); taps is the number of LDS byte reads of the six passes.
  tail     D.GpuInputTail (flip, rotation, colour jitter, erasing; resident uint8 batch from pinned memory) with the blur at
           p = 0.5, sigma 0..3, and without it, alternating, host clock around a call that ends in a synchronise: the draws on
           the host, the upload and every kernel of the tail.
  loop     trainers._engine.train_one_epoch for EfficientNet-B0 (replayed step, micro-batch `--batch` x 1) fed with pinned uint8
           batches through those two tails, alternating inside a round.  The tail without the blur draws and launches exactly
           what it did before the option existed, so it stands for the loop of the commit before it.
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path
from time import perf_counter

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np  # noqa: E402
import torch  # noqa: E402

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
_PICTURES = None
_SIGMA = 3.0


def _one(i: int) -> int:
    from PIL import Image

    from deepfakedetection_amd import data as D

    torch.manual_seed(i)
    out = D.RandomBlur(1.0, (_SIGMA, _SIGMA))(Image.fromarray(_PICTURES[i]))
    return out.size[0]


def spread(vals, digits=3) -> dict:
    return {"median": round(statistics.median(vals), digits), "min": round(min(vals), digits), "max": round(max(vals), digits)}


def part_host(args, rec_base) -> dict:
    import multiprocessing as mp

    n = len(_PICTURES)
    t0 = perf_counter()
    for i in range(n):
        _one(i)
    single = 1e3 * (perf_counter() - t0)
    times = []
    with mp.get_context("fork").Pool(args.workers) as pool:
        pool.map(_one, range(n), chunksize=max(1, n // (4 * args.workers)))            # warm: imports, page faults
        for _ in range(args.rounds):
            t0 = perf_counter()
            pool.map(_one, range(n), chunksize=max(1, n // (4 * args.workers)))
            times.append(1e3 * (perf_counter() - t0))
    return {**rec_base, "part": "host", "workers": args.workers, "one_process_ms_per_batch": round(single, 2),
            "one_process_us_per_picture": round(1e3 * single / n, 1), "pool_ms_per_batch": spread(times, 2)}


def part_kernel(args, rec_base) -> dict:
    from deepfakedetection_amd import data as D
    from deepfakedetection_amd import kernels as K

    n, size = args.batch, args.size
    src = torch.from_numpy(_PICTURES).cuda()
    plan = D.blur_plan(_SIGMA)
    jobs = torch.tensor([[*plan, 0]] * n, dtype=torch.int32)
    out = K.blur_u8(src, jobs)
    torch.cuda.synchronize()
    lib = K._L()
    dst = torch.empty_like(src)
    jobs_dev = jobs.cuda()

    def launch() -> None:
        code = lib.dfd_blur_u8(src.data_ptr(), jobs_dev.data_ptr(), dst.data_ptr(), n, size, size, torch.cuda.current_stream().cuda_stream)
        assert code == 0, code

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            launch()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(dst, out), "the replayed launch and the wrapper disagree"
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    replayed, plain = [], []
    for _ in range(args.rounds):
        start.record()
        for _ in range(args.replays):
            graph.replay()
        stop.record()
        torch.cuda.synchronize()
        replayed.append(1e3 * start.elapsed_time(stop) / args.replays)
        start.record()
        for _ in range(args.replays):
            launch()
        stop.record()
        torch.cuda.synchronize()
        plain.append(1e3 * start.elapsed_time(stop) / args.replays)
    bytes_min = n * size * size * 6
    taps = n * size * size * 3 * 6 * (2 * plan[0] + 3)
    us = statistics.median(replayed)
    return {**rec_base, "part": "kernel", "plan": list(plan), "replays_per_round": args.replays, "replayed_us": spread(replayed, 2),
            "plain_launch_us": spread(plain, 2), "bytes_min": bytes_min, "gb_per_s_of_bytes_min": round(bytes_min / us / 1e3, 1),
            "taps": taps, "gtaps_per_s": round(taps / us / 1e3, 1), "ns_per_picture": round(1e3 * us / n, 1)}


def _tails():
    from deepfakedetection_amd import data as D

    kw = dict(flip_p=0.5, erase_p=0.5, rotate_degrees=10.0, jitter=(0.2, 0.2, 0.2, 0.05))
    return {"off": D.GpuInputTail(MEAN, STD, **kw), "on": D.GpuInputTail(MEAN, STD, blur=(0.5, 0.0, 3.0), **kw)}


def part_tail(args, rec_base) -> dict:
    tails = _tails()
    batch = torch.from_numpy(_PICTURES).pin_memory()
    times = {v: [] for v in tails}
    torch.manual_seed(3)
    for v, tail in tails.items():
        for _ in range(3):
            tail(batch, "cuda")
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for v, tail in tails.items():
            t0 = perf_counter()
            for _ in range(10):
                tail(batch, "cuda")
            torch.cuda.synchronize()
            times[v].append(1e3 * (perf_counter() - t0) / 10)
    return {**rec_base, "part": "tail", "p": 0.5, "sigma_range": [0.0, 3.0], "calls_per_round": 10, "off_ms": spread(times["off"]),
            "on_ms": spread(times["on"]), "extra_ms": round(statistics.median(times["on"]) - statistics.median(times["off"]), 3)}


class Uint8Loader:
    """The attributes train_one_epoch touches on a DataLoader, over pre-pinned uint8 NHWC batches."""

    def __init__(self, batch: int, steps: int) -> None:
        g = torch.Generator().manual_seed(1)
        base = torch.from_numpy(_PICTURES)
        self.batches = [(base.roll(k, 0).contiguous().pin_memory(), torch.randint(0, 2, (batch,), generator=g)) for k in range(4)]
        self.batch_size, self.steps = batch, steps
        self.dataset = range(batch * steps)
        self.sampler = None

    def __len__(self) -> int:
        return self.steps

    def __iter__(self):
        for i in range(self.steps):
            yield self.batches[i % 4]


def part_loop(args, rec_base) -> dict:
    from rich.progress import Progress

    from deepfakedetection_amd.graph_step import GraphedTrainStep
    from deepfakedetection_amd.optim import HipAdamW, HipCrossEntropyLoss
    from deepfakedetection_amd.orchestration.model_registry import get_model_spec
    from deepfakedetection_amd.trainers._engine import train_one_epoch

    name = "efficientnet_b0"
    tails = _tails()
    built = {}
    for v in tails:
        torch.manual_seed(0)
        model = get_model_spec(name).builder(name, 2).cuda()
        opt = HipAdamW(model.parameters(), lr=1e-4, weight_decay=5e-2)
        crit = HipCrossEntropyLoss(0.1)
        built[v] = (model, opt, crit, GraphedTrainStep(model, crit, opt, accum_steps=1))
    scaler = torch.amp.GradScaler(enabled=False)
    rates = {v: [] for v in tails}

    def epoch(v: str, steps: int):
        model, opt, crit, stepper = built[v]
        dl = Uint8Loader(args.batch, steps)
        with Progress(disable=True) as progress:
            return train_one_epoch(model, dl, opt, scaler, crit, "cuda", use_cuda_amp=True, progress=progress,
                                   task=progress.add_task("t", total=len(dl)), accum_steps=1, stepper=stepper, tail=tails[v],
                                   with_loss=True).stats

    for v in tails:
        epoch(v, 4)
    launch = None
    for _ in range(args.rounds):
        for v in tails:
            stats = epoch(v, args.loop_steps)
            rates[v].append(stats["images_per_sec"])
            launch = stats["launch"]
    off, on = statistics.median(rates["off"]), statistics.median(rates["on"])
    return {**rec_base, "part": "loop", "model": name, "p": 0.5, "sigma_range": [0.0, 3.0], "launch": launch,
            "steps_per_round": args.loop_steps, "off_images_per_sec": spread(rates["off"], 1),
            "on_images_per_sec": spread(rates["on"], 1), "on_over_off": round(on / off, 4),
            "extra_ms_per_step": round(1e3 * args.batch * (1 / on - 1 / off), 3)}


def main() -> None:
    global _PICTURES, _SIGMA
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--sigma", type=float, default=3.0)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--loop-steps", type=int, default=40)
    ap.add_argument("--parts", default="host,kernel,tail,loop")
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    parts = [p for p in args.parts.split(",") if p]
    assert parts and set(parts) <= {"host", "kernel", "tail", "loop"}, parts
    _SIGMA = float(args.sigma)
    _PICTURES = np.random.default_rng(0).integers(0, 256, (args.batch, args.size, args.size, 3), dtype=np.uint8)   # the cost does not depend on the content
    rec_base = {"batch": args.batch, "size": args.size, "sigma": _SIGMA, "rounds": args.rounds}
    if args.tag:
        rec_base["tag"] = args.tag
    lines = []
    table = {"host": part_host, "kernel": part_kernel, "tail": part_tail, "loop": part_loop}
    for part in ("host", "kernel", "tail", "loop"):             # host first: it forks, and must do so before the device is opened
        if part not in parts:
            continue
        if part != "host" and not torch.cuda.is_available():
            raise SystemExit("bench_blur.py measures on the GPU only (--parts host runs without one)")
        lines.append(json.dumps(table[part](args, rec_base)))
        print(lines[-1], flush=True)
    if args.out:
        path = Path(args.out)
        path.parent.mkdir(parents=True, exist_ok=True)
        with path.open("a", encoding="utf-8") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
