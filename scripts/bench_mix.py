"""Kernel time of dfd_mix_batch (Mixup / CutMix of a batch in place) at a training batch's size.

    python scripts/bench_mix.py [--case mixup|cutmix|keep|elem] [--batch 256] [--size 224] [--iters 50] [--layout nhwc|nchw]

One job table for the whole run: every sample a mixup (`mixup`), every sample a cutmix with lam = 0.5 and the box in the
middle (`cutmix`), every sample kept (`keep`), or BatchMixer's elem mode with both kinds (`elem`).  The launches rotate over
four batches (4 x 154 MB at the default size, more than the 256 MiB Infinity Cache holds), so that a launch finds its
pictures in HBM like a batch the loader has just copied in.  Prints one JSON line: event-timed microseconds per launch, the
picture bytes a launch has to move and the rate.  Run it under `rocprofv3 --kernel-trace --stats` for per-launch kernel
times (profiles/r05_mix_kernel_stats.csv); numbers quoted in DESIGN.md.
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="mixup", choices=("mixup", "cutmix", "keep", "elem"))
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--layout", default="nhwc", choices=("nhwc", "nchw"))
    args = ap.parse_args()
    from deepfakedetection_amd import kernels as K
    from deepfakedetection_amd._lib import MIX_CUTMIX, MIX_KEEP, MIX_MIXUP
    from deepfakedetection_amd.mix import BatchMixer, Decision, cutmix_box, job_table

    N, H = args.batch, args.size
    if args.case == "mixup":
        table = job_table([Decision(MIX_MIXUP, 0.3)] * N)
    elif args.case == "cutmix":
        y0, y1, x0, x1, lam = cutmix_box(0.5, H // 2, H // 2, H, H)
        table = job_table([Decision(MIX_CUTMIX, lam, (y0, y1, x0, x1))] * N)
    elif args.case == "keep":
        table = job_table([Decision()] * N)
    else:
        torch.manual_seed(0)
        table = BatchMixer(0.8, 1.0, mode="elem", num_classes=2).sample(N, H, H)
    if N % 2:
        table[N // 2] = job_table([Decision()])[0]
    # picture bytes a launch must move: a pair with a mixup reads both pictures and writes the mixed ones; a cutmix-only pair
    # reads and writes, in both pictures, the union of its boxes (here: equal boxes or one box)
    px = 0
    for i in range(N // 2):
        a, b = table[i].tolist(), table[N - 1 - i].tolist()
        if MIX_MIXUP in (a[0], b[0]):
            px += 2 * H * H + sum(H * H for r in (a, b) if r[0] != MIX_KEEP)
        else:
            boxes = [(r[4] - r[3]) * (r[6] - r[5]) for r in (a, b) if r[0] == MIX_CUTMIX]
            px += 4 * max(boxes) if boxes and (len(boxes) == 1 or a[3:7] == b[3:7]) else 4 * sum(boxes)
    nbytes = px * 3 * 4
    g = torch.Generator().manual_seed(1)
    fmt = torch.channels_last if args.layout == "nhwc" else torch.contiguous_format
    xs = [torch.randn(N, 3, H, H, generator=g).cuda().contiguous(memory_format=fmt) for _ in range(4)]
    labels = torch.randint(0, 2, (N,), generator=g).cuda()
    table = table.pin_memory()
    for x in xs:
        K.mix_batch(x, labels, table, 2)
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(args.iters):
        K.mix_batch(xs[i % 4], labels, table, 2)
    stop.record()
    torch.cuda.synchronize()
    us = 1e3 * start.elapsed_time(stop) / args.iters
    print(json.dumps({"case": args.case, "batch": N, "size": H, "layout": args.layout, "launches": args.iters,
                      "us_per_launch_incl_upload": round(us, 2), "picture_bytes": nbytes,
                      "TBps": round(nbytes / us / 1e6, 3) if nbytes else 0.0}), flush=True)


if __name__ == "__main__":
    main()
