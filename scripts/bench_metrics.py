"""Cost of one split's evaluation metrics: the device path (metrics.py over csrc/dfd_metrics.hip) against the host path of the
inference orchestrator, on n binary scores that already sit on the device as a forward pass leaves them.

    python scripts/bench_metrics.py [--sizes 100000,1000000] [--batch 256] [--reps 20] [--rounds 5] [--host-rounds 1]
                                    [--tag TEXT] [--out FILE]

One JSON line per size; `--out` appends them to a file (profiles/metrics_eval.jsonl).

  device   torch.sort + the label gather, then dfd_roc_curve (four launches), dfd_roc_sweep over the orchestrator's 501 cuts and
           dfd_confusion: `--reps` eager repetitions between two device events, per round; the same captured into one graph and
           replayed (null when the capture is refused); and the sort + gather alone.  Nothing in it reads back: the one transfer
           of the results (stats, 2 x 501 counts, 4 cells) is timed apart as `readback_ms`.
  host     what the orchestrator's inference job does without inference.device_metrics: one blocking copy of the probabilities,
           the predictions and the targets per batch of `--batch` into a host metrics.ScoreBook, then _split_metrics (sklearn's
           roc_auc_score where sklearn is present, and the Python loop of confusion_counts) and the [501, n] numpy sweep of
           best_balanced_accuracy_threshold.  Host clock, `--host-rounds` rounds.
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


def spread(vals, digits=3) -> dict:
    return {"median": round(statistics.median(vals), digits), "min": round(min(vals), digits), "max": round(max(vals), digits)}


def make_case(n: int):
    """Probabilities [n, 2], arg-max predictions and targets on the device: a 1:4 split with overlapping classes."""
    g = torch.Generator().manual_seed(n)
    targets = (torch.rand(n, generator=g) < 0.2).long()
    logit = torch.randn(n, generator=g) + 1.5 * targets
    p1 = torch.sigmoid(logit)
    probs = torch.stack([1 - p1, p1], dim=1).float().contiguous()
    return probs.cuda(), probs.argmax(1).cuda(), targets.cuda()


def part_device(n: int, args) -> dict:
    from deepfakedetection_amd import kernels as K
    from deepfakedetection_amd.orchestration.orchestrator import SWEEP_STEPS

    probs, preds, targets = make_case(n)
    scores = probs[:, 1].contiguous()
    cuts = torch.linspace(0.0, 1.0, SWEEP_STEPS, dtype=torch.float64).cuda()
    ws = torch.empty(K.roc_ws(n), dtype=torch.uint8, device="cuda")
    curve = (torch.empty(n, device="cuda"), torch.empty(n, dtype=torch.int64, device="cuda"),
             torch.empty(n, dtype=torch.int64, device="cuda"), torch.empty(K.ROC_STATS_LEN, dtype=torch.int64, device="cuda"))
    swept = (torch.empty(SWEEP_STEPS, dtype=torch.int64, device="cuda"), torch.empty(SWEEP_STEPS, dtype=torch.int64, device="cuda"))
    conf = (torch.empty((2, 2), dtype=torch.int64, device="cuda"), torch.empty(1, dtype=torch.int64, device="cuda"))

    def sort_only():
        ordered, order = torch.sort(scores)
        return ordered, targets[order]

    def whole() -> None:
        ordered, lab = sort_only()
        K.roc_curve(ordered, lab, 1, ws=ws, out=curve)
        K.roc_sweep(*curve, cuts, out=swept)
        K.confusion_counts(targets, preds, 2, out=conf)

    def timed(fn) -> list:
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        out = []
        for _ in range(args.rounds):
            start.record()
            for _ in range(args.reps):
                fn()
            stop.record()
            torch.cuda.synchronize()
            out.append(start.elapsed_time(stop) / args.reps)
        return out

    for _ in range(3):
        whole()
    torch.cuda.synchronize()
    stats = curve[3].tolist()
    rec = {"part": "device", "n": n, "reps_per_round": args.reps, "stats": stats, "auc": stats[4] / (2 * stats[0] * stats[1]),
           "eager_ms": spread(timed(whole)), "sort_gather_ms": spread(timed(sort_only))}
    t0 = perf_counter()
    for _ in range(args.reps):
        curve[3].tolist(), swept[0].cpu(), swept[1].cpu(), conf[0].cpu()
    rec["readback_ms"] = round(1e3 * (perf_counter() - t0) / args.reps, 3)
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            whole()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            whole()
        graph.replay()
        torch.cuda.synchronize()
        assert curve[3].tolist() == stats, "the replayed launches and the eager ones disagree"
        rec["replayed_ms"] = spread(timed(graph.replay))
    except RuntimeError as exc:                                        # a sort that cannot be captured: the eager figures stand
        rec["replayed_ms"], rec["capture_error"] = None, str(exc).splitlines()[0][:200]
    return rec


def part_host(n: int, args) -> dict:
    from deepfakedetection_amd.metrics import ScoreBook
    from deepfakedetection_amd.orchestration import orchestrator as O

    try:
        import sklearn  # noqa: F401

        have_sklearn = True
    except ImportError:
        have_sklearn = False
    probs, preds, targets = make_case(n)
    torch.cuda.synchronize()
    copies, split, sweep = [], [], []
    auc = None
    for _ in range(args.host_rounds):
        t0 = perf_counter()
        book = ScoreBook(n, 2, "cpu")
        for i in range(0, n, args.batch):
            book.append(probs[i:i + args.batch], preds[i:i + args.batch], targets[i:i + args.batch])
        probs_t, preds_t, targets_t = book.probs, book.preds, book.targets
        t1 = perf_counter()
        record, _, _ = O._split_metrics("bench", "test", probs_t, preds_t, targets_t, 2, 0.5)
        t2 = perf_counter()
        O.best_balanced_accuracy_threshold(probs_t[:, 1].numpy(), targets_t.numpy())
        t3 = perf_counter()
        copies.append(1e3 * (t1 - t0))
        split.append(1e3 * (t2 - t1))
        sweep.append(1e3 * (t3 - t2))
        auc = record.get("roc_auc")
    total = [a + b + c for a, b, c in zip(copies, split, sweep)]
    return {"part": "host", "n": n, "batch": args.batch, "rounds": args.host_rounds, "sklearn": have_sklearn, "auc": auc,
            "per_batch_copies_ms": spread(copies, 1), "auc_and_confusion_ms": spread(split, 1), "numpy_sweep_ms": spread(sweep, 1),
            "total_ms": spread(total, 1)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-rounds", type=int, default=1)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics.py measures on the GPU only")
    lines = []
    for n in (int(s) for s in args.sizes.split(",") if s):
        device, host = part_device(n, args), part_host(n, args)
        rec = {"n": n, "device": device, "host": host,
               "host_over_device": round(host["total_ms"]["median"] / (device["eager_ms"]["median"] + device["readback_ms"]), 1)}
        if args.tag:
            rec["tag"] = args.tag
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        path = Path(args.out)
        path.parent.mkdir(parents=True, exist_ok=True)
        with path.open("a", encoding="utf-8") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
