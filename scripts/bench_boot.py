"""Cost of bootstrap intervals for the ROC figures: metrics.bootstrap (csrc/dfd_boot.hip) against what the parent commit offers.

    python scripts/bench_boot.py [--sizes 100000,1000000] [--members 1,3] [--replicates 2000] [--reps 3] [--baseline-rounds 100]
                                 [--host-rounds 3] [--passes 2000,500,100,25] [--tag TEXT] [--out FILE]

One JSON line per (n, M); `--out` appends them to a file (profiles/boot_eval.jsonl).  Scores: a 1:4 split with overlapping classes.

  bootstrap      metrics.bootstrap end to end on the host clock: M sorts, the point figures, the resamples, the one read-back.
  launches       kernels.boot_stats alone on sorted scores between two device events (`--reps` repetitions, median), with the tier
                 dfd_boot_plan names and the workspace boot_stats allocates by itself; `lds_tier` is the same at n =
                 BOOT_LDS_MAX_N, the largest n of the LDS tier (both --sizes defaults run in the global tier).
  by_workspace   the global tier's launches against R, the resamples per pass (n = the first size, M = 1).
  rounds         the parent commit's way: per resample torch.randint + index_select + metrics.binary_roc (one sort, the counting
                 kernels, one read-back).  `--baseline-rounds` rounds are timed; `scaled_to_B_ms` is that times B / rounds, and says so.
  host_numpy     numpy on the host: rng.integers + a sort-based AUC per resample, `--host-rounds` rounds, scaled the same way.
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


def make_case(n: int, members: int):
    g = torch.Generator().manual_seed(n)
    labels = (torch.rand(n, generator=g) < 0.2).long()
    scores = [torch.sigmoid(torch.randn(n, generator=g) + (1.5 - 0.25 * m) * labels).float().cuda() for m in range(members)]
    return scores, labels.cuda()


def device_ms(fn, reps: int) -> dict:
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        start.record()
        fn()
        stop.record()
        torch.cuda.synchronize()
        out.append(start.elapsed_time(stop))
    return {"median": round(statistics.median(out), 3), "min": round(min(out), 3), "max": round(max(out), 3), "reps": reps}


def launches(scores, labels, B: int, reps: int, ws_bytes: int | None = None) -> dict:
    from deepfakedetection_amd import kernels as K

    n = labels.numel()
    ordered, perms = [], []
    for s in scores:
        o, order = torch.sort(s)
        ordered.append(o.contiguous())
        perms.append(order.to(torch.int32).contiguous())
    is_pos = (labels == 1).to(torch.uint8)
    plan = K.boot_plan(n, B, len(scores), ws_bytes)
    ws = torch.empty(ws_bytes if ws_bytes is not None else (K.boot_ws(n, B) and plan.per_pass * 4 * n), dtype=torch.uint8, device="cuda")
    out = torch.empty((len(scores), B, K.BOOT_STATS_LEN), dtype=torch.int64, device="cuda")
    cuts = [0.5] * len(scores)
    rec = device_ms(lambda: K.boot_stats(ordered, perms, is_pos, B, 0, cuts, ws=ws, out=out), reps)
    rec.update(tier="lds" if plan.tier == K.BOOT_TIER_LDS else "global", per_pass=plan.per_pass, passes=plan.passes, ws_bytes=ws.numel())
    return rec


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--members", default="1,3")
    ap.add_argument("--replicates", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--baseline-rounds", type=int, default=100)
    ap.add_argument("--host-rounds", type=int, default=3)
    ap.add_argument("--passes", default="2000,500,100,25")
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_boot.py measures on the GPU only")
    from deepfakedetection_amd import kernels as K
    from deepfakedetection_amd import metrics as M

    B = args.replicates
    sizes = [int(s) for s in args.sizes.split(",") if s]
    lines = []

    def emit(rec: dict) -> None:
        if args.tag:
            rec["tag"] = args.tag
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for n in sizes:
        for members in (int(m) for m in args.members.split(",") if m):
            scores, labels = make_case(n, members)
            M.bootstrap(scores, labels, cut=0.5, replicates=B)                                          # warm-up: allocations, first launches
            torch.cuda.synchronize()
            times = []
            for _ in range(args.reps):
                t0 = perf_counter()
                res = M.bootstrap(scores, labels, cut=0.5, replicates=B)
                times.append(1e3 * (perf_counter() - t0))
            rec = {"n": n, "M": members, "B": B, "runs": "one run",
                   "bootstrap_ms": {"median": round(statistics.median(times), 1), "min": round(min(times), 1), "reps": args.reps},
                   "auc": res.point[0]["auc"], "auc_ci": res.interval("auc"), "launches_ms": launches(scores, labels, B, args.reps)}
            # the parent commit's way, member by member
            rounds = min(args.baseline_rounds, B)
            g = torch.Generator(device="cuda").manual_seed(0)
            for _ in range(3):
                idx = torch.randint(n, (n,), device="cuda", generator=g)
                M.binary_roc(scores[0].index_select(0, idx), labels.index_select(0, idx), cuts=[0.5])
            torch.cuda.synchronize()
            t0 = perf_counter()
            for _ in range(rounds):
                idx = torch.randint(n, (n,), device="cuda", generator=g)
                lab = labels.index_select(0, idx)
                for s in scores:
                    M.binary_roc(s.index_select(0, idx), lab, cuts=[0.5])
            spent = 1e3 * (perf_counter() - t0)
            rec["rounds"] = {"timed_rounds": rounds, "per_round_ms": round(spent / rounds, 3),
                             "scaled_to_B_ms": round(spent * B / rounds, 1), "scaled": rounds != B}
            host_scores, host_labels = [s.cpu().numpy() for s in scores], labels.cpu().numpy()
            rng = np.random.default_rng(0)
            t0 = perf_counter()
            for _ in range(args.host_rounds):
                idx = rng.integers(0, n, size=n)
                lab = host_labels[idx] == 1
                for s in host_scores:
                    drawn = s[idx]
                    neg = np.sort(drawn[~lab])
                    pos = drawn[lab]
                    (np.searchsorted(neg, pos, side="left").sum() + np.searchsorted(neg, pos, side="right").sum()) / (2 * pos.size * neg.size)
            spent = 1e3 * (perf_counter() - t0)
            rec["host_numpy"] = {"timed_rounds": args.host_rounds, "per_round_ms": round(spent / args.host_rounds, 2),
                                 "scaled_to_B_ms": round(spent * B / args.host_rounds, 1), "scaled": True, "figures": "auc only"}
            rec["rounds_over_bootstrap"] = round(rec["rounds"]["scaled_to_B_ms"] / rec["bootstrap_ms"]["median"], 2)
            emit(rec)

    scores, labels = make_case(K.BOOT_LDS_MAX_N, 1)
    emit({"part": "lds_tier", "n": K.BOOT_LDS_MAX_N, "M": 1, "B": B, "launches_ms": launches(scores, labels, B, args.reps)})
    n = sizes[0]
    if n > K.BOOT_LDS_MAX_N:
        scores, labels = make_case(n, 1)
        table = []
        for per_pass in (int(p) for p in args.passes.split(",") if p):
            per_pass = min(per_pass, B)
            table.append(launches(scores, labels, B, args.reps, ws_bytes=4 * n * per_pass))
        emit({"part": "by_workspace", "n": n, "M": 1, "B": B, "launches_ms": table})
    if args.out:
        path = Path(args.out)
        path.parent.mkdir(parents=True, exist_ok=True)
        with path.open("a", encoding="utf-8") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
