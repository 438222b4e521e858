"""Cost of the ensemble figures of one split: the device path (metrics.fuse, metrics.fit_fusion and metrics.diversity over
csrc/dfd_fuse.hip) against the numpy reference of tests/_fuse_ref.py, on K members' n rows of J logits that already sit on the
device.

    python scripts/bench_fuse.py [--shapes 100000x2x3,1000000x2x3] [--reps 5] [--rounds 3] [--host-elements 8000000]
                                 [--tag TEXT] [--out FILE]

One JSON line per (n, J, K); `--out` appends them to a file (profiles/fuse_eval.jsonl).

  device   metrics.fuse (two launches, nothing read back: `--reps` repetitions between two device events, per round), then the
           whole calls with their read-backs on the host clock: metrics.fit_fusion (one launch pair and one read-back per Newton
           iteration) and metrics.diversity (one read-back).  Medians over the rounds.
  host     _fuse_ref.scores, _fuse_ref.fit and _fuse_ref.agree on the same data, host clock, one round; skipped (null, with the
           reason) above `--host-elements` n * J * K elements.
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


def part_device(zs, targets, args) -> dict:
    from deepfakedetection_amd import kernels as K
    from deepfakedetection_amd import metrics as M

    members = [torch.from_numpy(z).cuda() for z in zs]
    y = torch.from_numpy(targets).cuda()
    n, J = zs[0].shape
    M.fuse(members)
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fuse_ms, fit_ms, div_ms = [], [], []
    for _ in range(args.rounds):
        start.record()
        for _ in range(args.reps):
            probs, preds, _ = M.fuse(members)
        stop.record()
        torch.cuda.synchronize()
        fuse_ms.append(start.elapsed_time(stop) / args.reps)
    member_preds = [K.softmax_argmax(z, False)[1] for z in members]
    M.fit_fusion(members, y)
    M.diversity(member_preds, y, J)
    for _ in range(args.rounds):
        torch.cuda.synchronize()
        t0 = perf_counter()
        for _ in range(args.reps):
            fit = M.fit_fusion(members, y)
        t1 = perf_counter()
        for _ in range(args.reps):
            div = M.diversity(member_preds, y, J)
        t2 = perf_counter()
        fit_ms.append(1e3 * (t1 - t0) / args.reps)
        div_ms.append(1e3 * (t2 - t1) / args.reps)
    plan = K.fuse_plan(n, J, len(zs))
    return {"part": "device", "reps_per_round": args.reps, "rounds": args.rounds, "plan": [plan.layout, plan.rows, plan.blocks, plan.trips],
            "fuse_ms": spread(fuse_ms), "fit_fusion_ms": spread(fit_ms), "diversity_ms": spread(div_ms), "coef": fit.coef,
            "iterations": fit.iterations, "converged": fit.converged, "nll_after": fit.nll_after, "oracle_accuracy": div.oracle_accuracy,
            "pair": div.pair, "member_preds": [p.cpu().numpy() for p in member_preds], "probs": probs.cpu().numpy()}


def part_host(zs, targets, member_preds, args) -> dict:
    from tests import _fuse_ref as R

    n, J = zs[0].shape
    if n * J * len(zs) > args.host_elements:
        return {"part": "host", "total_ms": None, "reason": f"n * J * K above --host-elements {args.host_elements}"}
    t0 = perf_counter()
    probs = R.scores(zs, [1.0 / len(zs)] * len(zs))[0]
    t1 = perf_counter()
    fit = R.fit(zs, targets)
    t2 = perf_counter()
    pair, _, _ = R.agree(member_preds, targets, J)
    t3 = perf_counter()
    return {"part": "host", "rounds": 1, "scores_ms": round(1e3 * (t1 - t0), 1), "fit_ms": round(1e3 * (t2 - t1), 1),
            "agree_ms": round(1e3 * (t3 - t2), 1), "total_ms": round(1e3 * (t3 - t0), 1), "coef": fit.coef, "iterations": fit.iterations,
            "pair": pair, "probs": probs}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="100000x2x3,1000000x2x3", help="n x J x K, comma separated")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-elements", type=int, default=8_000_000)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fuse.py measures on the GPU only")
    from tests import _fuse_ref as R

    lines = []
    for n, J, K in (tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",") if s):
        zs, targets = R.members_case(n + J + K, n, J, K)
        device = part_device(zs, targets, args)
        host = part_host(zs, targets, device.pop("member_preds"), args)
        device_probs = device.pop("probs")
        rec = {"n": n, "J": J, "K": K, "device": device, "host": host}
        if host["total_ms"] is not None:
            differ, worst = R.ulp_mismatches(device_probs, host.pop("probs"))
            assert worst <= 1 and differ * 1000 <= device_probs.size and host["pair"] == device["pair"]
            assert np.allclose(host["coef"], device["coef"], rtol=0.0, atol=1e-8)
            total = device["fuse_ms"]["median"] + device["fit_fusion_ms"]["median"] + device["diversity_ms"]["median"]
            rec["host_over_device"] = round(host["total_ms"] / total, 1)
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
