"""Cost of per-video scores and of the cluster bootstrap: kernels.group_pool (csrc/dfd_group.hip) against what the parent commit
offers, and kernels.boot_stats_grouped against kernels.boot_stats at the same n in the same run.

    python scripts/bench_group.py [--sizes 100000,1000000] [--per-group 100] [--members 1,3] [--replicates 2000] [--reps 5]
                                  [--rounds 3] [--tag TEXT] [--out FILE]

One JSON line per measurement; `--out` appends them to a file (profiles/group_eval.jsonl).  Every timing is the median over
`--rounds` rounds of `--reps` repetitions between two device events, replayed from a captured graph where the capture succeeds
(`replayed` says whether it did); the first round is preceded by a warm-up replay.

  pool        kernels.group_pool (three launches, nothing read back) for n rows of J = 2 classes in G = n / --per-group groups, ids
              sorted (ImageFolder order) and shuffled, in the three modes, with the tier dfd_group_plan names.
              `index_add`: torch.zeros(G, J).index_add_(0, ids, probs) / counts, the float-atomic way of the parent commit.
              `same_bits`: whether sorted and shuffled ids gave identical bits (group_pool must; index_add_ need not).
  bootstrap   kernels.boot_stats_grouped for B resamples of the G groups of the same n samples, against kernels.boot_stats at that n:
              the difference is the gather through group[] and the smaller counts array.  `identity_groups`: the same call with
              every sample its own group (G = n), which leaves the gather as the only difference to boot_stats.
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch  # noqa: E402


def timed(fn, reps: int, rounds: int) -> dict:
    """Median / min / max of `rounds` rounds of `reps` calls of fn, in ms per call, replayed from a graph when fn can be captured."""
    fn()
    torch.cuda.synchronize()
    replayed, run = False, fn
    try:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fn()
        run, replayed = graph.replay, True
    except Exception:                                                   # the eager launches are timed instead, and the record says so
        torch.cuda.synchronize()
    run()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(rounds):
        start.record()
        for _ in range(reps):
            run()
        stop.record()
        torch.cuda.synchronize()
        out.append(start.elapsed_time(stop) / reps)
    return {"median": round(statistics.median(out), 4), "min": round(min(out), 4), "max": round(max(out), 4), "reps": reps, "rounds": rounds,
            "replayed": replayed}


def pool_part(n: int, per_group: int, args, emit) -> None:
    from deepfakedetection_amd import kernels as K

    J, G = 2, max(n // per_group, 1)
    g = torch.Generator().manual_seed(n)
    p1 = torch.rand(n, generator=g)
    probs = torch.stack([1 - p1, p1], dim=1).float().cuda().contiguous()
    ids_sorted = ((torch.arange(n, dtype=torch.int64) * G) // n).to(torch.int32)
    order = torch.randperm(n, generator=g)
    targets = (ids_sorted.long() % J)
    plan = K.group_plan(n, G, J)
    ws = torch.empty(K.group_ws(n, G, J), dtype=torch.uint8, device="cuda")
    rec = {"part": "pool", "n": n, "G": G, "J": J, "tier": "lds" if plan.tier == K.GROUP_TIER_LDS else "global", "workgroups": plan.workgroups}
    bits = {}
    for layout, perm in (("sorted", None), ("shuffled", order)):
        ids = (ids_sorted if perm is None else ids_sorted[perm]).cuda().contiguous()
        rows = (probs if perm is None else probs[perm.cuda()]).contiguous()
        tgt = (targets if perm is None else targets[perm]).cuda().contiguous()
        counts = torch.bincount(ids.long(), minlength=G).float().unsqueeze(1)
        ids64 = ids.long()
        for mode, code in (("mean", K.GROUP_MEAN), ("vote", K.GROUP_VOTE), ("max", K.GROUP_MAX)):
            out = [torch.empty((G, J), device="cuda"), torch.empty(G, dtype=torch.int64, device="cuda"),
                   torch.empty(G, dtype=torch.int64, device="cuda"), torch.empty(G, dtype=torch.int32, device="cuda"),
                   torch.empty(4, dtype=torch.int64, device="cuda")]
            rec[f"{mode}_{layout}_ms"] = timed(lambda: K.group_pool(rows, ids, tgt, G, code, 1, ws=ws, out=out), args.reps, args.rounds)
            if mode == "mean":
                bits[layout] = out[0].clone()
        base = torch.empty((G, J), device="cuda")

        def index_add():
            base.zero_()
            base.index_add_(0, ids64, rows)
            base.div_(counts)

        rec[f"index_add_{layout}_ms"] = timed(index_add, args.reps, args.rounds)
        bits[f"index_add_{layout}"] = base.clone()
    rec["same_bits"] = bool(torch.equal(bits["sorted"].view(torch.int32), bits["shuffled"].view(torch.int32)))
    rec["index_add_same_bits"] = bool(torch.equal(bits["index_add_sorted"].view(torch.int32), bits["index_add_shuffled"].view(torch.int32)))
    rec["max_abs_mean_minus_index_add"] = float((bits["sorted"] - bits["index_add_sorted"]).abs().max())
    emit(rec)


def boot_part(n: int, per_group: int, members: int, args, emit) -> None:
    from deepfakedetection_amd import kernels as K

    B, G = args.replicates, max(n // per_group, 1)
    g = torch.Generator().manual_seed(n + members)
    ids = ((torch.arange(n, dtype=torch.int64) * G) // n).to(torch.int32).cuda()
    labels = (ids.long() % 5 == 0).long()
    ordered, perms = [], []
    for m in range(members):
        s = torch.sigmoid(torch.randn(n, generator=g).cuda() + (1.5 - 0.25 * m) * labels).float()
        o, order = torch.sort(s)
        ordered.append(o.contiguous())
        perms.append(order.to(torch.int32).contiguous())
    is_pos = (labels == 1).to(torch.uint8)
    largest = int(torch.bincount(ids.long()).max())
    cuts = [0.5] * members
    out = torch.empty((members, B, K.BOOT_STATS_LEN), dtype=torch.int64, device="cuda")
    plan_g, plan = K.boot_plan_grouped(n, G, largest, B, members), K.boot_plan(n, B, members)
    ws_g = torch.empty(max(K.boot_ws_grouped(n, G, B), 1), dtype=torch.uint8, device="cuda")
    ws = torch.empty(max(plan.per_pass * 4 * n if K.boot_ws(n, B) else 1, 1), dtype=torch.uint8, device="cuda")
    rec = {"part": "bootstrap", "n": n, "G": G, "M": members, "B": B, "max_size": largest,
           "grouped_tier": "lds" if plan_g.tier == K.BOOT_TIER_LDS else "global", "plain_tier": "lds" if plan.tier == K.BOOT_TIER_LDS else "global",
           "plain_passes": plan.passes}
    reps = max(args.reps // 2, 1)
    rec["grouped_ms"] = timed(lambda: K.boot_stats_grouped(ordered, perms, is_pos, ids, G, largest, B, 0, cuts, ws=ws_g, out=out), reps, args.rounds)
    rec["plain_ms"] = timed(lambda: K.boot_stats(ordered, perms, is_pos, B, 0, cuts, ws=ws, out=out), reps, args.rounds)
    rec["grouped_over_plain"] = round(rec["grouped_ms"]["median"] / rec["plain_ms"]["median"], 3)
    # the gather alone: every sample its own group, so both sides draw n counts in the same tier with the same workspace
    own = torch.arange(n, dtype=torch.int32, device="cuda")
    rec["identity_groups_ms"] = timed(lambda: K.boot_stats_grouped(ordered, perms, is_pos, own, n, 1, B, 0, cuts, ws=ws, out=out), reps, args.rounds)
    rec["identity_over_plain"] = round(rec["identity_groups_ms"]["median"] / rec["plain_ms"]["median"], 3)
    emit(rec)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--per-group", type=int, default=100)
    ap.add_argument("--members", default="1,3")
    ap.add_argument("--replicates", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_group.py measures on the GPU only")
    lines = []

    def emit(rec: dict) -> None:
        rec["runs"] = "one run"
        if args.tag:
            rec["tag"] = args.tag
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for n in (int(s) for s in args.sizes.split(",") if s):
        pool_part(n, args.per_group, args, emit)
        for members in (int(m) for m in args.members.split(",") if m):
            boot_part(n, args.per_group, members, args, emit)
    if args.out:
        path = Path(args.out)
        path.parent.mkdir(parents=True, exist_ok=True)
        with path.open("a", encoding="utf-8") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
