"""Cost of the calibration figures of one split: the device path (metrics.calibration and metrics.fit_temperature over
csrc/dfd_calib.hip) against the numpy reference of tests/_calib_ref.py, on n rows of J logits that already sit on the device.

    python scripts/bench_calib.py [--sizes 100000,1000000] [--classes 2,1000] [--reps 10] [--rounds 5] [--host-elements 4000000]
                                  [--tag TEXT] [--out FILE]

One JSON line per (n, J); `--out` appends them to a file (profiles/calib_eval.jsonl).

  device   the launches that read nothing back — dfd_calib_bins (three launches), dfd_calib_nll at the 32 betas of one fitting
           round (two launches) and dfd_softmax_argmax_t — `--reps` eager repetitions between two device events, per round, and
           the same captured into one graph and replayed; then the whole calls with their read-backs on the host clock:
           metrics.calibration (one read-back) and metrics.fit_temperature (one per round).
  host     _calib_ref.bins + ece_mce and _calib_ref.fit_temperature on the same data, host clock, one round; skipped (null, with
           the reason) above `--host-elements` n * J elements, where the float64 copies and Python lists of the reference do not fit.
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


def spread(vals, digits=3) -> dict:
    return {"median": round(statistics.median(vals), digits), "min": round(min(vals), digits), "max": round(max(vals), digits)}


def make_case(n: int, J: int):
    """Logits 1.5 times too sharp for their labels (the best temperature is about 1.5) and the labels, on the device."""
    g = torch.Generator(device="cuda").manual_seed(n + J)
    z = torch.randn((n, J), generator=g, device="cuda") * 2.0
    targets = torch.multinomial(torch.softmax(z, dim=1), 1, generator=g).reshape(-1)
    return (1.5 * z).contiguous(), targets.contiguous()


def part_device(n: int, J: int, args) -> dict:
    from deepfakedetection_amd import kernels as K
    from deepfakedetection_amd import metrics as M

    logits, targets = make_case(n, J)
    betas = M._geometric(0.01, 20.0, M.FIT_ROUND_BETAS)
    probs = K.softmax_argmax(logits, True)[0]
    bins_out = (torch.empty((15, 3), dtype=torch.int64, device="cuda"), torch.empty(4, dtype=torch.int64, device="cuda"),
                torch.empty(1, dtype=torch.float64, device="cuda"))
    nll_out = (torch.empty((len(betas), 3), dtype=torch.float64, device="cuda"), torch.empty(2, dtype=torch.int64, device="cuda"))
    ws = torch.empty(K.calib_nll_ws(n, J, len(betas)) // 8, dtype=torch.float64, device="cuda").view(torch.uint8)      # 8-byte aligned

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

    def both(fn) -> dict:
        fn()
        torch.cuda.synchronize()
        rec = {"eager_ms": spread(timed(fn))}
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                fn()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                fn()
            graph.replay()
            torch.cuda.synchronize()
            rec["replayed_ms"] = spread(timed(graph.replay))
        except RuntimeError as exc:
            rec["replayed_ms"], rec["capture_error"] = None, str(exc).splitlines()[0][:200]
        return rec

    plan = K.calib_plan(n, J)
    rec = {"part": "device", "n": n, "J": J, "reps_per_round": args.reps, "rounds": args.rounds,
           "plan": [plan.layout, plan.rows, plan.blocks, plan.trips],
           "calib_bins": both(lambda: K.calib_bins(probs, targets, 15, ws=ws, out=bins_out)),
           "calib_nll_32": both(lambda: K.calib_nll(logits, targets, betas, ws=ws, out=nll_out)),
           "softmax_argmax_t": both(lambda: K.softmax_argmax_t(logits, 1.0 / 1.5))}
    whole_cal, whole_fit = [], []
    for _ in range(args.rounds):
        torch.cuda.synchronize()
        t0 = perf_counter()
        res = M.calibration(probs, targets, 15)
        t1 = perf_counter()
        fit = M.fit_temperature(logits, targets)
        t2 = perf_counter()
        whole_cal.append(1e3 * (t1 - t0))
        whole_fit.append(1e3 * (t2 - t1))
    rec.update(calibration_ms=spread(whole_cal), fit_temperature_ms=spread(whole_fit), ece=res.ece, brier=res.brier,
               temperature=fit.temperature, fit_rounds=fit.rounds)
    return rec


def part_host(n: int, J: int, args) -> dict:
    from deepfakedetection_amd import kernels as K
    from tests import _calib_ref as R

    if n * J > args.host_elements:
        return {"part": "host", "n": n, "J": J, "total_ms": None, "reason": f"n * J above --host-elements {args.host_elements}"}
    logits, targets = make_case(n, J)
    probs = K.softmax_argmax(logits, True)[0].cpu().numpy()
    logits, targets = logits.cpu().numpy(), targets.cpu().numpy()
    t0 = perf_counter()
    ref = R.bins(probs, targets, 15)
    ece, _ = R.ece_mce(ref.table, ref.stats[0])
    t1 = perf_counter()
    fit = R.fit_temperature(logits, targets)
    t2 = perf_counter()
    return {"part": "host", "n": n, "J": J, "rounds": 1, "bins_ms": round(1e3 * (t1 - t0), 1), "fit_ms": round(1e3 * (t2 - t1), 1),
            "total_ms": round(1e3 * (t2 - t0), 1), "ece": ece, "temperature": fit.temperature}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--classes", default="2,1000")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-elements", type=int, default=4_000_000)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_calib.py measures on the GPU only")
    lines = []
    for n in (int(s) for s in args.sizes.split(",") if s):
        for J in (int(s) for s in args.classes.split(",") if s):
            device, host = part_device(n, J, args), part_host(n, J, args)
            rec = {"n": n, "J": J, "device": device, "host": host}
            if host["total_ms"] is not None:
                rec["host_over_device"] = round(host["total_ms"] / (device["calibration_ms"]["median"] + device["fit_temperature_ms"]["median"]), 1)
                assert host["ece"] == device["ece"] and abs(host["temperature"] - device["temperature"]) <= 1e-6 * host["temperature"]
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
