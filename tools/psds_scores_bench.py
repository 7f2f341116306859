#!/usr/bin/env python3
"""Score-based PSDS (every distinct frame score a threshold) of a validation pass, three ways on the same device-resident scores
in one process.  Needs the GPU: no fallback.

--pairs (4096) (clip, phrase) pairs in batches of --batch (64), --T (250) frames, 1 .. 4 ground truths per pair, time resolution
0.04 s (tools/eval_bench.py's setting and its scores):
  device    per batch ScorePsdsEvaluator.update (tag_psds_score_deltas + two small sums), then compute (the merge on the device)
  host      the yardstick: the scores copied to the host, psds_scores.pair_regimes per pair, points_from_deltas, psds_from_counts
  composed  existing ops only, per chunk of --compose (1, 8, 64) pairs: the chunk's distinct values (torch.unique) and -inf as
            the threshold row of ops.segments (window 1, n_connect 0), ops.grounding_counts, the sum over the chunk's pairs; a
            chunk then enters the same merge as ONE pair.  The regions buffer is chunk x (chunk T + 1) x ceil(T / 2) x 16 bytes,
            so the work and the memory of a pass grow with the chunk size.
The PSDS values of all paths (max_efpr None and the reference's list) are asserted equal as floats BEFORE any time is printed.
Wall times around a synchronise, the paths alternate, one untimed warm-up round each; median [min - max] over --runs (5) rounds
(--host_runs (2) for the host path), 30 event-timed launches for the kernel alone on one batch.

    python tools/psds_scores_bench.py [--pairs 4096] [--batch 64] [--T 250] [--runs 5] [--host_runs 2] [--compose 1,8,64]
                                      [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

RES = 0.04


def summary(ts):
    ts = np.asarray(ts, dtype=np.float64)
    return {"ms_median": float(np.median(ts)), "ms_min": float(ts.min()), "ms_max": float(ts.max()), "runs": int(ts.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--T", type=int, default=250)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--host_runs", type=int, default=2)
    ap.add_argument("--compose", default="1,8,64")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("psds_scores_bench: no GPU; this measurement has no fallback")
    from eval_bench import make_ground_truth, make_scores
    from texttoaudiogrounding_amd import ops
    from texttoaudiogrounding_amd.utils import psds_scores as PS
    from texttoaudiogrounding_amd.utils.device_eval import ScorePsdsEvaluator, best_tp_per_fp, ground_truth_arrays

    dev = torch.device("cuda:0")
    max_efprs = list(PS.REFERENCE_MAX_EFPRS)
    items = make_ground_truth(args.pairs, args.T, 7)
    n_refs = sum(len(r) for r in items)
    total = float(args.pairs * args.T * RES)
    scores = make_scores(args.pairs, args.T, 17).to(dev)

    def chunks(size):
        cuts = [(a, min(a + size, args.pairs)) for a in range(0, args.pairs, size)]
        arrays = [ground_truth_arrays(items[a:b]) for a, b in cuts]         # (built by the data loader's workers in a real pass)
        return [(scores[a:b].contiguous(), torch.as_tensor(gt).to(dev), torch.as_tensor(gc).to(dev)) for (a, b), (gt, gc) in
                zip(cuts, arrays)]

    batches = chunks(args.batch)
    evaluator = ScorePsdsEvaluator(RES, device=dev)
    stats = {}

    def device_path():
        evaluator.reset()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        for fs, gt, gc in batches:
            evaluator.update(fs, gt, gc)
        out = evaluator.compute(total, max_efpr=max_efprs)
        ops.check_async_errors()
        stats["held_bytes"] = int(sum(t.numel() * t.element_size() for k in ("values", "deltas", "n_values")
                                      for t in evaluator.state()[k]))
        stats["peak_bytes_above_start"] = int(torch.cuda.max_memory_allocated() - before)
        stats["n_operating_points"] = out["n_operating_points"]
        stats["bytes_read_by_compute"] = evaluator.bytes_read
        return out["psds"]

    def host_path():
        rows = scores.cpu().numpy()
        values, deltas, base = [], [], np.zeros(2, dtype=np.int64)
        for row, gt in zip(rows, items):
            v, c = PS.pair_regimes(row, gt, RES)
            values.append(v)
            deltas.append(np.diff(c, axis=0))
            base += c[0]
        _, counts = PS.points_from_deltas(np.concatenate(values), np.concatenate(deltas), base)
        return PS.psds_from_counts(counts, n_refs, total, max_efprs)[0]

    def composed_path(parts):
        values, deltas = [], []
        base = torch.zeros(2, device=dev, dtype=torch.int64)
        for fs, gt, gc in parts:
            v = torch.unique(fs)
            th = torch.cat([torch.full((1,), -float("inf"), device=dev, dtype=torch.float64), v.double()])
            regions, counts = ops.segments(fs, th, 1, 0)
            c = ops.grounding_counts(regions, counts, gt, gc, RES, check=False)[..., 2:].sum(0, dtype=torch.int64)
            base += c[0]
            values.append(v)
            deltas.append(c[1:] - c[:-1])
        _, counts = PS.points_from_deltas(torch.cat(values), torch.cat(deltas), base)
        return PS.psds_from_counts(best_tp_per_fp(counts).cpu().numpy(), n_refs, total, max_efprs)[0]

    sizes = [int(s) for s in args.compose.split(",") if s]
    parts = {s: chunks(s) for s in sizes}
    paths = {"device": device_path, "host": host_path}
    paths.update({f"composed_{s}": (lambda s=s: composed_path(parts[s])) for s in sizes})
    values = {k: fn() for k, fn in paths.items()}                            # warm-up round, and the values
    for k, v in values.items():
        assert v == values["host"], f"{k} disagrees with the host yardstick: {v} != {values['host']}"
    assert 0.0 < values["host"][None] <= 1.0, values
    times = {k: [] for k in paths}
    for r in range(args.runs):
        for name, fn in paths.items():
            if name == "host" and r >= args.host_runs:
                continue
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
            assert got == values[name]

    fs, gt, gc = batches[0]
    ktimes = []
    for _ in range(3):
        ops.psds_score_deltas(fs, gt, gc, RES, check=False)
    torch.cuda.synchronize()
    for _ in range(30):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.psds_score_deltas(fs, gt, gc, RES, check=False)
        e1.record()
        torch.cuda.synchronize()
        ktimes.append(e0.elapsed_time(e1))

    res = {"pairs": args.pairs, "batch": args.batch, "T": args.T, "batches": len(batches), "n_refs": n_refs,
           "psds": {str(k): v for k, v in values["host"].items()}, "paths_equal": True,
           "n_operating_points": stats["n_operating_points"], "evaluator_held_bytes": stats["held_bytes"],
           "device_peak_bytes_above_start": stats["peak_bytes_above_start"],
           "bytes_read_by_compute": stats["bytes_read_by_compute"],
           "composed_regions_bytes_per_chunk": {str(s): int(s * (s * args.T + 1) * ((args.T + 1) // 2) * 16) for s in sizes},
           "kernel_one_batch": summary(ktimes)}
    res.update({k: summary(t) for k, t in times.items()})
    res["host_over_device"] = res["host"]["ms_median"] / res["device"]["ms_median"]
    line = json.dumps(res)
    print(line)
    for k in list(paths) + ["kernel_one_batch"]:
        s = res[k]
        print(f"{k:20s} {s['ms_median']:12.3f} ms [{s['ms_min']:.3f} - {s['ms_max']:.3f}] over {s['runs']} runs", file=sys.stderr)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
