#!/usr/bin/env python3
"""The metric phase of a validation pass, host path beside device path, on the same synthetic scores in one process.  Needs the
GPU: no fallback.

--pairs (4096) (clip, phrase) pairs in batches of --batch (64), --T (250) frames, --thresholds (50), 1 .. 4 ground truths per
pair (the evaluation leaves pairs without one out before it gets here), time resolution 0.04 s, window 1:
  host     per batch eval_util.segments_for_thresholds (tag_segments + the copy of every segment to the host), then
           grounding_eval.tables_from_segments, compute_th_auc and psds_intersection over all pairs
  device   per batch GroundingEvaluator.update (tag_segments + tag_grounding_counts + three small sums), then compute: ONE
           host read of (NT, 6) integers
  counts   ops.grounding_counts alone on one batch's segments, by device events
th-AUC and PSDS of the two paths are asserted equal as floats BEFORE any time is printed.  The scores are on the device before a
timed window opens (they come from the model there); wall times are taken around a synchronise, the two paths alternate, one
untimed warm-up round; median [min - max] over --runs (5) rounds, and 30 event-timed launches for the kernel.

    python tools/eval_bench.py [--pairs 4096] [--batch 64] [--T 250] [--thresholds 50] [--runs 5] [--out FILE.json]
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

RES, WINDOW = 0.04, 1


def summary(ts):
    ts = np.asarray(ts, dtype=np.float64)
    return {"ms_median": float(np.median(ts)), "ms_min": float(ts.min()), "ms_max": float(ts.max()), "runs": int(ts.size)}


def make_scores(n, T, seed):
    """As tests/test_gpu_path.py::test_device_segments_to_th_auc_and_psds: a level per clip, a slow sine and noise."""
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(n, 1, generator=g) * 0.5 + 0.2
    return (base + 0.35 * torch.sin(torch.arange(T)[None, :] / (3.0 + 5.0 * torch.rand(n, 1, generator=g))) +
            0.05 * torch.randn(n, T, generator=g)).clamp(1e-7, 1.0)


def make_ground_truth(n, T, seed):
    """1 .. 4 rows per pair, half of them on the frame grid."""
    rng = np.random.default_rng(seed)
    items = []
    for _ in range(n):
        rows = []
        for i in range(int(rng.integers(1, 5))):
            if i % 2 == 0:
                k = int(rng.integers(0, T - 1))
                rows.append([k * RES, (k + int(rng.integers(1, 60))) * RES])
            else:
                on = float(rng.uniform(0.0, T * RES * 0.9))
                rows.append([on, on + float(rng.uniform(0.05, 2.5))])
        items.append(rows)
    return items


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--T", type=int, default=250)
    ap.add_argument("--thresholds", type=int, default=50)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--max_efpr", type=float, default=800.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench: no GPU; this measurement has no fallback")
    from texttoaudiogrounding_amd import ops
    from texttoaudiogrounding_amd.utils import eval_util, grounding_eval as GE
    from texttoaudiogrounding_amd.utils.device_eval import GroundingEvaluator, ground_truth_arrays

    dev = torch.device("cuda:0")
    th = eval_util.eval_thresholds(args.thresholds)
    n_connect = eval_util.n_connect_for(RES)
    names = [f"clip{i}_0" for i in range(args.pairs)]
    items = make_ground_truth(args.pairs, args.T, 7)
    gt_table = {n: np.array(r, dtype=np.float64).reshape(-1, 2) for n, r in zip(names, items)}
    durations = {n: args.T * RES for n in names}
    total = float(sum(durations.values()))
    cuts = [(a, min(a + args.batch, args.pairs)) for a in range(0, args.pairs, args.batch)]
    scores = make_scores(args.pairs, args.T, 17).to(dev)
    batches = [scores[a:b].contiguous() for a, b in cuts]
    gt_arrays = [ground_truth_arrays(items[a:b]) for a, b in cuts]          # (built by the data loader's workers in a real pass)

    def host_path():
        segments = []
        for fs in batches:
            segments.extend(eval_util.segments_for_thresholds(fs, th, WINDOW, n_connect))
        tables = GE.tables_from_segments(segments, names, th, RES)
        return (GE.compute_th_auc(tables, gt_table), GE.psds_intersection(tables, gt_table, durations, max_efpr=args.max_efpr))

    evaluator = GroundingEvaluator(th, WINDOW, RES, device=dev)

    def device_path():
        evaluator.reset()
        for fs, (gt, gt_count) in zip(batches, gt_arrays):
            evaluator.update(fs, gt, gt_count)
        out = evaluator.compute(total, max_efpr=args.max_efpr)
        ops.check_async_errors()
        return out["th_auc"], out["psds"]

    paths = {"host": host_path, "device": device_path}
    values = {k: fn() for k, fn in paths.items()}                            # warm-up round, and the values
    assert values["host"] == values["device"], f"the two paths disagree: {values}"
    assert 0.0 < values["host"][0] < 1.0 and 0.0 < values["host"][1] <= 1.0, values
    times = {k: [] for k in paths}
    for _ in range(args.runs):
        for name, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
            assert got == values[name]

    regions, counts = ops.segments(batches[0], th, WINDOW, n_connect)
    gt0 = torch.as_tensor(gt_arrays[0][0]).to(dev)
    gc0 = torch.as_tensor(gt_arrays[0][1]).to(dev)
    out = torch.empty(regions.shape[0], regions.shape[1], 4, device=dev, dtype=torch.int32)
    kernel = {"counts": lambda: ops.grounding_counts(regions, counts, gt0, gc0, RES, out=out, check=False),
              "segments": lambda: ops.segments(batches[0], th, WINDOW, n_connect)}
    ktimes = {k: [] for k in kernel}
    for fn in kernel.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(30):
        for name, fn in kernel.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ktimes[name].append(e0.elapsed_time(e1))

    res = {"pairs": args.pairs, "batch": args.batch, "T": args.T, "thresholds": args.thresholds, "batches": len(cuts),
           "th_auc": values["host"][0], "psds": values["host"][1], "paths_equal": True,
           "mean_detections_per_pair_and_threshold": float(counts.double().mean().item()),
           "bytes_to_host_per_batch": {"host": int(regions.numel() * 8 + counts.numel() * 4), "device": 0},
           "bytes_to_host_per_evaluation": {"device": int(evaluator.counts.numel() * 8)},
           "host": summary(times["host"]), "device": summary(times["device"]),
           "counts_kernel_one_batch": summary(ktimes["counts"]), "segments_one_batch": summary(ktimes["segments"])}
    res["host_over_device"] = res["host"]["ms_median"] / res["device"]["ms_median"]
    line = json.dumps(res)
    print(line)
    for k in ("host", "device", "counts_kernel_one_batch", "segments_one_batch"):
        s = res[k]
        print(f"{k:28s} {s['ms_median']:10.3f} ms [{s['ms_min']:.3f} - {s['ms_max']:.3f}] over {s['runs']} runs", file=sys.stderr)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not res["device"]["ms_median"] < res["host"]["ms_median"]:
        raise SystemExit("eval_bench: the device path's metric phase is not faster than the host path's")


if __name__ == "__main__":
    main()
