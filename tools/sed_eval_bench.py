#!/usr/bin/env python3
"""The sed_eval protocol of a validation pass, host path beside device path, on the same synthetic scores in one process.  Needs
the GPU: no fallback.

--pairs (4096) (clip, phrase) pairs in batches of --batch (64), --T (250) frames, --thresholds (50), 1 .. 4 ground truths per
pair, time resolution 0.04 s, window 1, collar 0.2 s / 20 %, 1 s segments (the shapes of tools/eval_bench.py):
  host     per batch eval_util.segments_for_thresholds (tag_segments + the copy of every segment to the host), then per threshold
           a detection table and sed_metrics.compute_sed_eval over all pairs
  device   per batch SedEvaluator.update (tag_segments + tag_sed_counts + three small sums), then compute: ONE host read of
           (NT, 7) integers
  counts   ops.sed_counts alone on one batch's segments, by device events; segments_double likewise
The counts and every score of the two paths are asserted equal BEFORE any time is printed.  The scores are on the device before
a timed window opens; wall times are taken around a synchronise, the two paths alternate, one untimed warm-up round; median
[min - max] over --runs (5) rounds, and 30 event-timed launches for the kernels.  The host path is the baseline.

    python tools/sed_eval_bench.py [--pairs 4096] [--batch 64] [--T 250] [--thresholds 50] [--runs 5] [--out FILE.json]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from eval_bench import RES, WINDOW, make_ground_truth, make_scores, summary  # noqa: E402

T_COLLAR, PERCENTAGE, SEGMENT = 0.2, 0.2, 1.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--T", type=int, default=250)
    ap.add_argument("--thresholds", type=int, default=50)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sed_eval_bench: no GPU; this measurement has no fallback")
    from texttoaudiogrounding_amd import ops
    from texttoaudiogrounding_amd.utils import eval_util, sed_metrics
    from texttoaudiogrounding_amd.utils.device_eval import SedEvaluator, ground_truth_arrays

    dev = torch.device("cuda:0")
    th = eval_util.eval_thresholds(args.thresholds)
    n_connect = eval_util.n_connect_for(RES)
    names = [f"clip{i}_0" for i in range(args.pairs)]
    items = make_ground_truth(args.pairs, args.T, 7)
    gt_table = {n: np.array(r, dtype=np.float64).reshape(-1, 2) for n, r in zip(names, items)}
    cuts = [(a, min(a + args.batch, args.pairs)) for a in range(0, args.pairs, args.batch)]
    scores = make_scores(args.pairs, args.T, 17).to(dev)
    batches = [scores[a:b].contiguous() for a, b in cuts]
    gt_arrays = [ground_truth_arrays(items[a:b]) for a, b in cuts]          # (built by the data loader's workers in a real pass)

    def host_path():
        segments = []
        for fs in batches:
            segments.extend(eval_util.segments_for_thresholds(fs, th, WINDOW, n_connect))
        counts = np.stack([sed_metrics.count_tables(gt_table, {n: segments[b][t].astype(np.float64) * RES for b, n in enumerate(names)},
                                                    T_COLLAR, SEGMENT, PERCENTAGE) for t in range(len(th))])
        ev_tp, seg_tp, seg_fp, seg_fn, seg_n, n_sys, n_ref = counts.T
        return counts, sed_metrics.scores_from_counts(ev_tp, n_sys, n_ref, seg_tp, seg_fp, seg_fn, seg_n)

    evaluator = SedEvaluator(thresholds=th, window_size=WINDOW, time_resolution=RES, t_collar=T_COLLAR,
                             percentage_of_length=PERCENTAGE, segment_resolution=SEGMENT, device=dev)

    def device_path():
        evaluator.reset()
        for fs, (gt, gt_count) in zip(batches, gt_arrays):
            evaluator.update(fs, gt, gt_count)
        out = evaluator.compute()
        ops.check_async_errors()
        return out["counts"], out

    def same(a, b):
        return np.array_equal(a[0], b[0]) and all(np.array_equal(a[1][f][k], b[1][f][k]) for f in ("event", "segment") for k in a[1][f])

    paths = {"host": host_path, "device": device_path}
    values = {k: fn() for k, fn in paths.items()}                            # warm-up round, and the values
    assert same(values["host"], values["device"]), "the two paths disagree"
    best_event = float(values["host"][1]["event"]["f_measure"].max())
    best_segment = float(values["host"][1]["segment"]["f_measure"].max())
    assert 0.0 < best_event < 1.0 and 0.0 < best_segment < 1.0, (best_event, best_segment)
    times = {k: [] for k in paths}
    for _ in range(args.runs):
        for name, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
            assert same(got, values[name])

    regions, counts = ops.segments(batches[0], th, WINDOW, n_connect)
    gt0 = torch.as_tensor(gt_arrays[0][0]).to(dev)
    gc0 = torch.as_tensor(gt_arrays[0][1]).to(dev)
    out = torch.empty(regions.shape[0], regions.shape[1], 5, device=dev, dtype=torch.int32)
    high = torch.as_tensor(np.minimum(th + 0.2, 1.0))
    kernel = {"counts": lambda: ops.sed_counts(regions, counts, gt0, gc0, RES, T_COLLAR, PERCENTAGE, SEGMENT, out=out, check=False),
              "segments": lambda: ops.segments(batches[0], th, WINDOW, n_connect),
              "segments_double": lambda: ops.segments_double(batches[0], high, th, n_connect)}
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
           "best_event_f": best_event, "best_segment_f": best_segment, "paths_equal": True,
           "mean_detections_per_pair_and_threshold": float(counts.double().mean().item()),
           "bytes_to_host_per_batch": {"host": int(regions.numel() * 8 + counts.numel() * 4), "device": 0},
           "bytes_to_host_per_evaluation": {"device": int(evaluator.counts.numel() * 8 + 8)},
           "host": summary(times["host"]), "device": summary(times["device"]),
           "counts_kernel_one_batch": summary(ktimes["counts"]), "segments_one_batch": summary(ktimes["segments"]),
           "segments_double_one_batch": summary(ktimes["segments_double"])}
    res["host_over_device"] = res["host"]["ms_median"] / res["device"]["ms_median"]
    line = json.dumps(res)
    print(line)
    for k in ("host", "device", "counts_kernel_one_batch", "segments_one_batch", "segments_double_one_batch"):
        s = res[k]
        print(f"{k:28s} {s['ms_median']:10.3f} ms [{s['ms_min']:.3f} - {s['ms_max']:.3f}] over {s['runs']} runs", file=sys.stderr)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
