#!/usr/bin/env python3
"""The fused phrase-to-label cosine map (csrc/label_map.hip: ops.label_map) beside the same result composed from what the library
already had, and beside the reference's per-item sklearn call on the host.  Device events, every device path alternated in one
process, one JSON object.  Needs the GPU: there is no fallback.

Paths at N = --n (32768) phrases, C = --c (527) labels, D = --d (384), seeded Gaussian rows, thresholds at the 0.6 and 0.999
quantiles of a sample of the similarities:
  fused           ops.label_map(x, e, th0, th1): best, best_sim, min_sim, win_best, win_count, win_bits; N + C floats of workspace
  fused_sim       the same with the (N, C) similarities written
  fused_top4      fused_sim + the top-4 launch over them
  composed        rows through x / ||x|| (torch), ops.gemm into an (N, C) buffer, torch max / min, the window compare, its
                  count and the masked argmax
  composed_top4   composed + torch.topk(4) over the masked scores
  sklearn_items   sklearn's cosine_similarity(phrase.reshape(1, -1), label_embs) + argmax per item, --sk_items (4096) items spread
                  over --sk_workers (16) host processes (started BEFORE the GPU is opened), as every ``__getitem__`` of the
                  reference's datasets does; skipped when sklearn is not importable
Each device path is warmed up, then timed --runs (>= 20) times with the paths interleaved; median, min, max and quartiles.

    python tools/label_map_bench.py [--n 32768] [--c 527] [--d 384] [--runs 20] [--sk_items 4096] [--sk_workers 16] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP32_MFMA_PEAK_TFLOPS = 157.0
_LABELS = None


def summary(ts):
    ts = np.asarray(ts)
    return {"ms_median": float(np.median(ts)), "ms_min": float(ts.min()), "ms_max": float(ts.max()),
            "ms_q1": float(np.percentile(ts, 25)), "ms_q3": float(np.percentile(ts, 75)), "runs": int(ts.size)}


def _sk_init(labels):
    global _LABELS
    _LABELS = labels


def _sk_items(rows):
    from sklearn.metrics.pairwise import cosine_similarity
    return [int(cosine_similarity(r.reshape(1, -1), _LABELS)[0].argmax()) for r in rows]


def bench_sklearn(x, e, items, workers):
    try:
        import sklearn  # noqa: F401
    except ImportError:
        return None
    import multiprocessing
    rows = x[:items]
    with multiprocessing.get_context("fork").Pool(workers, initializer=_sk_init, initargs=(e,)) as pool:
        pool.map(_sk_items, np.array_split(rows[: 16 * workers], workers))           # warm-up: imports
        t0 = time.perf_counter()
        best = pool.map(_sk_items, np.array_split(rows, workers))
        dt = time.perf_counter() - t0
    return {"items": int(len(rows)), "workers": workers, "ms": dt * 1e3, "us_per_item": dt / len(rows) * 1e6,
            "ms_for_all_rows": dt / len(rows) * len(x) * 1e3, "best": np.concatenate([np.asarray(b) for b in best])}


def device_paths(x, e, th0, th1):
    import torch
    from texttoaudiogrounding_amd import ops
    N, D = x.shape
    C = e.shape[0]
    scores = torch.empty(N, C, device=x.device)
    neg = torch.tensor(float("-inf"), device=x.device)

    def composed(k=0):
        xn, en = x / x.norm(dim=1, keepdim=True), e / e.norm(dim=1, keepdim=True)
        ops.gemm(xn, en, N, C, D, transB=True, out=scores)
        best_sim, best = scores.max(1)
        min_sim = scores.min(1).values
        mask = (scores >= th0) & (scores <= th1) & (scores != 0)
        count = mask.sum(1)
        masked = torch.where(mask, scores, neg)
        win_best = torch.where(count > 0, masked.argmax(1), -1)
        top = torch.topk(masked, k, dim=1).indices if k else None
        return best, best_sim, min_sim, win_best, count, top

    return {"fused": lambda: ops.label_map(x, e, th0, th1),
            "fused_sim": lambda: ops.label_map(x, e, th0, th1, want_sim=True),
            "fused_top4": lambda: ops.label_map(x, e, th0, th1, topk=4, want_sim=True),
            "composed": composed, "composed_top4": lambda: composed(4)}, scores


def bench_device(x, e, th0, th1, runs):
    import torch
    from texttoaudiogrounding_amd import ops
    paths, scores = device_paths(x, e, th0, th1)
    out = {}
    for name, fn in paths.items():                                # warm-up: code objects, allocator
        for _ in range(3):
            out[name] = fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(runs):
        for name, fn in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
    (N, D), C = x.shape, e.shape[0]
    res = {k: summary(v) for k, v in times.items()}
    for k in ("fused", "fused_sim"):
        res[k]["tflops"] = 2.0 * N * C * D / (res[k]["ms_median"] * 1e-3) / 1e12
        res[k]["share_of_fp32_mfma_peak"] = res[k]["tflops"] / FP32_MFMA_PEAK_TFLOPS
    res["fused_over_composed"] = res["fused"]["ms_median"] / res["composed"]["ms_median"]
    res["fused_sim_over_composed"] = res["fused_sim"]["ms_median"] / res["composed"]["ms_median"]
    res["fused_top4_over_composed_top4"] = res["fused_top4"]["ms_median"] / res["composed_top4"]["ms_median"]
    res["composed_spread_ms"] = res["composed"]["ms_max"] - res["composed"]["ms_min"]
    res["fused_spread_ms"] = res["fused"]["ms_max"] - res["fused"]["ms_min"]
    f, c = out["fused_sim"], out["composed"]
    res["best_differing_from_composed"] = int((f.best != c[0]).sum().item())
    res["win_best_differing_from_composed"] = int((f.win_best != c[3]).sum().item())
    res["max_sim_difference"] = float((f.sim - scores).abs().max().item())
    res["bytes"] = {"fused_ws": int(ops.query("tag_label_map_ws_bytes", N, C, D)), "fused_outputs": 4 * N * (5 + (C + 31) // 32),
                    "sim": 4 * N * C, "composed_score_buffer": scores.numel() * 4, "composed_unit_rows": 4 * (N + C) * D}
    return res, out


def main(args):
    g = np.random.RandomState(args.n * 31 + args.d)
    x, e = g.randn(args.n, args.d).astype(np.float32), g.randn(args.c, args.d).astype(np.float32)
    result = {"N": args.n, "C": args.c, "D": args.d}
    sk = bench_sklearn(x, e, args.sk_items, args.sk_workers)            # first: its processes are forked before the GPU is opened
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("label_map_bench.py needs the GPU: the HIP path has no CPU fallback")
    dev = torch.device("cuda:0")
    tx, te = torch.from_numpy(x).to(dev), torch.from_numpy(e).to(dev)
    sample = torch.nn.functional.normalize(tx[:2048]) @ torch.nn.functional.normalize(te).T
    th0, th1 = (float(t) for t in torch.quantile(sample.flatten()[:: 4], torch.tensor([0.6, 0.999], device=dev)))
    result["thresholds"] = [th0, th1]
    result["device"], out = bench_device(tx, te, th0, th1, max(args.runs, 20))
    if sk is not None:
        best = sk.pop("best")
        sk["best_differing_from_fused"] = int((best != out["fused"].best[: len(best)].cpu().numpy()).sum())
        sk["speedup_of_fused_sim_over_all_rows"] = sk["ms_for_all_rows"] / result["device"]["fused_sim"]["ms_median"]
    result["sklearn_items"] = sk
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--n", type=int, default=32768)
    parser.add_argument("--c", type=int, default=527)
    parser.add_argument("--d", type=int, default=384)
    parser.add_argument("--runs", type=int, default=20)
    parser.add_argument("--sk_items", type=int, default=4096)
    parser.add_argument("--sk_workers", type=int, default=16)
    parser.add_argument("--out", type=str, default=None)
    return parser


if __name__ == "__main__":
    main(build_parser().parse_args())
