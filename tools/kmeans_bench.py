#!/usr/bin/env python3
"""One Lloyd iteration of the device k-means (csrc/kmeans.hip: ops.kmeans_assign + ops.kmeans_update) beside the same step
composed from what the library already had, and a whole fit beside sklearn on the host.  Device events for the steps, wall
time for the fits, every path alternated in one process, one JSON object.  Needs the GPU: there is no fallback.

Paths at N = --n (32768), D = --d (512), K in --k (32, 256), on rows around --blobs (64) planted means:
  fused_step     ops.kmeans_assign(x, c) + ops.kmeans_update(x, label, c): K floats + slices x K x (D + 1) words of workspace
  fused_assign   the assignment alone (||c||^2, the marching kernel, dist2)
  fused_update   the update alone (the one-hot MFMA reduction and its fp64 fold)
  composed_step  ops.gemm(x, c^T) into an (N, K) buffer, ||c||^2 - 2 x.c and torch argmin over it, dist2 from gathered centres,
                 then zeros(K, D).index_add_(0, label, x) (fp32 atomics: not reproducible), bincount and the division
  fit            KMeans(K, init=rows, max_iter=--iters, tol=0).fit(x) with x on the device (wall time, synchronised)
  sklearn_fit    sklearn.cluster.KMeans(init=the same rows, n_init=1, max_iter=--iters, tol=0, algorithm="lloyd") on the host's
                 threads (skipped when sklearn is not importable); --sk_runs timed runs
Each step path is warmed up, then timed --runs (>= 20) times with the paths interleaved; median, min, max and quartiles.

    python tools/kmeans_bench.py [--n 32768] [--d 512] [--k 32 256] [--runs 20] [--iters 20] [--sk_runs 3] [--only steps|fits]
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

FP32_MFMA_PEAK_TFLOPS = 157.0


def summary(ts):
    ts = np.asarray(ts)
    return {"ms_median": float(np.median(ts)), "ms_min": float(ts.min()), "ms_max": float(ts.max()),
            "ms_q1": float(np.percentile(ts, 25)), "ms_q3": float(np.percentile(ts, 75)), "runs": int(ts.size)}


def make_rows(N, D, blobs, dev):
    g = torch.Generator(device=dev).manual_seed(N * 31 + D)
    means = torch.randn(blobs, D, device=dev, generator=g)
    x = means[torch.randint(blobs, (N,), device=dev, generator=g)] + 0.7 * torch.randn(N, D, device=dev, generator=g)
    return x / x.norm(dim=1, keepdim=True)


def step_paths(x, init):
    from texttoaudiogrounding_amd import ops
    N, D = x.shape
    K = init.shape[0]
    scores = torch.empty(N, K, device=x.device)
    state = {}

    def fused_assign():
        state["label"], state["dist2"] = ops.kmeans_assign(x, init)
        return state["label"]

    def fused_update():
        c = init.clone()
        ops.kmeans_update(x, state["label"], c, check_labels=False)
        return c

    def fused_step():
        c = init.clone()
        label, dist2 = ops.kmeans_assign(x, c)
        ops.kmeans_update(x, label, c, check_labels=False)
        return label, c

    def composed_step():
        c = init.clone()
        ops.gemm(x, c, N, K, D, transB=True, out=scores)
        label = torch.argmin((c * c).sum(1)[None, :] - 2.0 * scores, dim=1)
        dist2 = ((x - c[label]) ** 2).sum(1)
        sums = torch.zeros(K, D, device=x.device).index_add_(0, label, x)
        count = torch.bincount(label, minlength=K)
        live = count > 0
        c[live] = sums[live] / count[live, None]
        return label, c, dist2

    return {"fused_assign": fused_assign, "fused_update": fused_update, "fused_step": fused_step,
            "composed_step": composed_step}, scores


def bench_steps(x, init, runs):
    from texttoaudiogrounding_amd import ops
    paths, scores = step_paths(x, init)
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
    N, D = x.shape
    K = init.shape[0]
    res = {k: summary(v) for k, v in times.items()}
    for k in ("fused_assign", "fused_update"):
        res[k]["tflops"] = 2.0 * N * K * D / (res[k]["ms_median"] * 1e-3) / 1e12
        res[k]["share_of_fp32_mfma_peak"] = res[k]["tflops"] / FP32_MFMA_PEAK_TFLOPS
    res["fused_over_composed"] = res["fused_step"]["ms_median"] / res["composed_step"]["ms_median"]
    res["composed_spread_ms"] = res["composed_step"]["ms_max"] - res["composed_step"]["ms_min"]
    res["labels_differing_from_fused"] = int((out["composed_step"][0] != out["fused_step"][0]).sum().item())
    res["max_centre_difference"] = float((out["composed_step"][1] - out["fused_step"][1]).abs().max().item())
    res["bytes"] = {"fused_assign_ws": int(ops.query("tag_kmeans_assign_ws_bytes", N, K, D)),
                    "fused_update_ws": int(ops.query("tag_kmeans_update_ws_bytes", N, K, D)),
                    "composed_score_buffer": scores.numel() * 4}
    return res


def bench_fit(x, init, iters, runs, sk_runs):
    from texttoaudiogrounding_amd.utils.phrase_cluster import KMeans
    K = init.shape[0]
    res = {}
    ts = []
    for r in range(runs + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        km = KMeans(K, init=init, max_iter=iters, tol=0.0, device=x.device).fit(x)
        torch.cuda.synchronize()
        if r >= 2:
            ts.append((time.perf_counter() - t0) * 1e3)
    res["fit"] = dict(summary(ts), n_iter=km.n_iter_, inertia=km.inertia_)
    try:
        from sklearn.cluster import KMeans as SkKMeans
    except ImportError:
        res["sklearn_fit"] = "skipped: sklearn is not importable"
        return res
    xh, ih = x.cpu().numpy(), init.cpu().numpy()
    ts = []
    for r in range(sk_runs + 1):
        t0 = time.perf_counter()
        sk = SkKMeans(n_clusters=K, init=ih, n_init=1, max_iter=iters, tol=0.0, algorithm="lloyd").fit(xh)
        if r >= 1:
            ts.append((time.perf_counter() - t0) * 1e3)
    res["sklearn_fit"] = dict(summary(ts), n_iter=int(sk.n_iter_), inertia=float(sk.inertia_), threads=os.cpu_count(),
                              omp_num_threads=os.environ.get("OMP_NUM_THREADS"))
    res["labels_differing_from_sklearn"] = int((sk.labels_ != km.labels_).sum())
    res["fit_over_sklearn"] = res["fit"]["ms_median"] / res["sklearn_fit"]["ms_median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--k", type=int, nargs="+", default=[32, 256])
    ap.add_argument("--blobs", type=int, default=64)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sk_runs", type=int, default=3)
    ap.add_argument("--only", choices=["steps", "fits"], default=None, help="time the steps or the fits alone (steps: for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.runs < 20:
        raise SystemExit("--runs must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("kmeans_bench.py needs the GPU: the HIP path has no CPU fallback")
    dev = torch.device("cuda:0")
    x = make_rows(a.n, a.d, a.blobs, dev)
    g = torch.Generator(device=dev).manual_seed(5)
    inits = {K: x[torch.randperm(a.n, device=dev, generator=g)[:K]].clone() for K in a.k}
    res = {"shape": {"N": a.n, "D": a.d, "blobs": a.blobs}, "device": torch.cuda.get_device_name(0), "steps": {}, "fits": {}}
    rounds = {K: [] for K in a.k}
    # the K values alternate as well: two passes of --runs each
    for half in range(2 if a.only != "fits" else 0):
        for K in a.k:
            rounds[K].append(bench_steps(x, inits[K], a.runs))
    for K in a.k:
        if a.only != "fits":
            res["steps"][str(K)] = {"pass_1": rounds[K][0], "pass_2": rounds[K][1]}
        if a.only != "steps":
            res["fits"][str(K)] = bench_fit(x, inits[K], a.iters, a.runs, a.sk_runs)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
