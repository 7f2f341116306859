#!/usr/bin/env python3
"""The device average-linkage clustering (csrc/agc.hip) beside what the library already had and beside the reference's host recipe.
Device events for the kernels, wall time for the fits, every path alternated in one process, one JSON object.  Needs the GPU: no
fallback.

At N = --n (32768), D = --d (512), n_clusters = --k (256), on unit rows around --blobs (64) planted means whose per-row noise
level varies plus 10 % unstructured rows (tools/dbscan_bench.py's rows):
  nearest           ops.agc_nearest at the first round's M = N: the marching kernel with the (score, index) epilogue + the fold
  composed_nearest  ops.gemm (2048 rows per call) into an M x M fp32 buffer (4 M^2 bytes), the diagonal set to -inf, torch max
                    over the rows
  merge             ops.agc_merge on the first round's nn (two launches)
  fit               AgglomerativeClustering(k).fit(x), x on the device (wall time, synchronised); its rounds and peak device memory
  composed_fit      the same rounds with composed_nearest in place of ops.agc_nearest (the merge stays ops.agc_merge, the host half
                    the same); its rounds, peak device memory, and the labels that differ.  The composed scores are not
                    bit-symmetric and torch's argmax does not promise the lowest index: a round without a pair ends it
                    ("stalled").
  sklearn_fit       at --sk_n rows (8192: a 4 N^2 = 256 MiB distance matrix): the reference's recipe, sklearn
                    AgglomerativeClustering(linkage="average", metric="precomputed") on 1 - cosine_similarity, on the host's
                    threads; whether the partitions agree with the device fit on the same rows, and the smallest gap among the
                    top k heights (labels are only promised equal where that gap exceeds the fp32 error of a height)
Kernel paths are warmed up, then timed --runs (>= 20) times interleaved; median, min, max and quartiles.

    python tools/agc_bench.py [--n 32768] [--d 512] [--k 256] [--runs 20] [--fit_runs 3] [--sk_n 8192] [--sk_runs 1] [--out FILE.json]
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
CHUNK = 2048


def summary(ts):
    ts = np.asarray(ts)
    return {"ms_median": float(np.median(ts)), "ms_min": float(ts.min()), "ms_max": float(ts.max()),
            "ms_q1": float(np.percentile(ts, 25)), "ms_q3": float(np.percentile(ts, 75)), "runs": int(ts.size)}


def make_rows(N, D, blobs, dev):
    g = torch.Generator(device=dev).manual_seed(N * 31 + D)
    means = torch.randn(blobs, D, device=dev, generator=g)
    level = 0.5 + 0.9 * torch.rand(N, 1, device=dev, generator=g)
    x = means[torch.randint(blobs, (N,), device=dev, generator=g)] + level * torch.randn(N, D, device=dev, generator=g)
    loose = torch.rand(N, device=dev, generator=g) < 0.1
    x[loose] = torch.randn(int(loose.sum()), D, device=dev, generator=g)
    return (x / x.norm(dim=1, keepdim=True)).contiguous()


def composed_nearest(m, scores):
    """(nn int32, dist fp32) from ops.gemm and torch on the first M * M floats of ``scores``."""
    from texttoaudiogrounding_amd import ops
    M, D = m.shape
    s = scores[:M * M].view(M, M)
    for r0 in range(0, M, CHUNK):                                  # (row chunks: one product's output stays below 2^31 bytes)
        n = min(CHUNK, M - r0)
        ops.gemm(m[r0:r0 + n], m, n, M, D, transB=True, out=s[r0:r0 + n])
    s.fill_diagonal_(float("-inf"))
    best, nn = s.max(1)
    return nn.int(), 1.0 - best


def fit_rounds(x, nearest, profile=False):
    """The rounds of AgglomerativeClustering.fit with ``nearest`` for the first step -> (log_dist, log_ids, rounds, stalled[, the
    per-round device times of both steps and the cluster counts])."""
    from texttoaudiogrounding_amd import ops
    N, D = x.shape
    dev = x.device
    means = x.clone()
    sums, sizes, ids = means.double(), torch.ones(N, device=dev, dtype=torch.int64), torch.arange(N, device=dev, dtype=torch.int32)
    sums2, sizes2, ids2 = torch.empty_like(sums), torch.empty_like(sizes), torch.empty_like(ids)
    log_dist = torch.empty(N - 1, device=dev, dtype=torch.float32)
    log_ids = torch.empty(N - 1, 3, device=dev, dtype=torch.int32)
    counts = torch.empty(2, device=dev, dtype=torch.int32)
    M, rounds, stalled = N, 0, False
    prof = {"nearest_ms": [], "merge_ms": [], "M": []}
    while M > 1:
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if profile else None
        if profile:
            ev[0].record()
        nn, dist = nearest(means[:M])
        if profile:
            ev[1].record()
        ops.agc_merge(nn, dist, sums, sizes, ids, sums2, sizes2, ids2, means, log_dist, log_ids, counts, log_off=N - M, next_id=2 * N - M)
        if profile:
            ev[2].record()
        pairs, new_m = counts.tolist()
        if profile:
            torch.cuda.synchronize()
            prof["nearest_ms"].append(ev[0].elapsed_time(ev[1]))
            prof["merge_ms"].append(ev[1].elapsed_time(ev[2]))
            prof["M"].append(M)
        if pairs < 1:
            stalled = True
            break
        sums, sums2, sizes, sizes2, ids, ids2 = sums2, sums, sizes2, sizes, ids2, ids
        M = new_m
        rounds += 1
    return (log_dist, log_ids, rounds, stalled, prof) if profile else (log_dist, log_ids, rounds, stalled)


def bench_kernels(x, runs):
    from texttoaudiogrounding_amd import ops
    N, D = x.shape
    dev = x.device
    scores = torch.empty(N * N, device=dev)
    nn, dist = ops.agc_nearest(x)
    sums, sizes, ids = x.double(), torch.ones(N, device=dev, dtype=torch.int64), torch.arange(N, device=dev, dtype=torch.int32)
    sums2, sizes2, ids2, means2 = torch.empty_like(sums), torch.empty_like(sizes), torch.empty_like(ids), torch.empty_like(x)
    log_dist, log_ids = torch.empty(N - 1, device=dev), torch.empty(N - 1, 3, device=dev, dtype=torch.int32)
    counts = torch.empty(2, device=dev, dtype=torch.int32)
    paths = {"nearest": lambda: ops.agc_nearest(x),
             "composed_nearest": lambda: composed_nearest(x, scores),
             "merge": lambda: ops.agc_merge(nn, dist, sums, sizes, ids, sums2, sizes2, ids2, means2, log_dist, log_ids, counts, 0, N)}
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
    res = {k: summary(v) for k, v in times.items()}
    for k in ("nearest", "composed_nearest"):
        res[k]["tflops"] = 2.0 * N * N * D / (res[k]["ms_median"] * 1e-3) / 1e12
        res[k]["share_of_fp32_mfma_peak"] = res[k]["tflops"] / FP32_MFMA_PEAK_TFLOPS
    res["nearest_over_composed"] = res["nearest"]["ms_median"] / res["composed_nearest"]["ms_median"]
    res["nn_differing_from_composed"] = int((out["nearest"][0] != out["composed_nearest"][0]).sum())
    res["largest_dist_difference_from_composed"] = float((out["nearest"][1] - out["composed_nearest"][1]).abs().max())
    res["first_round_pairs"] = int(counts[0])
    res["bytes"] = {"nearest_ws": int(ops.query("tag_agc_nearest_ws_bytes", N, D)), "merge_ws": int(ops.query("tag_agc_merge_ws_bytes", N, D)),
                    "composed_scores": 4 * N * N}
    return res


def bench_fits(x, k, runs):
    from texttoaudiogrounding_amd import ops
    from texttoaudiogrounding_amd.utils.phrase_cluster import AgglomerativeClustering
    N, D = x.shape
    times = {"fit": [], "composed_fit": []}
    peak, composed = {}, None
    for r in range(runs + 1):
        for name in times:
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            if name == "fit":
                model = AgglomerativeClustering(k, device=x.device).fit(x)
            else:
                scores = torch.empty(N * N, device=x.device)
                log_dist, log_ids, rounds, stalled = fit_rounds(x, lambda m: composed_nearest(m, scores))
                if not stalled:
                    log = log_ids.cpu().numpy()
                    composed = AgglomerativeClustering(k)._set_tree(log_dist.cpu().numpy(), log[:, 0], log[:, 1], N, rounds)
                del scores
            torch.cuda.synchronize()
            if r >= 1:
                times[name].append((time.perf_counter() - t0) * 1e3)
            peak[name] = int(torch.cuda.max_memory_allocated() - base)
    res = {"fit": dict(summary(times["fit"]), n_rounds=model.n_rounds_, n_clusters=k, peak_device_bytes=peak["fit"],
                       peak_over_20ND=peak["fit"] / (20.0 * N * D), distance_matrix_bytes=4 * N * N,
                       smallest_gap_among_top_k_heights=float(np.diff(model.distances_[-k:]).min()),
                       height_error_bound=(D + 6) * 2.0 ** -24)}
    res["composed_fit"] = dict(summary(times["composed_fit"]), n_rounds=rounds, stalled=bool(stalled), peak_device_bytes=peak["composed_fit"])
    if composed is not None:
        res["composed_fit"]["labels_differing_from_fit"] = int((composed.labels_ != model.labels_).sum())
        res["composed_fit"]["largest_height_difference_from_fit"] = float(np.abs(composed.distances_ - model.distances_).max())
    res["fit_over_composed"] = res["fit"]["ms_median"] / res["composed_fit"]["ms_median"]
    # where the time goes: device events around the two steps of every round of one more fit, and the host half on its own
    log_dist, log_ids, rounds, _, prof = fit_rounds(x, ops.agc_nearest, profile=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    log = log_ids.cpu().numpy()
    again = AgglomerativeClustering(k)._set_tree(log_dist.cpu().numpy(), log[:, 0], log[:, 1], N, rounds)
    host_ms = (time.perf_counter() - t0) * 1e3
    res["fit"]["where_the_time_goes"] = {"nearest_ms_sum": float(sum(prof["nearest_ms"])), "merge_ms_sum": float(sum(prof["merge_ms"])),
                                         "log_copy_and_host_half_ms": host_ms, "clusters_per_round": prof["M"],
                                         "nearest_ms_per_round": [round(v, 3) for v in prof["nearest_ms"]],
                                         "labels_equal_fit": bool(np.array_equal(again.labels_, model.labels_))}
    return res


def same_partition(a, b):
    """Equal up to the names of the labels."""
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


def bench_sklearn(x, n, k, runs):
    from texttoaudiogrounding_amd.utils.phrase_cluster import AgglomerativeClustering
    try:
        from sklearn.cluster import AgglomerativeClustering as SkAgc
        from sklearn.metrics.pairwise import cosine_similarity
    except ImportError:
        return "skipped: sklearn is not importable"
    sub = x[:n].contiguous()
    xh = sub.cpu().numpy()
    ts, td = [], []
    for r in range(runs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model = AgglomerativeClustering(k, device=x.device).fit(sub)
        torch.cuda.synchronize()
        if r >= 1:
            td.append((time.perf_counter() - t0) * 1e3)
    for r in range(runs):
        t0 = time.perf_counter()
        distances = 1 - cosine_similarity(xh, xh)
        sk = SkAgc(n_clusters=k, linkage="average", metric="precomputed").fit(distances)
        ts.append((time.perf_counter() - t0) * 1e3)
    res = {"N": n, "n_clusters": k, "distance_matrix_bytes": 4 * n * n, "fit": summary(td), "sklearn_fit": summary(ts),
           "threads": os.cpu_count(), "omp_num_threads": os.environ.get("OMP_NUM_THREADS"), "n_rounds": model.n_rounds_,
           "labels_differing_from_sklearn": int((sk.labels_ != model.labels_).sum()),
           "same_partition_as_sklearn": bool(same_partition(sk.labels_, model.labels_)),
           "smallest_gap_among_top_k_heights": float(np.diff(model.distances_[-k:]).min()),
           "height_error_bound": (x.shape[1] + 6) * 2.0 ** -24}
    res["fit_over_sklearn"] = res["fit"]["ms_median"] / res["sklearn_fit"]["ms_median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--k", type=int, default=256)
    ap.add_argument("--blobs", type=int, default=64)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--fit_runs", type=int, default=3)
    ap.add_argument("--sk_n", type=int, default=8192)
    ap.add_argument("--sk_runs", type=int, default=1)
    ap.add_argument("--only", choices=["kernels", "fits", "sklearn"], default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.runs < 20:
        raise SystemExit("--runs must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("agc_bench.py needs the GPU: the HIP path has no CPU fallback")
    dev = torch.device("cuda:0")
    x = make_rows(a.n, a.d, a.blobs, dev)
    res = {"shape": {"N": a.n, "D": a.d, "n_clusters": a.k, "blobs": a.blobs}, "device": torch.cuda.get_device_name(0)}
    if a.only in (None, "kernels"):
        res["kernels"] = {"pass_1": bench_kernels(x, a.runs), "pass_2": bench_kernels(x, a.runs)}
    if a.only in (None, "fits"):
        res["fits"] = bench_fits(x, min(a.k, a.n), a.fit_runs)
    if a.only in (None, "sklearn"):
        res["sklearn"] = bench_sklearn(x, min(a.sk_n, a.n), min(a.k, a.sk_n, a.n), a.sk_runs)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
