#!/usr/bin/env python3
"""The device DBSCAN (csrc/dbscan.hip) beside what the library already had and beside the reference's host recipe.  Device events
for the kernels, wall time for the fits, every path alternated in one process, one JSON object.  Needs the GPU: no fallback.

At N = --n (32768), D = --d (512), eps 0.5, min_samples 5, on unit rows around --blobs (64) planted means whose per-row noise
level varies (tight rows are core, loose ones border or noise) plus 10 % unstructured rows (noise):
  graph          ops.dbscan_graph(x, normalize=False): the marching kernel with the ballot epilogue + the popcount launch
  sim_count      ops.phrase_sim_count(x, x, threshold=0.5, normalize=False): the same products, int64 counts instead of bits
  hook           one ops.dbscan_hook pass from f = 0 .. N - 1 (the densest pass: no row has converged)
  fit            DBSCAN().fit(x), x on the device (wall time, synchronised); its passes
  composed_fit   ops.gemm row chunks (--chunk rows) -> compare into a boolean N x N -> degrees, core flags, the same FastSV
                 passes and the border rule in torch on that matrix, chunk by chunk; its peak device memory beside N^2 / 8 bytes
  sklearn_fit    at --sk_n rows (8192: a 4 N^2 = 256 MiB distance matrix): the reference's recipe, sklearn
                 DBSCAN(metric="precomputed") on (1 - cosine_similarity).clip(0), on the host's threads; label agreement with
                 DBSCAN().fit on the same rows and the number of pairs inside the gap of tests/dbscan_ref.py
Kernel paths are warmed up, then timed --runs (>= 20) times interleaved; median, min, max and quartiles.

    python tools/dbscan_bench.py [--n 32768] [--d 512] [--runs 20] [--fit_runs 5] [--sk_n 8192] [--sk_runs 2] [--out FILE.json]
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
EPS, MIN_SAMPLES = 0.5, 5


def summary(ts):
    ts = np.asarray(ts)
    return {"ms_median": float(np.median(ts)), "ms_min": float(ts.min()), "ms_max": float(ts.max()),
            "ms_q1": float(np.percentile(ts, 25)), "ms_q3": float(np.percentile(ts, 75)), "runs": int(ts.size)}


def make_rows(N, D, blobs, dev):
    g = torch.Generator(device=dev).manual_seed(N * 31 + D)
    means = torch.randn(blobs, D, device=dev, generator=g)
    level = 0.5 + 0.9 * torch.rand(N, 1, device=dev, generator=g)              # cosine of two rows of a blob: 1 / sqrt((1 + a^2)(1 + b^2))
    x = means[torch.randint(blobs, (N,), device=dev, generator=g)] + level * torch.randn(N, D, device=dev, generator=g)
    loose = torch.rand(N, device=dev, generator=g) < 0.1
    x[loose] = torch.randn(int(loose.sum()), D, device=dev, generator=g)
    return (x / x.norm(dim=1, keepdim=True)).contiguous()


def bench_kernels(x, runs):
    from texttoaudiogrounding_amd import ops
    N, D = x.shape
    adj, degree = ops.dbscan_graph(x, eps=EPS, normalize=False)
    core_bits = ops.dbscan_core(degree, MIN_SAMPLES)
    f0 = torch.arange(N, device=x.device, dtype=torch.int32)
    g, changed = torch.empty_like(f0), torch.empty(1, device=x.device, dtype=torch.int32)
    paths = {"graph": lambda: ops.dbscan_graph(x, eps=EPS, normalize=False),
             "sim_count": lambda: ops.phrase_sim_count(x, x, threshold=1.0 - EPS, normalize=False),
             "hook": lambda: ops.dbscan_hook(adj, core_bits, f0, g, changed, check=False)}
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
    for k in ("graph", "sim_count"):
        res[k]["tflops"] = 2.0 * N * N * D / (res[k]["ms_median"] * 1e-3) / 1e12
        res[k]["share_of_fp32_mfma_peak"] = res[k]["tflops"] / FP32_MFMA_PEAK_TFLOPS
    res["graph_over_sim_count"] = res["graph"]["ms_median"] / res["sim_count"]["ms_median"]
    res["degree_equals_sim_count"] = bool(torch.equal(out["graph"][1].long(), out["sim_count"]))
    res["adjacency_density"] = float(degree.double().mean().item() / N)
    res["core_rows"] = int((degree >= MIN_SAMPLES).sum().item())
    res["bytes"] = {"adj": adj.numel() * 4, "sim_count_ws": int(ops.query("tag_phrase_sim_count_ws_bytes", N, N, D))}
    return res


def composed_fit(x, chunk):
    """The same labels from ops.gemm and torch on a boolean N x N."""
    from texttoaudiogrounding_amd import ops
    N, D = x.shape
    big = torch.iinfo(torch.int64).max
    adj = torch.empty(N, N, device=x.device, dtype=torch.bool)
    scores = torch.empty(chunk, N, device=x.device)
    degree = torch.empty(N, device=x.device, dtype=torch.int64)
    for r0 in range(0, N, chunk):
        n = min(chunk, N - r0)
        ops.gemm(x[r0:r0 + n], x, n, N, D, transB=True, out=scores[:n])
        torch.ge(scores[:n], 1.0 - EPS, out=adj[r0:r0 + n])
        degree[r0:r0 + n] = adj[r0:r0 + n].sum(1)                   # (per chunk: a sum over the whole matrix widens all of it to int64)
    core = degree >= MIN_SAMPLES
    idx = torch.nonzero(core).flatten()

    def masked_min(values, rows):                                   # min of values[j] over the core neighbours j of each row
        out = torch.full((rows.numel(),), big, device=x.device, dtype=torch.int64)
        for r0 in range(0, rows.numel(), chunk):
            r = rows[r0:r0 + chunk]
            out[r0:r0 + chunk] = torch.where(adj[r] & core[None, :], values[None, :], big).min(1).values
        return out

    f = torch.arange(N, device=x.device)
    passes = 0
    while True:
        gf = f[f]
        m = masked_min(gf, idx)
        new = torch.minimum(f, gf)
        new.scatter_reduce_(0, f[idx], m, reduce="amin")
        new[idx] = torch.minimum(new[idx], m)
        passes += 1
        if torch.equal(new, f):
            break
        f = new
    rest = torch.nonzero(~core).flatten()
    root = f.clone()
    cand = masked_min(f, rest)
    root[rest] = torch.where(cand == big, torch.full_like(cand, -1), cand)
    roots = torch.unique(root[root >= 0])
    labels = torch.where(root >= 0, torch.searchsorted(roots, root.clamp(min=0)), torch.full_like(root, -1))
    return labels, passes


def bench_fits(x, runs, chunk):
    from texttoaudiogrounding_amd.utils.phrase_cluster import DBSCAN
    N = x.shape[0]
    res = {}
    times = {"fit": [], "composed_fit": []}
    peak = {}
    for r in range(runs + 1):
        for name in times:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            if name == "fit":
                model = DBSCAN(EPS, MIN_SAMPLES, device=x.device).fit(x)
            else:
                labels, passes = composed_fit(x, chunk)
            torch.cuda.synchronize()
            if r >= 1:
                times[name].append((time.perf_counter() - t0) * 1e3)
            peak[name] = int(torch.cuda.max_memory_allocated() - base)
    lab = model.labels_
    res["fit"] = dict(summary(times["fit"]), n_passes=model.n_passes_, clusters=int(lab.max() + 1), noise_rows=int((lab < 0).sum()),
                      core_rows=int(model.core_sample_indices_.size), peak_device_bytes=peak["fit"], adj_bytes=N * 4 * 4 * ((N + 127) // 128))
    core = np.zeros(N, dtype=bool)
    core[model.core_sample_indices_] = True
    res["fit"]["border_rows"] = int(((lab >= 0) & ~core).sum())
    res["composed_fit"] = dict(summary(times["composed_fit"]), n_passes=passes, peak_device_bytes=peak["composed_fit"], chunk_rows=chunk,
                               labels_differing_from_fit=int((labels.cpu().numpy() != lab).sum()))
    res["fit_over_composed"] = res["fit"]["ms_median"] / res["composed_fit"]["ms_median"]
    return res


def bench_sklearn(x, n, runs):
    from texttoaudiogrounding_amd.utils.phrase_cluster import DBSCAN
    try:
        from sklearn.cluster import DBSCAN as SkDBSCAN
        from sklearn.metrics.pairwise import cosine_similarity
    except ImportError:
        return "skipped: sklearn is not importable"
    sub = x[:n].contiguous()
    xh = sub.cpu().numpy()
    ts, td = [], []
    for r in range(runs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model = DBSCAN(EPS, MIN_SAMPLES, device=x.device).fit(sub)
        torch.cuda.synchronize()
        if r >= 1:
            td.append((time.perf_counter() - t0) * 1e3)
    for r in range(runs):
        t0 = time.perf_counter()
        distances = (1 - cosine_similarity(xh, xh)).clip(0.0)
        sk = SkDBSCAN(metric="precomputed").fit(distances)
        ts.append((time.perf_counter() - t0) * 1e3)
    u = xh.astype(np.float64)
    u /= np.maximum(np.sqrt((u * u).sum(1, keepdims=True)), 1e-12)
    inside = 0
    for r0 in range(0, n, 2048):
        c = np.abs(u[r0:r0 + 2048] @ u.T - (1.0 - EPS)) < 2.5e-4
        inside += int(c.sum())
    res = {"N": n, "distance_matrix_bytes": 4 * n * n, "fit": summary(td), "sklearn_fit": summary(ts), "threads": os.cpu_count(),
           "omp_num_threads": os.environ.get("OMP_NUM_THREADS"),
           "labels_differing_from_sklearn": int((sk.labels_ != model.labels_).sum()),
           "core_rows_differing": int(np.setxor1d(sk.core_sample_indices_, model.core_sample_indices_).size),
           "ordered_pairs_inside_the_gap": inside, "clusters": int(sk.labels_.max() + 1), "noise_rows": int((sk.labels_ < 0).sum())}
    res["fit_over_sklearn"] = res["fit"]["ms_median"] / res["sklearn_fit"]["ms_median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--blobs", type=int, default=64)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--fit_runs", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=2048)
    ap.add_argument("--sk_n", type=int, default=8192)
    ap.add_argument("--sk_runs", type=int, default=2)
    ap.add_argument("--only", choices=["kernels", "fits", "sklearn"], default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.runs < 20:
        raise SystemExit("--runs must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("dbscan_bench.py needs the GPU: the HIP path has no CPU fallback")
    dev = torch.device("cuda:0")
    x = make_rows(a.n, a.d, a.blobs, dev)
    res = {"shape": {"N": a.n, "D": a.d, "blobs": a.blobs, "eps": EPS, "min_samples": MIN_SAMPLES}, "device": torch.cuda.get_device_name(0)}
    if a.only in (None, "kernels"):
        res["kernels"] = {"pass_1": bench_kernels(x, a.runs), "pass_2": bench_kernels(x, a.runs)}
    if a.only in (None, "fits"):
        res["fits"] = bench_fits(x, a.fit_runs, a.chunk)
    if a.only in (None, "sklearn"):
        res["sklearn"] = bench_sklearn(x, min(a.sk_n, a.n), a.sk_runs)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
