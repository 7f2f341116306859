#!/usr/bin/env python3
"""ops.phrase_sim_count (csrc/phrase_sim.hip) beside the same count composed from what the library already had: ops.gemm of a
row chunk of q against the bank into a (chunk, N) score buffer, then a torch compare-and-weighted-sum of that buffer, over all
chunks.  Device events, every path alternated in one process, one JSON object.  Needs the GPU: there is no fallback.

Paths, all on unit rows prepared once (normalisation is not timed):
  fused          ops.phrase_sim_count(q, bank, weight, thr, normalize=False): no score buffer
  composed_where gemm + torch.where(scores >= thr, weight, 0).sum(1) in int64
  composed_mv    gemm + (scores >= thr).double() @ weight.double() (exact below 2^53), rounded back to int64
  gemm_only      the chunked GEMMs alone: the floor of any composed path
Shapes: M = N = --n (default 32768) with q = bank, and --m (default 128) query rows against the same bank; D = --d (512).
Each path is warmed up, then timed --runs (>= 20) times with the paths interleaved; median, min, max and the quartiles are
reported, the fused result is compared with both composed results, and the fused rate is given as a share of the 157 TFLOP/s
fp32 MFMA peak of the MI355X.

    python tools/phrase_sim_bench.py [--n 32768] [--d 512] [--m 128] [--chunk 4096] [--threshold 0.5] [--runs 20]
                                     [--inner 1] [--only square|few_rows] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP32_MFMA_PEAK_TFLOPS = 157.0


def summary(ts):
    ts = np.asarray(ts)
    return {"ms_median": float(np.median(ts)), "ms_min": float(ts.min()), "ms_max": float(ts.max()),
            "ms_q1": float(np.percentile(ts, 25)), "ms_q3": float(np.percentile(ts, 75)), "runs": int(ts.size)}


def unit_bank(N, D, dev):
    """Seeded rows with every third one a near-duplicate of its predecessor (cosine about 0.98), as unit rows."""
    from texttoaudiogrounding_amd import dispatch
    g = torch.Generator(device=dev).manual_seed(N * 31 + D)
    x = torch.randn(N, D, device=dev, generator=g)
    x[1::3] = x[0::3][: x[1::3].shape[0]] + 0.2 * torch.randn(x[1::3].shape, device=dev, generator=g)
    return dispatch._unit_rows(x, N, D)


def make_paths(q, bank, weight, thr, chunk):
    from texttoaudiogrounding_amd import ops
    M, D = q.shape
    N = bank.shape[0]
    chunk = min(chunk, M)
    scores = torch.empty(chunk, N, device=q.device)
    wd, zero = weight.double(), torch.zeros((), dtype=torch.int64, device=q.device)

    def chunks():
        for r0 in range(0, M, chunk):
            rows = min(chunk, M - r0)
            ops.gemm(q[r0:r0 + rows], bank, rows, N, D, transB=True, out=scores)
            yield r0, rows

    def fused():
        return ops.phrase_sim_count(q, bank, weight, threshold=thr, normalize=False)

    def composed_where():
        out = torch.empty(M, dtype=torch.int64, device=q.device)
        for r0, rows in chunks():
            out[r0:r0 + rows] = torch.where(scores[:rows] >= thr, weight, zero).sum(1)
        return out

    def composed_mv():
        out = torch.empty(M, dtype=torch.int64, device=q.device)
        for r0, rows in chunks():
            out[r0:r0 + rows] = ((scores[:rows] >= thr).double() @ wd).round().long()
        return out

    def gemm_only():
        for _ in chunks():
            pass

    return {"fused": fused, "composed_where": composed_where, "composed_mv": composed_mv, "gemm_only": gemm_only}, scores


def bench(q, bank, weight, a):
    from texttoaudiogrounding_amd import ops
    paths, scores = make_paths(q, bank, weight, a.threshold, a.chunk)
    results = {}
    for name, fn in paths.items():                                # warm-up: code objects, allocator
        for _ in range(3):
            results[name] = fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(a.runs):
        for name, fn in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.inner)
    M, D = q.shape
    N = bank.shape[0]
    res = {k: summary(v) for k, v in times.items()}
    flop = 2.0 * M * N * D
    for k in ("fused", "gemm_only"):
        res[k]["tflops"] = flop / (res[k]["ms_median"] * 1e-3) / 1e12
        res[k]["share_of_fp32_mfma_peak"] = res[k]["tflops"] / FP32_MFMA_PEAK_TFLOPS
    best = min(("composed_where", "composed_mv"), key=lambda k: res[k]["ms_median"])
    res["best_composed"] = best
    res["fused_over_best_composed"] = res["fused"]["ms_median"] / res[best]["ms_median"]
    res["best_composed_spread_ms"] = res[best]["ms_max"] - res[best]["ms_min"]
    res["fused_minus_best_composed_ms"] = res["fused"]["ms_median"] - res[best]["ms_median"]
    res["rows_differing_from_fused"] = {k: int((results[k] != results["fused"]).sum().item())
                                        for k in ("composed_where", "composed_mv")}
    res["count_sum"] = int(results["fused"].sum().item())
    res["bytes"] = {"fused_ws": int(ops.query("tag_phrase_sim_count_ws_bytes", M, N, D)),
                    "composed_score_buffer": scores.numel() * 4}
    res["shape"] = {"M": M, "N": N, "D": D}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--m", type=int, default=128)
    ap.add_argument("--chunk", type=int, default=4096)
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--inner", type=int, default=1, help="calls per timed window (the few-rows shape uses at least 20)")
    ap.add_argument("--only", choices=["square", "few_rows"], default=None, help="time one of the two shapes (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.runs < 20:
        raise SystemExit("--runs must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("phrase_sim_bench.py needs the GPU: the HIP path has no CPU fallback")
    dev = torch.device("cuda:0")
    bank = unit_bank(a.n, a.d, dev)
    weight = torch.randint(1, 1000, (a.n,), generator=torch.Generator().manual_seed(3)).to(dev)
    res = {}
    if a.only != "few_rows":
        res["square"] = bench(bank, bank, weight, a)
    if a.only != "square":
        small = argparse.Namespace(**{**vars(a), "inner": max(a.inner, 20)})   # a window of one call would time the launch
        res["few_rows"] = bench(bank[: a.m].clone(), bank, weight, small)
    res["config"] = vars(a)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
