#!/usr/bin/env python3
"""The fused BERTScore phrase-to-label map (csrc/bertscore.hip: ops.bertscore_map) beside the same result composed from what the
library already had.  Device events, the two legs alternated in one process, one JSON object.  Needs the GPU: there is no fallback.

Legs at N = --n (32768) phrases in slots of --la (16) tokens, C = --c (527) labels in slots of --lb (8), D = --d (768), seeded
unit token vectors, random lengths and weights:
  fused      ops.bertscore_map(..., normalize=False): best, best_f, best_p, best_r; no score array of any kind, slices x N x 16
             bytes of workspace
  composed   row chunks of --chunk (2048) phrases: ops.gemm of the chunk's token rows against all label token rows into a
             (chunk * la, C * lb) token x token buffer, then torch: the length masks, amax over a label's columns and over a
             phrase's rows, the weighted sums, F, argmax and the gathers of F, P, R
Both legs get unit rows (the normalisation is the same launch for both and is left out).  Each leg is warmed up, then timed
--runs (>= 20) times, interleaved; median, min, max and quartiles; the peak device memory of each leg above what the inputs hold;
the fused leg's rate of useful products (2 N la C lb D flop per call) as a share of the fp32 MFMA rate measured on the same
board by the register-resident probe (utils.telemetry.mfma_probe).

    python tools/bertscore_bench.py [--n 32768] [--c 527] [--la 16] [--lb 8] [--d 768] [--chunk 2048] [--runs 20] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(ts):
    ts = np.asarray(ts)
    return {"ms_median": float(np.median(ts)), "ms_min": float(ts.min()), "ms_max": float(ts.max()),
            "ms_q1": float(np.percentile(ts, 25)), "ms_q3": float(np.percentile(ts, 75)), "runs": int(ts.size)}


def make_inputs(args, dev):
    import torch
    g = torch.Generator(device=dev).manual_seed(args.n * 31 + args.d)          # (drawn on the device: 1.6 GB of phrase tokens)

    def side(rows, L):
        x = torch.randn(rows, L, args.d, generator=g, device=dev) + 0.5
        x = x / x.norm(dim=-1, keepdim=True)
        lens = torch.randint(1, L + 1, (rows,), generator=g, device=dev, dtype=torch.int32)
        w = (0.5 + torch.rand(rows, L, generator=g, device=dev)) * (torch.arange(L, device=dev)[None, :] < lens[:, None])
        return x, lens, w
    return side(args.n, args.la) + side(args.c, args.lb)


def composed_leg(a, a_len, a_w, b, b_len, b_w, chunk):
    import torch
    from texttoaudiogrounding_amd import ops
    (N, La, D), (C, Lb, _) = a.shape, b.shape
    dev = a.device
    buf = torch.empty(chunk * La, C * Lb, device=dev)
    ma = torch.arange(La, device=dev)[None, :] < a_len[:, None]                   # (N, La)
    mb = torch.arange(Lb, device=dev)[None, :] < b_len[:, None]                   # (C, Lb)
    wa, wb = (a_w * ma).sum(1), (b_w * mb).sum(1)
    neg = torch.tensor(float("-inf"), device=dev)
    b_rows = b.reshape(C * Lb, D)

    def run():
        best, best_f, best_p, best_r = [], [], [], []
        for r0 in range(0, N, chunk):
            n = min(chunk, N - r0)
            s = ops.gemm(a[r0: r0 + n].reshape(n * La, D), b_rows, n * La, C * Lb, D, transB=True, out=buf[: n * La])
            s = s.view(n, La, C, Lb)
            row_max = torch.where(mb[None, None], s, neg).amax(3)                 # (n, La, C)
            col_max = torch.where(ma[r0: r0 + n, :, None, None], s, neg).amax(1)  # (n, C, Lb)
            aw = (a_w[r0: r0 + n] * ma[r0: r0 + n])[:, :, None]
            P = torch.where(aw != 0, aw * row_max, 0.0).sum(1) / wa[r0: r0 + n, None]
            bw = (b_w * mb)[None]
            R = torch.where(bw != 0, bw * col_max, 0.0).sum(2) / wb[None, :]
            F = torch.where(P + R != 0, 2 * P * R / (P + R), 0.0)
            idx = F.argmax(1, keepdim=True)
            best.append(idx[:, 0])
            best_f.append(F.gather(1, idx)[:, 0])
            best_p.append(P.gather(1, idx)[:, 0])
            best_r.append(R.gather(1, idx)[:, 0])
        return torch.cat(best), torch.cat(best_f), torch.cat(best_p), torch.cat(best_r)
    return run, buf


def bench(args):
    import torch
    from texttoaudiogrounding_amd import ops
    from texttoaudiogrounding_amd.utils.telemetry import mfma_probe
    dev = torch.device("cuda:0")
    a, a_len, a_w, b, b_len, b_w = make_inputs(args, dev)
    N, C, D = args.n, args.c, args.d
    base = torch.cuda.memory_allocated()
    legs, peak, out = {"fused": lambda: ops.bertscore_map(a, a_len, a_w, b, b_len, b_w, normalize=False)}, {}, {}
    torch.cuda.reset_peak_memory_stats()
    for _ in range(3):                                            # warm-up: code objects, allocator
        out["fused"] = legs["fused"]()
    torch.cuda.synchronize()
    peak["fused"] = torch.cuda.max_memory_allocated() - base
    legs["composed"], buf = composed_leg(a, a_len, a_w, b, b_len, b_w, min(args.chunk, N))
    torch.cuda.reset_peak_memory_stats()
    for _ in range(3):
        out["composed"] = legs["composed"]()
    torch.cuda.synchronize()
    peak["composed"] = torch.cuda.max_memory_allocated() - base
    times = {k: [] for k in legs}
    for _ in range(max(args.runs, 20)):
        for name, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
    res = {k: summary(v) for k, v in times.items()}
    for k in legs:
        res[k]["peak_bytes_above_inputs"] = int(peak[k])
        res[k]["spread_ms"] = res[k]["ms_max"] - res[k]["ms_min"]
    sa, sb = ops.bertscore_slot(args.la), ops.bertscore_slot(args.lb)
    ceiling = mfma_probe("f32_random", 50.0)
    flop = 2.0 * N * sa * C * sb * D
    res["fused"]["tflops_of_products"] = flop / (res["fused"]["ms_median"] * 1e-3) / 1e12
    res["fused"]["share_of_measured_fp32_mfma_ceiling"] = res["fused"]["tflops_of_products"] / ceiling["TFLOP/s"]
    res["fused"]["ws_bytes"] = int(ops.query("tag_bertscore_map_ws_bytes", N, C, D, sa, sb))
    res["measured_fp32_mfma_ceiling"] = ceiling
    res["fused_over_composed"] = res["fused"]["ms_median"] / res["composed"]["ms_median"]
    res["composed_token_buffer_bytes"] = buf.numel() * 4
    res["whole_token_matrix_bytes"] = 4 * N * args.la * C * args.lb
    f, c = out["fused"], out["composed"]
    res["best_differing_from_composed"] = int((f.best != c[0]).sum().item())
    res["max_difference_from_composed"] = {k: float((x - y).abs().max().item())
                                           for k, x, y in zip("FPR", (f.best_f, f.best_p, f.best_r), c[1:])}
    return res


def main(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bertscore_bench.py needs the GPU: the HIP path has no CPU fallback")
    result = {"N": args.n, "C": args.c, "La": args.la, "Lb": args.lb, "D": args.d, "chunk": args.chunk}
    result["device"] = bench(args)
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
    parser.add_argument("--la", type=int, default=16)
    parser.add_argument("--lb", type=int, default=8)
    parser.add_argument("--d", type=int, default=768)
    parser.add_argument("--chunk", type=int, default=2048)
    parser.add_argument("--runs", type=int, default=20)
    parser.add_argument("--out", type=str, default=None)
    return parser


if __name__ == "__main__":
    main(build_parser().parse_args())
