#!/usr/bin/env python3
"""The text intra-attention (IntraAttention, csrc/text_intra.hip), timed with device events, everything alternated in one process.
Prints one JSON object.

--mode kernel (default): for each (R, L, E) of --shapes the row-local core tag_text_intra_forward / _backward (p = 0 and p = 0.2),
  the four element-wise launches of the ConvGRU cell and, for scale, one gate product ([message ; x] @ W^T as two tag_gemm calls),
  on preallocated buffers, with the bytes each pass must move and the rate that gives.
--mode step: BiEncoder(Cnn8Rnn, IntraAttention(EmbeddingLayer(5221, 512), 2), DotProduct) through StrongRunner.train_step at
  B x 10 s against the same model with EmbeddingAgg(5221, 512); median / min / max, difference and ratio.

    python tools/text_intra_bench.py [--mode kernel|step] [--shapes 1024x10x512,1024x33x512] [--rounds 5] [--iters 100]
                                     [--B 64] [--L 8] [--steps 5] [--out FILE.json]

Per-kernel times: a separate profiler run with few iterations, e.g.
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/text_intra_bench.py --rounds 1 --iters 3
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pass_bytes(R, L, E):
    """Bytes a pass must move (x, message, ... are (R, L, E) tensors ``t``; attn is (R, L, L); pe is shared by all rows)."""
    t, attn = 4.0 * R * L * E, 4.0 * R * L * L
    return {"core_forward": 2 * t + attn,                  # reads x, writes message and attn
            "core_backward": 3 * t + attn,                 # reads dmessage, x, attn, writes dx
            "gates_forward": 6 * t,                        # u, r read and written, x read, xr written
            "update_forward": 5 * t,                       # o read and written, u, x read, xnew written
            "update_backward": 7 * t,                      # dnew, x, u, o read, do_pre, du_pre, dx written
            "gates_backward": 6 * t}                       # dxr, x, r, dx read, dr_pre, dx written


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def summary(ts):
    return {"ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts))}


def _time_alternating(fns, rounds, iters):
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n in fns}
    for _ in range(rounds):
        for n, fn in fns.items():
            times[n].append(timed(fn, iters))
    return {n: summary(t) for n, t in times.items()}


def kernel_fns(R, L, E, dev):
    """Closures over preallocated buffers."""
    from texttoaudiogrounding_amd import dispatch
    from texttoaudiogrounding_amd.lib import call, ptr
    from tests.text_selfattn_ref import position_table
    g = torch.Generator().manual_seed(R + L + E)
    M = R * L
    x = (0.2 * torch.randn(R, L, E, generator=g)).to(dev)
    pe = position_table(E)[0].to(dev)
    lens = torch.randint(1, L + 1, (R,), generator=g).to(dev)
    w = (torch.randn(E, 2 * E, generator=g) / (2 * E) ** 0.5).to(dev)
    b = torch.zeros(E, device=dev)
    t = {k: torch.randn(M, E, generator=g).to(dev) for k in ("u", "r", "o", "dnew", "dxr", "dmsg")}
    out = {k: torch.empty(M, E, device=dev) for k in ("msg", "xr", "xnew", "do_pre", "du_pre", "dr_pre", "dx", "dxc", "gate")}
    attn = torch.empty(R, L, L, device=dev)

    def core_fwd(p):
        return lambda: call("tag_text_intra_forward", ptr(x), ptr(pe), ptr(lens), ptr(out["msg"]), ptr(attn), R, L, E, p, 11, 12)

    def core_bwd(p):
        return lambda: call("tag_text_intra_backward", ptr(t["dmsg"]), ptr(x), ptr(pe), ptr(attn), ptr(lens), ptr(out["dxc"]), 0, R, L,
                            E, p, 11, 12)

    def gate():
        dispatch.gemm(out["msg"], w, M, E, E, transB=True, ldb=2 * E, bias=b, out=out["gate"])
        dispatch.gemm(x, w[:, E:], M, E, E, transB=True, ldb=2 * E, out=out["gate"], accumulate=True)

    return {
        "core_forward": core_fwd(0.0), "core_backward": core_bwd(0.0),
        "core_forward_p02": core_fwd(0.2), "core_backward_p02": core_bwd(0.2),
        # u, r, o are squashed in place again at every call: the values change, the work does not
        "gates_forward": lambda: call("tag_convgru_gates_forward", ptr(t["u"]), ptr(t["r"]), ptr(x), ptr(out["xr"]), M, E),
        "update_forward": lambda: call("tag_convgru_update_forward", ptr(t["o"]), ptr(t["u"]), ptr(x), ptr(out["xnew"]), ptr(lens),
                                       None, R, L, E),
        "update_backward": lambda: call("tag_convgru_update_backward", ptr(t["dnew"]), None, ptr(lens), ptr(x), ptr(t["u"]), ptr(t["o"]),
                                        ptr(out["do_pre"]), ptr(out["du_pre"]), ptr(out["dx"]), R, L, E),
        "gates_backward": lambda: call("tag_convgru_gates_backward", ptr(t["dxr"]), ptr(x), ptr(t["r"]), ptr(out["dr_pre"]),
                                       ptr(out["dx"]), M, E),
        "one_gate_product": gate,
    }


def bench_kernel(a, dev):
    from texttoaudiogrounding_amd import dispatch
    res = {}
    for shape in a.shapes.split(","):
        R, L, E = (int(v) for v in shape.split("x"))
        r = _time_alternating(kernel_fns(R, L, E, dev), a.rounds, a.iters)
        dispatch.check_async_errors()
        for k, nb in pass_bytes(R, L, E).items():
            r[f"{k}_bytes"] = nb
            r[f"{k}_GBps"] = nb / (r[k]["ms_median"] * 1e-3) / 1e9
        r["one_gate_product_GFLOP"] = 2.0 * R * L * E * 2 * E / 1e9
        r["layer_forward_ms"] = (r["core_forward"]["ms_median"] + 3 * r["one_gate_product"]["ms_median"]
                                 + r["gates_forward"]["ms_median"] + r["update_forward"]["ms_median"])
        r["core_share_of_layer_forward"] = r["core_forward"]["ms_median"] / r["layer_forward_ms"]
        res[shape] = r
    return res


def bench_step(a, dev):
    from oracle import tag_oracle as O
    from texttoaudiogrounding_amd.models import audio_encoder, audio_text_model, match, text_encoder
    from texttoaudiogrounding_amd.runner import StrongRunner
    torch.manual_seed(0)
    encoders = {"intra": text_encoder.IntraAttention(text_encoder.EmbeddingLayer(5221, 512), 2),
                "agg": text_encoder.EmbeddingAgg(5221, 512)}
    runners = {n: StrongRunner(audio_text_model.BiEncoder(audio_encoder.Cnn8Rnn(32000), te, match.DotProduct(), 512), device=dev)
               for n, te in encoders.items()}
    batch = O.synthetic_batch(a.B, 320000, seed=99, ragged=True)
    g = torch.Generator().manual_seed(1)
    L = a.L
    batch["text"] = torch.randint(2, 5221, (a.B, L), generator=g)
    batch["text_len"] = torch.randint(1, L + 1, (a.B,), generator=g).numpy()
    batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}

    def strong(n):
        return lambda: runners[n].train_step({k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()})

    r = _time_alternating({n: strong(n) for n in runners}, a.rounds, a.steps)
    r["intra_minus_agg_ms"] = r["intra"]["ms_median"] - r["agg"]["ms_median"]
    r["ratio_intra_over_agg"] = r["intra"]["ms_median"] / r["agg"]["ms_median"]
    return {f"strong_step_B{a.B}_L{L}": r}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["kernel", "step"], default="kernel")
    ap.add_argument("--shapes", default="1024x10x512,1024x33x512")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--L", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = bench_kernel(a, dev) if a.mode == "kernel" else bench_step(a, dev)
    res["config"] = vars(a)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
