#!/usr/bin/env python3
"""The text self-attention (SelfAttention, csrc/text_attn.hip), timed with device events, everything alternated in one process.
Prints one JSON object.

--mode kernel (default): for each (R, S, E, H) of --shapes the row-local core tag_text_selfattn_forward / _backward on the packed
  (R, S, 3E) in-projection, on preallocated buffers, with the bytes each pass must move and the rate that gives.  Where the
  audio-over-tokens core is defined (S <= 32) the same work is timed through tag_mha_cross_forward / _backward (every position a
  "frame" over S "tokens") PLUS the copies that route needs: qkv split into three contiguous tensors before, dq / dk / dv packed
  into dqkv after; also the largest difference between the two routes' outputs.
--mode step: BiEncoder(Cnn8Rnn, SelfAttention(5221, 512, 8), DotProduct) through StrongRunner.train_step at B x 10 s against the
  same model with EmbeddingAgg(5221, 512); median / min / max, difference, ratio, and the core's forward + backward at the step's
  own shape (R = B, S = L + 1) as a share of the step.

    python tools/text_selfattn_bench.py [--mode kernel|step] [--shapes 1024x10x512x8,1024x33x512x8] [--rounds 5] [--iters 200]
                                        [--B 64] [--L 8] [--steps 5] [--out FILE.json]

Per-kernel times: a separate profiler run with few iterations, e.g.
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/text_selfattn_bench.py --rounds 1 --iters 3
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pass_bytes(R, S, E, H):
    """Bytes a pass must move: forward reads qkv, writes ctx and attn; backward reads qkv, attn, dctx and writes dqkv."""
    qkv, ctx, attn = 4.0 * R * S * 3 * E, 4.0 * R * S * E, 4.0 * R * H * S * S
    return {"forward": qkv + ctx + attn, "backward": 2 * qkv + attn + ctx}


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


def core_fns(R, S, E, H, dev, with_old):
    """Closures over preallocated buffers: the new core, and (with_old) the audio-over-tokens core with its copies."""
    from texttoaudiogrounding_amd.lib import call, ptr, query
    g = torch.Generator().manual_seed(R + S + E + H)
    qkv = torch.randn(R, S, 3 * E, generator=g).to(dev)
    dctx = torch.randn(R, S, E, generator=g).to(dev)
    klen = torch.randint(1, S + 1, (R,), generator=g).to(dev)
    new = dict(ctx=torch.empty(R, S, E, device=dev), attn=torch.empty(R, H, S, S, device=dev), dqkv=torch.empty(R, S, 3 * E, device=dev))

    def new_fwd():
        call("tag_text_selfattn_forward", ptr(qkv), ptr(klen), ptr(new["ctx"]), ptr(new["attn"]), R, S, E, H, 0.0, 0)

    def new_bwd():
        call("tag_text_selfattn_backward", ptr(qkv), ptr(new["attn"]), ptr(dctx), ptr(klen), ptr(new["dqkv"]), R, S, E, H, 0.0, 0)

    fns = {"new_forward": new_fwd, "new_backward": new_bwd}
    old = None
    if with_old:
        old = dict(ctx=torch.empty(R, S, E, device=dev), attn=torch.empty(R, S, H, S, device=dev), dqkv=torch.empty(R, S, 3 * E, device=dev))
        parts = [torch.empty(R, S, E, device=dev) for _ in range(3)]
        dparts = [torch.empty(R, S, E, device=dev) for _ in range(3)]
        ws = torch.empty(max(int(query("tag_mha_cross_backward_ws_bytes", R, S, S, E)), 16) // 4 + 4, device=dev)

        def split():
            for i, t in enumerate(parts):
                t.copy_(qkv[:, :, i * E:(i + 1) * E])

        def old_fwd():
            split()
            call("tag_mha_cross_forward", ptr(parts[0]), ptr(parts[1]), ptr(parts[2]), ptr(klen), ptr(old["attn"]), ptr(old["ctx"]), R, S,
                 S, E, H, 0.0, 0)

        def old_bwd():                                       # the split tensors are the forward's: saved, not copied again
            call("tag_mha_cross_backward", ptr(parts[0]), ptr(parts[1]), ptr(parts[2]), ptr(old["attn"]), ptr(dctx), ptr(klen),
                 ptr(dparts[0]), ptr(dparts[1]), ptr(dparts[2]), R, S, S, E, H, 0.0, 0, ptr(ws))
            for i, t in enumerate(dparts):
                old["dqkv"][:, :, i * E:(i + 1) * E].copy_(t)

        fns.update(old_forward=old_fwd, old_backward=old_bwd)
    return fns, new, old


def bench_kernel(a, dev):
    from texttoaudiogrounding_amd import dispatch
    res = {}
    for shape in a.shapes.split(","):
        R, S, E, H = (int(v) for v in shape.split("x"))
        with_old = S <= 32
        fns, new, old = core_fns(R, S, E, H, dev, with_old)
        r = _time_alternating(fns, a.rounds, a.iters)
        dispatch.check_async_errors()
        nbytes = pass_bytes(R, S, E, H)
        for p in ("forward", "backward"):
            r[f"new_{p}_bytes"] = nbytes[p]
            r[f"new_{p}_GBps"] = nbytes[p] / (r[f"new_{p}"]["ms_median"] * 1e-3) / 1e9
        r["new_fwd_bwd_ms"] = r["new_forward"]["ms_median"] + r["new_backward"]["ms_median"]
        if with_old:
            r["old_fwd_bwd_ms"] = r["old_forward"]["ms_median"] + r["old_backward"]["ms_median"]
            r["ratio_new_over_old_fwd_bwd"] = r["new_fwd_bwd_ms"] / r["old_fwd_bwd_ms"]
            r["max_abs_diff_new_vs_old"] = {"ctx": float((new["ctx"] - old["ctx"]).abs().max()),
                                            "attn": float((new["attn"] - old["attn"].transpose(1, 2)).abs().max()),
                                            "dqkv": float((new["dqkv"] - old["dqkv"]).abs().max())}
        res[shape] = r
    return res


def bench_step(a, dev):
    from oracle import tag_oracle as O
    from texttoaudiogrounding_amd.models import audio_encoder, audio_text_model, match, text_encoder
    from texttoaudiogrounding_amd.runner import StrongRunner
    torch.manual_seed(0)
    encoders = {"selfattn": text_encoder.SelfAttention(5221, 512, 8), "agg": text_encoder.EmbeddingAgg(5221, 512)}
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
    r["selfattn_minus_agg_ms"] = r["selfattn"]["ms_median"] - r["agg"]["ms_median"]
    r["ratio_selfattn_over_agg"] = r["selfattn"]["ms_median"] / r["agg"]["ms_median"]
    fns, _, _ = core_fns(a.B, L + 1, 512, 8, dev, False)
    core = _time_alternating(fns, a.rounds, a.iters)
    r["core_fwd_bwd_ms_at_step_shape"] = core["new_forward"]["ms_median"] + core["new_backward"]["ms_median"]
    r["core_share_of_step"] = r["core_fwd_bwd_ms_at_step_shape"] / r["selfattn"]["ms_median"]
    return {f"strong_step_B{a.B}_L{L}": r}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["kernel", "step"], default="kernel")
    ap.add_argument("--shapes", default="1024x10x512x8,1024x33x512x8")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
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
