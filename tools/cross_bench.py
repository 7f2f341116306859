#!/usr/bin/env python3
"""Training step of an early-fusion model against its late-fusion twin, both through StrongRunner.train_step at B x 10 s, fp32,
dropout on, ALTERNATED in one process and timed with device events; plus one eval forward of each.  Prints one JSON object
(median / spread / peak memory per model, the step ratio).

--model cnn8rnn (default): CrossCnn8_Rnn against BiEncoder(Cnn8Rnn + EmbeddingAgg(5221, 512) + DotProduct);
--model cdur: CrossCDur(32000, EmbeddingAgg(5221, 256)) against BiEncoder(CrnnEncoder(32000, 256) + EmbeddingAgg(5221, 256) +
ExpNegL2), the strong eg_config.

    python tools/cross_bench.py [--model cnn8rnn|cdur] [--rounds 5] [--steps 10] [--B 64] [--out FILE.json]

--device-batch stages the batch on the device once, as bench.py does; without it every step re-stages the host batch (82 MB of
waveform at B = 64 x 10 s), which dominates the short CRNN steps.

Per-kernel times: a separate profiler run with few steps, e.g.
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/cross_bench.py --rounds 1 --steps 2
and ``--bytes`` prints the bytes each new pass moves at this size (for its TB/s).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import tag_oracle as O  # noqa: E402
from texttoaudiogrounding_amd.models import audio_encoder, audio_text_model, match, text_encoder  # noqa: E402
from texttoaudiogrounding_amd.runner import StrongRunner  # noqa: E402


def clip_sum_bytes(B, frames=501):
    """HBM bytes each per-clip bias-gradient pass of CrossCDur reads at B clips of `frames` frames, fp32: dz of block 1 to 5."""
    f2, f4 = frames // 2, frames // 4
    return {"rowgroup_colsum": [B * h * w * c * 4 for h, w, c in ((frames, 64, 32), (f2, 16, 128), (f2, 16, 128), (f4, 4, 128),
                                                                  (f4, 4, 128))]}


def pass_bytes(B, frames=1001):
    """HBM bytes (reads + writes) of each new pass at B clips of `frames` frames, fp32: one entry per conv block, 1 to 4."""
    out = {}
    h, w = frames, 64
    for c, (ph, pw) in zip((64, 128, 256, 512), ((2, 2), (2, 2), (1, 2), (1, 2))):
        n = B * h * w * c * 4
        out.setdefault("bias_bnrelu_forward", []).append(2 * n)                        # read y1, write a1
        out.setdefault("bias_pool_forward", []).append(n + n // (ph * pw))            # read y2, write pooled
        out.setdefault("bias_pool_bwd_reduce", []).append(n + n // (ph * pw))         # read y2 + dout
        out.setdefault("bias_pool_bwd_apply", []).append(2 * n + n // (ph * pw))      # read y2 + dout, write dy2
        out.setdefault("bias_bnrelu_bwd_reduce", []).append(2 * n)                    # read y1 + da1
        out.setdefault("bias_bnrelu_bwd_apply", []).append(3 * n)                     # read y1 + da1, write dy1
        h, w = h // ph, w // pw
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=["cnn8rnn", "cdur"], default="cnn8rnn")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--out", default=None)
    ap.add_argument("--bytes", action="store_true")
    ap.add_argument("--device-batch", action="store_true",
                    help="stage the batch on the device once (as bench.py does) instead of re-staging the host batch every step")
    a = ap.parse_args()
    if a.bytes:
        print(json.dumps(clip_sum_bytes(a.B) if a.model == "cdur" else pass_bytes(a.B)))
        return
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    if a.model == "cdur":
        bi = audio_text_model.BiEncoder(audio_encoder.CrnnEncoder(32000, 256), text_encoder.EmbeddingAgg(5221, 256),
                                        match.ExpNegL2(), 256)
        cross = audio_text_model.CrossCDur(32000, text_encoder.EmbeddingAgg(5221, 256))
        hop, T = 640, 125
    else:
        bi = audio_text_model.BiEncoder(audio_encoder.Cnn8Rnn(32000), text_encoder.EmbeddingAgg(5221, 512), match.DotProduct(), 512)
        cross = audio_text_model.CrossCnn8_Rnn(32000, text_encoder.EmbeddingAgg(5221, 512))
        hop, T = 320, 250
    runners = {"biencoder": StrongRunner(bi, device=dev), "cross": StrongRunner(cross, device=dev)}
    b = O.synthetic_batch(a.B, 320000, seed=99, ragged=True, hop=hop)
    b["label"] = (torch.rand(a.B, T, generator=torch.Generator().manual_seed(1)) > 0.7).float()

    if a.device_batch:
        b = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()}

    def step(name):
        return runners[name].train_step({k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()})

    for name in runners:                                  # warm-up: allocator, weight packs, GRU scratch
        for _ in range(3):
            step(name)
    torch.cuda.synchronize()
    times = {n: [] for n in runners}
    peak = {}
    for _ in range(a.rounds):
        for name in runners:
            torch.cuda.reset_peak_memory_stats()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                loss = step(name)
            e1.record()
            torch.cuda.synchronize()
            assert np.isfinite(loss.item())
            times[name].append(e0.elapsed_time(e1) / a.steps)
            peak[name] = max(peak.get(name, 0), torch.cuda.max_memory_allocated())
    ev = {}
    for name, r in runners.items():
        r.model.eval()
        with torch.no_grad():
            inp = {"waveform": b["waveform"].to(dev), "waveform_len": b["waveform_len"], "text": b["text"].to(dev),
                   "text_len": torch.as_tensor(b["text_len"]).to(dev), "specaug": False}
            r.model(inp)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r.model(inp)
            e1.record()
            torch.cuda.synchronize()
            ev[name] = e0.elapsed_time(e1)
    res = {n: {"step_ms_median": float(np.median(t)), "step_ms_min": float(np.min(t)), "step_ms_max": float(np.max(t)),
               "peak_alloc_gib": peak[n] / 2 ** 30, "eval_forward_ms": ev[n]} for n, t in times.items()}
    res["ratio_cross_over_biencoder"] = res["cross"]["step_ms_median"] / res["biencoder"]["step_ms_median"]
    res["config"] = {"model": a.model, "device_batch": a.device_batch, "B": a.B, "seconds": 10, "rounds": a.rounds, "steps": a.steps}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
