#!/usr/bin/env python3
"""The clip-level BCE objectives (csrc/clip_bce.hip), timed with device events, everything alternated in one process.  Prints one
JSON object.  Needs the GPU: there is no fallback.

--mode passes (default): forward and backward of every mode (the dispatch calls ops.clip_bce_forward / ops.clip_bce_backward, no
  autograd) on a (B,N) clip matrix at --shapes, beside tag_frame_bce_* (ClipBceLoss) on the same matrix; median / min / max over
  --rounds of --iters calls each.  At these sizes the time is launch and host latency.
--mode step: MultiTextBiEncoder(Cnn8Rnn + EmbeddingAgg + DotProduct) through WeakPhraseRunner.train_step at --B clips of
  --seconds s x --N phrases with each new loss (and VectorQuantizeLoss over the focal one) against the same step with ClipBceLoss.

    python tools/clip_bce_bench.py [--mode passes|step] [--shapes 64x8 32x32 128x64] [--B 64] [--N 8] [--seconds 10]
                                   [--rounds 5] [--iters 200] [--steps 5] [--out FILE.json]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def passes(B, N, dev):
    """name -> closure: forward and backward of every mode, and of the frame-BCE kernels, on one seeded input."""
    from texttoaudiogrounding_amd import ops
    g = torch.Generator().manual_seed(B * 1000 + N)
    p = (0.01 + 0.98 * torch.rand(B, N, generator=g)).to(dev)
    label = (torch.rand(B, N, generator=g) < 0.4).float().to(dev)
    counts = torch.randint(1, 500, (B, N), generator=g).double()
    weight, prior = ((100 / (100 + counts)) ** 0.5).float().to(dev), (counts / 1000).float().to(dev)
    length = torch.full((B,), N, dtype=torch.long, device=dev)
    one = torch.ones((), device=dev)
    M = ops.CLIP_BCE_MODES
    modes = {"focal": (M["focal"], None, 2.0, 0.25, 0.0), "freq_weight": (M["freq_weight"], weight, 0.0, 0.0, 0.0),
             "symmetric": (M["symmetric"], None, 1e-3, 0.0, 0.0),
             "origin_symmetric": (M["origin_symmetric"], None, 1.0, 1.0, math.log(1e-3)),
             "prior_adjusted": (M["prior_adjusted"], prior, 1.0, 0.0, 0.0)}
    fns = {"frame_bce/forward": lambda: ops.frame_bce_forward(p, label, length, N),
           "frame_bce/backward": lambda: ops.frame_bce_backward(p, label, length, N, one)}
    for name, (mode, aux, c0, c1, c2) in modes.items():
        fns[f"{name}/forward"] = lambda mode=mode, aux=aux, c=(c0, c1, c2): ops.clip_bce_forward(p, label, aux, mode, *c)
        fns[f"{name}/backward"] = lambda mode=mode, aux=aux, c=(c0, c1, c2): ops.clip_bce_backward(p, label, aux, mode, *c, one)
    return fns


def bench_passes(a, dev):
    res = {}
    for shape in a.shapes:
        B, N = (int(v) for v in shape.split("x"))
        fns = passes(B, N, dev)
        for fn in fns.values():                                   # warm-up: allocator, code objects
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                times[k].append(timed(fn, a.iters))
        res[f"{B}x{N}"] = {k: summary(v) for k, v in times.items()}
    return res


def bench_step(a, dev):
    from oracle import tag_oracle as O
    from texttoaudiogrounding_amd import losses
    from texttoaudiogrounding_amd.models import audio_encoder, audio_text_model, match, text_encoder
    from texttoaudiogrounding_amd.runner import WeakPhraseRunner
    torch.manual_seed(0)

    def model():
        return audio_text_model.MultiTextBiEncoder(audio_encoder.Cnn8Rnn(32000), text_encoder.EmbeddingAgg(5221, 512),
                                                   match.DotProduct(), 512, ["text"])
    loss_fns = {"clip_bce": losses.ClipBceLoss(), "focal": losses.FocalClipBceLoss(),
                "freq_weight": losses.ClipBceLossFreqWeight(100, 0.5), "symmetric": losses.SymmetricClipBceLoss(),
                "origin_symmetric": losses.OriginSymmetricClipBceLoss(), "prior_adjusted": losses.PriorAdjustedClipBceLoss(1000),
                "vq_focal": losses.VectorQuantizeLoss(losses.FocalClipBceLoss(), 0.25)}
    runners = {k: WeakPhraseRunner(model(), loss_fn=fn, device=dev) for k, fn in loss_fns.items()}
    b = O.synthetic_batch(a.B, int(a.seconds * 32000), seed=99, ragged=True)
    g = torch.Generator().manual_seed(1)
    batch = {"waveform": b["waveform"].to(dev), "waveform_len": b["waveform_len"],
             "text": torch.randint(2, 5221, (a.B, a.N, 6), generator=g).to(dev), "text_len": torch.full((a.B, a.N), 6),
             "label": (torch.rand(a.B, a.N, generator=g) < 0.3).float().to(dev),
             "counts": torch.randint(1, 500, (a.B, a.N), generator=g).numpy(), "vq_loss": torch.tensor(0.8, device=dev)}

    def step(name):
        return runners[name].train_step({k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()})

    for name in runners:
        for _ in range(2):
            step(name)
    torch.cuda.synchronize()
    times = {n: [] for n in runners}
    for _ in range(a.rounds):
        for name in runners:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                loss = step(name)
            e1.record()
            torch.cuda.synchronize()
            assert np.isfinite(loss.item()), name
            times[name].append(e0.elapsed_time(e1) / a.steps)
    res = {n: summary(t) for n, t in times.items()}
    for n in runners:
        if n != "clip_bce":
            res[f"ratio_{n}_over_clip_bce"] = res[n]["ms_median"] / res["clip_bce"]["ms_median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["passes", "step"], default="passes")
    ap.add_argument("--shapes", nargs="+", default=["64x8", "32x32", "128x64"])
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--N", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_bce_bench.py needs the GPU: the HIP path has no CPU fallback")
    dev = torch.device("cuda:0")
    res = bench_passes(a, dev) if a.mode == "passes" else bench_step(a, dev)
    res["config"] = vars(a)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
