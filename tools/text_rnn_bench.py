#!/usr/bin/env python3
"""The text GRU (RnnEncoder, csrc/text_gru.hip), timed with device events, everything alternated in one process.  Prints one
JSON object.

--mode passes (default): for each (R, L, H) of --shapes, one bidirectional layer: the row-local launches
  tag_text_gru_forward / tag_text_gru_backward against the same tensors routed through the audio recurrence
  tag_gru_forward / tag_gru_backward (persistent cooperative launch where its grid fits, one launch per step otherwise),
  all on preallocated buffers; also the largest difference between the two routes' outputs and the FLOP of a pass.
--mode step: BiEncoder(Cnn8Rnn, RnnEncoder(5221, 512, 256, 1, 0, True, "GRU"), DotProduct) through StrongRunner.train_step at
  B x 10 s against the same model with EmbeddingAgg(5221, 512), and MultiTextBiEncoder (forward + ClipBceLoss + backward,
  plain autograd) at --weak-B clips x --weak-N phrases with either text encoder; median / min / max, difference and ratio.

    python tools/text_rnn_bench.py [--mode passes|step] [--shapes 64x6x256,1024x8x256,...] [--rounds 5] [--iters 200]
                                   [--B 64] [--steps 5] [--weak-B 32] [--weak-N 32] [--out FILE.json]

Per-kernel times: a separate profiler run with few iterations, e.g.
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/text_rnn_bench.py --rounds 1 --iters 3
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pass_flop(R, L, H, dirs=2):
    """FLOP of the recurrent products of one pass: forward h W_hh^T over L - 1 steps, backward dgh W_hh likewise."""
    return 2.0 * R * (L - 1) * dirs * 3 * H * H


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


def bench_passes(a, dev):
    from texttoaudiogrounding_amd import dispatch
    from texttoaudiogrounding_amd.lib import call, ptr
    res = {}
    for shape in a.shapes.split(","):
        R, L, H = (int(v) for v in shape.split("x"))
        g = torch.Generator().manual_seed(R + L + H)
        k = 1.0 / H ** 0.5
        gi = torch.randn(R, L, 2, 3 * H, generator=g).to(dev)
        w = ((torch.rand(2, 3 * H, H, generator=g) * 2 - 1) * k).to(dev)
        b = ((torch.rand(2, 3 * H, generator=g) * 2 - 1) * k).to(dev)
        dy = torch.randn(R, L, 2 * H, generator=g).to(dev)
        new = dict(y=torch.empty(R, L, 2 * H, device=dev), gates=torch.empty(R, L, 2, 4 * H, device=dev))
        old = {k_: torch.empty_like(v) for k_, v in new.items()}
        for d in (new, old):
            d.update(dgi=torch.empty(R, L, 2, 3 * H, device=dev), dgh=torch.empty(R, L, 2, 3 * H, device=dev),
                     hprev=torch.empty(R, L, 2, H, device=dev))
        ws_f, ws_b = dispatch._gru_ws(R, L, H, gi, "fwd"), dispatch._gru_ws(R, L, H, gi, "bwd")

        def new_fwd():
            call("tag_text_gru_forward", ptr(gi), ptr(w), ptr(b), None, ptr(new["y"]), ptr(new["gates"]), None, R, L, H, 2)

        def old_fwd():
            call("tag_gru_forward", ptr(gi), ptr(w), ptr(b), ptr(old["y"]), ptr(old["gates"]), ptr(ws_f), R, L, H)

        def new_bwd():
            call("tag_text_gru_backward", ptr(dy), None, None, ptr(new["y"]), ptr(new["gates"]), ptr(w), ptr(new["dgi"]),
                 ptr(new["dgh"]), ptr(new["hprev"]), R, L, H, 2)

        def old_bwd():
            call("tag_gru_backward", ptr(dy), ptr(old["y"]), ptr(old["gates"]), ptr(w), ptr(old["dgi"]), ptr(old["dgh"]),
                 ptr(old["hprev"]), ptr(ws_b), R, L, H)

        fns = {"new_forward": new_fwd, "old_forward": old_fwd, "new_backward": new_bwd, "old_backward": old_bwd}
        for fn in fns.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        dispatch.check_async_errors()
        diff = {k_: float((new[k_] - old[k_]).abs().max()) for k_ in new}
        times = {n: [] for n in fns}
        for _ in range(a.rounds):
            for n, fn in fns.items():
                times[n].append(timed(fn, a.iters))
        r = {n: summary(t) for n, t in times.items()}
        for p in ("forward", "backward"):
            r[f"ratio_new_over_old_{p}"] = r[f"new_{p}"]["ms_median"] / r[f"old_{p}"]["ms_median"]
            r[f"new_{p}_tflops"] = pass_flop(R, L, H) / (r[f"new_{p}"]["ms_median"] * 1e-3) / 1e12
        r["max_abs_diff_new_vs_old"] = diff
        r["flop_per_pass"] = pass_flop(R, L, H)
        res[shape] = r
    return res


def _time_alternating(fns, rounds, steps):
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n in fns}
    for _ in range(rounds):
        for n, fn in fns.items():
            times[n].append(timed(fn, steps))
    return {n: summary(t) for n, t in times.items()}


def bench_step(a, dev):
    from oracle import tag_oracle as O
    from texttoaudiogrounding_amd.losses import ClipBceLoss
    from texttoaudiogrounding_amd.models import audio_encoder, audio_text_model, match, text_encoder
    from texttoaudiogrounding_amd.runner import StrongRunner
    torch.manual_seed(0)

    def encoders():
        return {"rnn": text_encoder.RnnEncoder(5221, 512, 256, 1, 0, True, "GRU"), "agg": text_encoder.EmbeddingAgg(5221, 512)}

    res = {}
    runners = {n: StrongRunner(audio_text_model.BiEncoder(audio_encoder.Cnn8Rnn(32000), te, match.DotProduct(), 512), device=dev)
               for n, te in encoders().items()}
    batch = O.synthetic_batch(a.B, 320000, seed=99, ragged=True)
    g = torch.Generator().manual_seed(1)
    L = 8
    batch["text"] = torch.randint(2, 5221, (a.B, L), generator=g)
    batch["text_len"] = torch.randint(1, L + 1, (a.B,), generator=g).numpy()
    batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}

    def strong(n):
        return lambda: runners[n].train_step({k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()})

    r = _time_alternating({n: strong(n) for n in runners}, a.rounds, a.steps)
    r["rnn_minus_agg_ms"] = r["rnn"]["ms_median"] - r["agg"]["ms_median"]
    r["ratio_rnn_over_agg"] = r["rnn"]["ms_median"] / r["agg"]["ms_median"]
    res[f"strong_step_B{a.B}_L{L}"] = r
    del runners
    torch.cuda.empty_cache()

    B, N, L = a.weak_B, a.weak_N, 8
    models = {n: audio_text_model.MultiTextBiEncoder(audio_encoder.Cnn8Rnn(32000), te, match.DotProduct(), 512,
                                                     text_forward_keys=["text"]).to(dev).train()
              for n, te in encoders().items()}
    wave = (0.1 * torch.randn(B, 320000, generator=g)).to(dev)
    text = torch.randint(2, 5221, (B, N, L), generator=g).to(dev)
    text_len = torch.randint(1, L + 1, (B, N), generator=g)
    label = (torch.rand(B, N, generator=g) < 0.5).float().to(dev)
    loss_fn = ClipBceLoss()

    def weak(n):
        def run():
            models[n].zero_grad(set_to_none=True)
            out = models[n]({"waveform": wave, "waveform_len": np.full(B, 320000), "text": text, "text_len": text_len,
                             "specaug": False})
            out["label"] = label
            loss_fn(out).backward()
        return run

    r = _time_alternating({n: weak(n) for n in models}, a.rounds, a.steps)
    r["rnn_minus_agg_ms"] = r["rnn"]["ms_median"] - r["agg"]["ms_median"]
    r["ratio_rnn_over_agg"] = r["rnn"]["ms_median"] / r["agg"]["ms_median"]
    res[f"weak_fwd_bwd_B{B}_N{N}_L{L}"] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["passes", "step"], default="passes")
    ap.add_argument("--shapes", default="64x6x256,1024x8x256,2048x12x256,1024x8x128")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--weak-B", type=int, default=32)
    ap.add_argument("--weak-N", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
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
