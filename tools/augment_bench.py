#!/usr/bin/env python3
"""Cost of SpecAugment / mixup in the Cnn8Rnn training step (csrc/augment.hip): B = 64 x 10 s fp32 encoder steps (forward +
backward of sum(embedding * R), dropout on) with augmentation off, SpecAugment on, and SpecAugment + mixup, ALTERNATED in
one process and timed with device events; plus the host time of the stripe draw (512 scalar torch.randint calls per 64-clip
step, torchlibrosa's draw order).

    python tools/augment_bench.py [--rounds R] [--steps K] [--B 64] [--out FILE.json]

The per-kernel times come from a separate profiler run of the same script with few steps, e.g.
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/augment_bench.py --rounds 1 --steps 3
(kernels augment_fwd_kernel / augment_bwd_kernel).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import tag_oracle as O  # noqa: E402
from texttoaudiogrounding_amd.models.audio_encoder import Cnn8Rnn  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    st = O.init_state(seed=5, logit_gain=120.0)
    m = Cnn8Rnn(32000)
    m.load_state_dict({k[len("audio_encoder."):]: v for k, v in st.items() if k.startswith("audio_encoder.")}, strict=False)
    m = m.to(dev).train()
    b = O.synthetic_batch(a.B, 320000, seed=99, ragged=True)
    wave = b["waveform"].to(dev)
    lens = b["waveform_len"]
    lam = np.tile([0.3, 0.7], a.B // 2)
    variants = {"off": {"specaug": False}, "specaug": {"specaug": True},
                "specaug+mixup": {"specaug": True, "mixup_lambda": lam}}
    R = {}

    def step(kw):
        out = m(dict(waveform=wave, waveform_len=lens, **kw))
        emb = out["embedding"]
        if emb.shape not in R:
            R[emb.shape] = torch.randn(emb.shape, generator=torch.Generator().manual_seed(1)).to(dev)
        (emb * R[emb.shape]).sum().backward()

    for kw in variants.values():                                   # warm-up: every shape the timed window uses
        for _ in range(2):
            step(kw)
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.rounds):
        for name, kw in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                step(kw)
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.steps)
    # host time of the stripe draw alone (what the module spends before the operator is called)
    frames = 320000 // m.hop_length + 1
    t0 = time.perf_counter()
    n_draw = 50
    for _ in range(n_draw):
        m.spec_augmenter.draw(a.B, frames, 64)
    draw_ms = (time.perf_counter() - t0) / n_draw * 1e3
    res = {"B": a.B, "clip_s": 10, "rounds": a.rounds, "steps_per_round": a.steps,
           "step_ms_median": {k: float(np.median(v)) for k, v in times.items()},
           "step_ms_min": {k: float(np.min(v)) for k, v in times.items()},
           "step_ms_all": times, "host_stripe_draw_ms": draw_ms}
    off = res["step_ms_median"]["off"]
    res["delta_vs_off_pct"] = {k: 100.0 * (v - off) / off for k, v in res["step_ms_median"].items() if k != "off"}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
