#!/usr/bin/env python3
"""The sentence-level contrastive objectives (csrc/contrastive.hip), timed with device events, everything alternated in one
process.  Prints one JSON object.  Needs the GPU: there is no fallback.

--mode passes (default): for InfoNce, Max / Weighted / RandomTriplet on an (n,n) matrix and MilNce on (n, 8), forward + backward
  * hip_kernels: the two dispatch calls (ops.*_forward + ops.*_backward), no autograd;
  * hip_autograd: the operator (torch.ops.tag.*) and loss.backward(), what a training step pays;
  * torch_autograd: the same objective composed from stock torch operators (tests/contrastive_ref.py, fp32 on the device) and
    loss.backward();
  at every --sizes n, median / min / max over --rounds of --iters calls each.  At these sizes the time is launch and host
  latency, so the autograd rows are bounded by the host.
--mode step: AudioTextAlignByPhrase(Cnn8Rnn + EmbeddingAgg + align.DotProduct + AudioMeanTextMean) through
  WeakSentenceRunner.train_step at B x 10 s with InfoNceLoss against MaxMarginRankingLoss.

    python tools/contrastive_bench.py [--mode passes|step] [--sizes 32 64 128 512] [--B 32] [--rounds 5] [--iters 200]
                                      [--steps 5] [--out FILE.json]
"""
import argparse
import json
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


def objectives(n, dev):
    """name -> (hip_kernels, hip_autograd, torch_autograd) closures on one seeded input."""
    import texttoaudiogrounding_amd.torch_ops  # noqa: F401
    from texttoaudiogrounding_amd import ops
    from tests import contrastive_ref as R
    g = torch.Generator().manual_seed(n)
    x = R.raised_diagonal_input(n, n, torch.float32).to(dev).requires_grad_(True)
    xd = x.detach()
    c = torch.rand(n, 8, generator=g).to(dev).requires_grad_(True)
    label = (torch.rand(n, 8, generator=g) < 0.4).float().to(dev)
    cd = c.detach()
    s = torch.randint(n, (n,), generator=g).to(dev)
    a = torch.randint(n, (n,), generator=g).to(dev)
    s32, a32 = s.int(), a.int()
    one = torch.ones((), device=dev)
    M = ops.TRIPLET_MODES

    def autograd(fn, leaf):
        def run():
            leaf.grad = None
            fn().backward()
        return run

    def kernels(fwd, bwd):
        def run():
            _, ws = fwd()
            bwd(ws)
        return run

    def triplet(mode, margin, si, ai, ref):
        return (kernels(lambda: ops.triplet_forward(xd, mode, margin, si, ai),
                        lambda ws: ops.triplet_backward(xd, mode, margin, si, ai, one, ws)),
                autograd(lambda: torch.ops.tag.triplet(x, mode, margin, si, ai), x), autograd(ref, x))

    return {
        "infonce": (kernels(lambda: ops.infonce_forward(xd, 0.07), lambda ws: ops.infonce_backward(xd, 0.07, one, ws)),
                    autograd(lambda: torch.ops.tag.infonce(x, 0.07), x), autograd(lambda: R.infonce(x, 0.07), x)),
        "max_triplet": triplet(M["max"], 0.2, None, None, lambda: R.max_triplet(x, 0.2)),
        "weighted_triplet": triplet(M["weighted"], 0.2, None, None, lambda: R.weighted_triplet(x, 0.2)),
        "random_triplet": triplet(M["random"], 0.2, s32, a32, lambda: R.random_triplet(x, 0.2, s, a)),
        "milnce": (kernels(lambda: ops.milnce_forward(cd, label, 1.0),
                           lambda ws: ops.milnce_backward(cd, label, 1.0, one, ws)),
                   autograd(lambda: torch.ops.tag.milnce(c, label, 1.0), c), autograd(lambda: R.milnce(c, label, 1.0), c)),
    }


def bench_passes(a, dev):
    res = {}
    for n in a.sizes:
        fns = {f"{name}/{how}": fn for name, three in objectives(n, dev).items()
               for how, fn in zip(("hip_kernels", "hip_autograd", "torch_autograd"), three)}
        for fn in fns.values():                                   # warm-up: allocator, code objects
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                times[k].append(timed(fn, a.iters))
        row = {k: summary(v) for k, v in times.items()}
        for name in {k.split("/")[0] for k in fns}:
            row[f"{name}/torch_over_hip_autograd"] = row[f"{name}/torch_autograd"]["ms_median"] / row[f"{name}/hip_autograd"]["ms_median"]
        res[f"n={n}"] = row
    return res


def bench_step(a, dev):
    from oracle import tag_oracle as O
    from texttoaudiogrounding_amd.losses import InfoNceLoss, MaxMarginRankingLoss
    from texttoaudiogrounding_amd.models import align, audio_encoder, audio_text_model, sim_pooling, text_encoder
    from texttoaudiogrounding_amd.runner import WeakSentenceRunner
    torch.manual_seed(0)

    def model():
        return audio_text_model.AudioTextAlignByPhrase(audio_encoder.Cnn8Rnn(32000), text_encoder.EmbeddingAgg(5221, 512),
                                                       align.DotProduct(), sim_pooling.AudioMeanTextMean(), 512)
    runners = {"maxmargin": WeakSentenceRunner(model(), loss_fn=MaxMarginRankingLoss(), device=dev),
               "infonce": WeakSentenceRunner(model(), loss_fn=InfoNceLoss(), device=dev)}
    b = O.synthetic_batch(a.B, 320000, seed=99, ragged=True)
    g = torch.Generator().manual_seed(1)
    nums = torch.randint(1, 5, (a.B,), generator=g).tolist()
    phrases = torch.randint(2, 5221, (sum(nums), 6), generator=g)
    batch = {"waveform": b["waveform"].to(dev), "waveform_len": b["waveform_len"], "phrases": phrases.to(dev),
             "phrases_len": torch.full((sum(nums),), 6), "phrases_num": nums, "text_key": "phrases"}

    def step(name):
        return runners[name].train_step({k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()})

    for name in runners:
        for _ in range(3):
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
            assert np.isfinite(loss.item())
            times[name].append(e0.elapsed_time(e1) / a.steps)
    res = {n: summary(t) for n, t in times.items()}
    res["ratio_infonce_over_maxmargin"] = res["infonce"]["ms_median"] / res["maxmargin"]["ms_median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["passes", "step"], default="passes")
    ap.add_argument("--sizes", type=int, nargs="+", default=[32, 64, 128, 512])
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("contrastive_bench.py needs the GPU: the HIP path has no CPU fallback")
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
