#!/usr/bin/env python3
"""The class-mapping baseline (AudioTagging, csrc/tagging.hip), timed with device events, everything alternated in one
process.  Prints one JSON object.

--mode passes (default): on one (B, T, C) probability tensor,
  * tag_class_pool_forward + tag_tagging_head_backward against tag_sim_pool_forward + tag_sim_pool_backward (tmode = -1,
    the only other way to pool this tensor), for --pooling;
  * tag_masked_frame_bce_forward + _backward (null class mask) against the route of ClipFrameBceLoss: transpose-copies of
    scores and labels to (B*C, T) + tag_frame_bce_forward + _backward;
  * every new pass on its own, with the bytes it moves (reads + writes, from the shapes) and hence TB/s.
--mode step: AudioTagging(Cnn8Rnn(32000), 527) + ClipMaskedFrameBceLoss(0.5) through ClassMappingRunner.train_step against
  BiEncoder(Cnn8Rnn + EmbeddingAgg + DotProduct) through StrongRunner.train_step at B x 10 s (--model crnn: CrnnEncoder(256),
  300 classes, against the strong eg_config BiEncoder), median / min / max step time and the ratio.
--bytes: only the bytes each new pass moves at this size.

    python tools/tagging_bench.py [--mode passes|step] [--model cnn8rnn|crnn] [--B 64] [--T 250] [--C 527] [--pooling linear_softmax]
                                  [--rounds 5] [--iters 200] [--steps 5] [--device-batch] [--out FILE.json]

Per-kernel times: a separate profiler run with few iterations, e.g.
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/tagging_bench.py --rounds 1 --iters 3
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pass_bytes(B, T, C):
    """HBM bytes (reads + writes) of each new pass on a full-length (B, T, C) fp32 tensor."""
    n, s = B * T * C * 4, B * C * 4
    return {"class_pool_forward": n + 2 * s,                       # read prob; write clip, aux
            "tagging_head_backward": 3 * n + 3 * s,                # read prob, dprob; write dlogit; read dclip, clip, aux
            "tagging_head_backward_no_dprob": 2 * n + 3 * s,
            "masked_frame_bce_forward": 2 * n,                     # read prob, label
            "masked_frame_bce_backward": 3 * n}                    # read prob, label; write dprob


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
    from texttoaudiogrounding_amd import ops
    from texttoaudiogrounding_amd.lib import call, ptr
    B, T, C = a.B, a.T, a.C
    mode = ops.POOL_MODES[a.pooling]
    g = torch.Generator().manual_seed(0)
    prob = torch.sigmoid(torch.randn(B, T, C, generator=g)).to(dev)
    label = (torch.rand(B, T, C, generator=g) < 0.3).float().to(dev)
    dprob, dclip = torch.randn(B, T, C, generator=g).to(dev), torch.randn(B, C, generator=g).to(dev)
    length = torch.randint(T // 2, T + 1, (B,), generator=g)
    length[0] = T
    length = length.to(dev)
    len_rows = length.repeat_interleave(C).contiguous()
    one = torch.ones((), device=dev)
    clip, aux = ops.class_pool_forward(prob, length, mode)
    out_old, dsim_old = torch.empty(B, C, device=dev), torch.empty_like(prob)
    dlogit = torch.empty_like(prob)

    def new_pool():
        c, x = ops.class_pool_forward(prob, length, mode)
        ops.tagging_head_dlogit(prob, None, dclip, c, x, length, mode, out=dlogit)

    def old_pool():
        call("tag_sim_pool_forward", ptr(prob), ptr(length), None, ptr(out_old), B, T, C, 1, 1, mode, -1)
        call("tag_sim_pool_backward", ptr(prob), ptr(length), None, ptr(dclip), ptr(dsim_old), B, T, C, 1, 1, mode, -1)

    def new_bce():
        ops.masked_frame_bce_forward(prob, label, length, None)
        ops.masked_frame_bce_backward(prob, label, length, None, one)

    def old_bce():
        fs2 = prob.transpose(1, 2).reshape(B * C, T).contiguous()
        lab2 = label.transpose(1, 2).reshape(B * C, T).contiguous()
        ops.frame_bce_forward(fs2, lab2, len_rows, T)
        ops.frame_bce_backward(fs2, lab2, len_rows, T, one)

    singles = {"class_pool_forward": lambda: ops.class_pool_forward(prob, length, mode),
               "tagging_head_backward": lambda: ops.tagging_head_dlogit(prob, dprob, dclip, clip, aux, length, mode, out=dlogit),
               "tagging_head_backward_no_dprob": lambda: ops.tagging_head_dlogit(prob, None, dclip, clip, aux, length, mode,
                                                                                  out=dlogit),
               "masked_frame_bce_forward": lambda: ops.masked_frame_bce_forward(prob, label, length, None),
               "masked_frame_bce_backward": lambda: ops.masked_frame_bce_backward(prob, label, length, None, one)}
    pairs = {"pool_new": new_pool, "pool_sim_pool": old_pool, "bce_new": new_bce, "bce_transpose_frame_bce": old_bce}
    # the two pooling routes compute the same thing
    new_pool()
    old_pool()
    torch.cuda.synchronize()
    agree = {"clip_max_abs_diff": float((ops.class_pool_forward(prob, length, mode)[0] - out_old).abs().max()),
             "dclip_term_max_abs_diff": float((dlogit - dsim_old * prob * (1 - prob)).abs().max())}
    everything = dict(pairs)
    everything.update(singles)
    for fn in everything.values():                              # warm-up: allocator, code objects
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in everything}
    for _ in range(a.rounds):
        for k, fn in everything.items():
            times[k].append(timed(fn, a.iters if k != "pool_sim_pool" else max(1, a.iters // 10)))
    res = {k: summary(v) for k, v in times.items()}
    by = pass_bytes(B, T, C)
    for k in singles:
        res[k]["bytes"] = by[k]
        res[k]["tb_per_s_at_median"] = by[k] / (res[k]["ms_median"] * 1e-3) / 1e12
    res["speedup_pool"] = res["pool_sim_pool"]["ms_median"] / res["pool_new"]["ms_median"]
    res["speedup_bce"] = res["bce_transpose_frame_bce"]["ms_median"] / res["bce_new"]["ms_median"]
    res["agreement"] = agree
    return res


def bench_step(a, dev):
    from oracle import tag_oracle as O
    from texttoaudiogrounding_amd.losses import ClipMaskedFrameBceLoss
    from texttoaudiogrounding_amd.models import audio_encoder, audio_text_model, match, text_encoder
    from texttoaudiogrounding_amd.runner import ClassMappingRunner, StrongRunner
    torch.manual_seed(0)
    if a.model == "crnn":
        bi = audio_text_model.BiEncoder(audio_encoder.CrnnEncoder(32000, 256), text_encoder.EmbeddingAgg(5221, 256),
                                        match.ExpNegL2(), 256)
        tag = audio_text_model.AudioTagging(audio_encoder.CrnnEncoder(32000, 256), 300)
        hop, T, C = 640, 125, 300
    else:
        bi = audio_text_model.BiEncoder(audio_encoder.Cnn8Rnn(32000), text_encoder.EmbeddingAgg(5221, 512), match.DotProduct(), 512)
        tag = audio_text_model.AudioTagging(audio_encoder.Cnn8Rnn(32000), 527)
        hop, T, C = 320, 250, 527
    runners = {"biencoder": StrongRunner(bi, device=dev),
               "tagging": ClassMappingRunner(tag, loss_fn=ClipMaskedFrameBceLoss(0.5), device=dev)}
    b = O.synthetic_batch(a.B, 320000, seed=99, ragged=True, hop=hop)
    g = torch.Generator().manual_seed(1)
    batches = {"biencoder": dict(b, label=(torch.rand(a.B, T, generator=g) > 0.7).float()),
               "tagging": {"waveform": b["waveform"], "waveform_len": b["waveform_len"],
                           "strong_label": (torch.rand(a.B, T, C, generator=g) < 0.05).float(),
                           "weak_label": (torch.rand(a.B, C, generator=g) < 0.05).float(),
                           "strong_label_mask": (torch.rand(a.B, C, generator=g) < 0.5).float()}}
    if a.device_batch:
        batches = {n: {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in bb.items()} for n, bb in batches.items()}

    def step(name):
        return runners[name].train_step({k: (v.clone() if torch.is_tensor(v) else v) for k, v in batches[name].items()})

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
    res["ratio_tagging_over_biencoder"] = res["tagging"]["ms_median"] / res["biencoder"]["ms_median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["passes", "step"], default="passes")
    ap.add_argument("--model", choices=["cnn8rnn", "crnn"], default="cnn8rnn")
    ap.add_argument("--pooling", default="linear_softmax")
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--T", type=int, default=250)
    ap.add_argument("--C", type=int, default=527)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--bytes", action="store_true")
    ap.add_argument("--device-batch", action="store_true",
                    help="stage the batch on the device once (as bench.py does) instead of re-staging the host batch every step")
    a = ap.parse_args()
    if a.bytes:
        print(json.dumps(pass_bytes(a.B, a.T, a.C)))
        return
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
