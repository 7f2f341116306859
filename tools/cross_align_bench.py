#!/usr/bin/env python3
"""AudioTextCrossAlignByPhrase: the fused all-pairs cross-encoder (ops.CrossPairsFunction, csrc/cross_pairs.hip) against the
model's loop path (the reference's per-clip data flow on the kernels of csrc/cross.hip), timed with device events, the paths
alternated in one process.  Prints one JSON object.  Needs the GPU: there is no fallback.

--mode kernel (default): the model on stub encoders that return random embeddings, at each (B,T,P,L,D) of --shapes
  (default 32,250,128,8,512 and 8,250,32,8,512; token lengths uniform in 1..L, P spread evenly over the clips): forward
  (no_grad) and forward + backward (sim_matrix.backward(dout)) of ``fused = True`` and ``fused = False``, median / min / max
  over --rounds of --iters calls, the peak device memory of one forward + backward of each path above what the inputs hold,
  the largest difference between the two sim matrices, and tag_crosspairs_ws_bytes.  A path that cannot allocate is reported
  as {"error": ...} and the comparison is made at the shapes both can run.
--mode step: WeakSentenceRunner.train_step at --step-B x 10 s, 1..4 phrases of 6 tokens per clip, MaxMarginRankingLoss, of
  * fused / loop: AudioTextCrossAlignByPhrase(Cnn8Rnn, EmbeddingAgg(5221, 512), match.DotProduct(text_level="token"),
    AudioMeanTextMean, cross_encoder=CrossAttentionGating(512));
  * align_by_phrase: AudioTextAlignByPhrase + align.DotProduct on the same batch (the step of tools/contrastive_bench.py):
    what the sentence-level model costs without the cross-encoder.

    python tools/cross_align_bench.py [--mode kernel|step] [--shapes 32,250,128,8,512 ...] [--step-B 32 8] [--rounds 5]
                                      [--iters 3] [--steps 3] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

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


class _Audio(nn.Module):
    downsample_ratio = 1

    def __init__(self, emb, length):
        super().__init__()
        self.e, self.length, self.embed_dim = nn.Parameter(emb), length, emb.shape[-1]

    def forward(self, d):
        return {"embedding": self.e, "length": self.length}


class _Tokens(nn.Module):
    def __init__(self, tok):
        super().__init__()
        self.t, self.embed_dim = nn.Parameter(tok), tok.shape[-1]

    def forward(self, d):
        return {"token_emb": self.t}


def bench_kernel(a, dev):
    from texttoaudiogrounding_amd import ops
    from texttoaudiogrounding_amd.models import audio_text_model, match, sim_pooling
    from texttoaudiogrounding_amd.models.cross_encoder import CrossAttentionGating
    res = {}
    for shape in a.shapes:
        B, T, P, L, D = (int(x) for x in shape.split(","))
        g = torch.Generator().manual_seed(B + P)
        pnum = [P // B + (1 if j < P % B else 0) for j in range(B)]
        length = torch.full((B,), T)
        length[1:] = torch.randint(T // 2, T + 1, (B - 1,), generator=g)
        tok_len = torch.randint(1, L + 1, (P,), generator=g)
        torch.manual_seed(0)
        model = audio_text_model.AudioTextCrossAlignByPhrase(
            _Audio(torch.randn(B, T, D, generator=g), length), _Tokens(torch.randn(P, L, D, generator=g)),
            match.DotProduct(text_level="token"), sim_pooling.AudioMeanTextMean(), D, False, CrossAttentionGating(D)).to(dev)
        inp = {"text_key": "phrases", "phrases": torch.zeros(P, L, dtype=torch.long), "phrases_len": tok_len, "phrases_num": pnum}
        dout = torch.randn(B, B, T, max(pnum), generator=g).to(dev)

        def fwd(fused):
            def run():
                model.fused = fused
                with torch.no_grad():
                    return model(dict(inp))["sim_matrix"]
            return run

        def fwd_bwd(fused):
            def run():
                model.fused = fused
                model.zero_grad(set_to_none=True)
                model(dict(inp))["sim_matrix"].backward(dout)
            return run

        row = {"ws_bytes": ops.query("tag_crosspairs_ws_bytes", B, T, P, L, D), "one_BPTD_fp32_tensor_bytes": B * P * T * D * 4,
               "tanh_evaluations_forward": int(sum(int(length[i]) for i in range(B)) * int(tok_len.sum()) * D)}
        fns, ok = {}, {}
        for name, fused in (("fused", True), ("loop", False)):
            try:                                              # warm-up, the peak memory of one forward + backward, the matrix
                fwd_bwd(fused)()
                torch.cuda.synchronize()
                model.zero_grad(set_to_none=True)
                torch.cuda.empty_cache()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                fwd_bwd(fused)()
                torch.cuda.synchronize()
                row[f"{name}/peak_bytes_above_inputs"] = torch.cuda.max_memory_allocated() - base
                ok[name] = fwd(fused)()
                fns[f"{name}/forward"], fns[f"{name}/forward_backward"] = fwd(fused), fwd_bwd(fused)
            except torch.cuda.OutOfMemoryError as e:
                row[name] = {"error": "out of memory: " + str(e).split("\n")[0]}
                model.zero_grad(set_to_none=True)
                torch.cuda.empty_cache()
        if len(ok) == 2:
            row["max_abs_diff_fused_vs_loop"] = (ok["fused"] - ok["loop"]).abs().max().item()
        ok.clear()
        times = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                times[k].append(timed(fn, a.iters))
        row.update({k: summary(v) for k, v in times.items()})
        for name in ("fused", "loop"):
            if f"{name}/forward" in row:
                row[f"{name}/backward_ms"] = row[f"{name}/forward_backward"]["ms_median"] - row[f"{name}/forward"]["ms_median"]
        if "fused/forward" in row and "loop/forward" in row:
            for how in ("forward", "forward_backward"):
                row[f"loop_over_fused_{how}"] = row[f"loop/{how}"]["ms_median"] / row[f"fused/{how}"]["ms_median"]
        res[shape] = row
        del model, dout
        torch.cuda.empty_cache()
    return res


def bench_step(a, dev):
    from oracle import tag_oracle as O
    from texttoaudiogrounding_amd.losses import MaxMarginRankingLoss
    from texttoaudiogrounding_amd.models import align, audio_encoder, audio_text_model, match, sim_pooling, text_encoder
    from texttoaudiogrounding_amd.models.cross_encoder import CrossAttentionGating
    from texttoaudiogrounding_amd.runner import WeakSentenceRunner
    res = {}
    for B in a.step_B:
        torch.manual_seed(0)

        def cross(fused):
            m = audio_text_model.AudioTextCrossAlignByPhrase(
                audio_encoder.Cnn8Rnn(32000), text_encoder.EmbeddingAgg(5221, 512), match.DotProduct(text_level="token"),
                sim_pooling.AudioMeanTextMean(), 512, False, cross_encoder=CrossAttentionGating(512))
            m.fused = fused
            return m
        plain = audio_text_model.AudioTextAlignByPhrase(audio_encoder.Cnn8Rnn(32000), text_encoder.EmbeddingAgg(5221, 512),
                                                        align.DotProduct(), sim_pooling.AudioMeanTextMean(), 512)
        runners = {"fused": WeakSentenceRunner(cross(True), loss_fn=MaxMarginRankingLoss(), device=dev),
                   "loop": WeakSentenceRunner(cross(False), loss_fn=MaxMarginRankingLoss(), device=dev),
                   "align_by_phrase": WeakSentenceRunner(plain, loss_fn=MaxMarginRankingLoss(), device=dev)}
        b = O.synthetic_batch(B, 320000, seed=99, ragged=True)
        g = torch.Generator().manual_seed(1)
        nums = torch.randint(1, 5, (B,), generator=g).tolist()
        phrases = torch.randint(2, 5221, (sum(nums), 6), generator=g)
        batch = {"waveform": b["waveform"].to(dev), "waveform_len": b["waveform_len"], "phrases": phrases.to(dev),
                 "phrases_len": torch.full((sum(nums),), 6), "phrases_num": nums, "text_key": "phrases"}

        def step(name):
            return runners[name].train_step({k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()})

        row = {"phrases": sum(nums)}
        for name in list(runners):
            try:
                for _ in range(2):
                    step(name)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                step(name)
                torch.cuda.synchronize()
                row[f"{name}/peak_bytes_allocated"] = torch.cuda.max_memory_allocated()
            except torch.cuda.OutOfMemoryError as e:
                row[name] = {"error": "out of memory: " + str(e).split("\n")[0]}
                del runners[name]
                torch.cuda.empty_cache()
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
        row.update({n: summary(t) for n, t in times.items()})
        if "fused" in times and "loop" in times:
            row["loop_over_fused"] = row["loop"]["ms_median"] / row["fused"]["ms_median"]
        if "fused" in times and "align_by_phrase" in times:
            row["fused_over_align_by_phrase"] = row["fused"]["ms_median"] / row["align_by_phrase"]["ms_median"]
        res[f"B={B}"] = row
        del runners
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["kernel", "step"], default="kernel")
    ap.add_argument("--shapes", nargs="+", default=["32,250,128,8,512", "8,250,32,8,512"])
    ap.add_argument("--step-B", type=int, nargs="+", default=[32, 8])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cross_align_bench.py needs the GPU: the HIP path has no CPU fallback")
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
