#!/usr/bin/env python3
"""align.ExpNegL2 (csrc/align.hip) and the MultiTextBiEncoderWithAlign training step, timed with device events, everything
alternated in one process.  Prints one JSON object.  Needs the GPU: there is no fallback.

--mode kernel (default): forward and forward + backward (out.backward(dout)) of
  * expnegl2:   align.ExpNegL2 (torch.ops.tag.align_expnegl2 under autograd);
  * dot_l2norm: align.DotProduct(l2norm=True), the MFMA GEMM on the same operands;
  * torch_fp32: ExpNegL2 stated with stock torch operators in fp32 on the same GPU -- the broadcast difference of
    tests/align_ref.py, one text clip at a time (the whole (B,B,T,N,D) difference is 17 GB at B = 64, N = 8);
  at B in --B, T' = 250, N in --N, D = 512; median / min / max over --rounds of --iters calls each.  With each ExpNegL2 time:
  the lane operations the algorithm needs (a subtraction and a fused multiply-add per pair and element: 2 B*T B*N D forward,
  6 B*T B*N D backward) over the unpacked fp32 VALU peak (256 CU x 4 SIMD x 32 lanes x 2.4 GHz = 78.6e12 lane operations / s;
  packed fp32 doubles it).
--mode step: WeakPhraseRunner.train_step at --step-B x 10 s, 8 phrases per clip, of
  * with_align: MultiTextBiEncoderWithAlign(Cnn8Rnn, EmbeddingAgg(5221, 512), match.DotProduct, align.ExpNegL2,
    AudioMeanTextMean) + MultipleLossSum(ClipBceLoss, MaxMarginRankingLoss(sim_key="sentence_sim"));
  * plain: MultiTextBiEncoder + ClipBceLoss, the same encoders and batch.

    python tools/with_align_bench.py [--mode kernel|step] [--B 32 64] [--N 4 8] [--step-B 64] [--rounds 5] [--iters 20]
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

VALU_LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9


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


def torch_exp_neg_l2(audio, text):
    an = torch.nn.functional.normalize(audio, dim=-1)
    tn = torch.nn.functional.normalize(text, dim=-1)
    cols = [torch.exp(-torch.norm(an[:, :, None, :] - tn[i][None, None, :, :], dim=-1)) for i in range(text.shape[0])]
    return torch.stack(cols, dim=1)                                       # (B, B, T, N)


def bench_kernel(a, dev):
    from texttoaudiogrounding_amd.models import align
    T, D = 250, 512
    res = {}
    for B in a.B:
        for N in a.N:
            g = torch.Generator().manual_seed(B * 10 + N)
            audio = torch.randn(B, T, D, generator=g).to(dev).requires_grad_(True)
            text = torch.randn(B, N, D, generator=g).to(dev).requires_grad_(True)
            dout = torch.randn(B, B, T, N, generator=g).to(dev)
            heads = {"expnegl2": align.ExpNegL2(), "dot_l2norm": align.DotProduct(l2norm=True), "torch_fp32": torch_exp_neg_l2}

            def fwd(head):
                def run():
                    with torch.no_grad():
                        head(audio, text)
                return run

            def fwd_bwd(head):
                def run():
                    audio.grad = text.grad = None
                    head(audio, text).backward(dout)
                return run

            fns = {f"{k}/{how}": make(h) for k, h in heads.items() for how, make in (("forward", fwd), ("forward_backward", fwd_bwd))}
            with torch.no_grad():
                diff = (heads["expnegl2"](audio, text) - heads["torch_fp32"](audio, text)).abs().max().item()
            for fn in fns.values():
                for _ in range(2):
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in fns}
            for _ in range(a.rounds):
                for k, fn in fns.items():
                    times[k].append(timed(fn, a.iters if not k.startswith("torch") else max(1, a.iters // 10)))
            row = {k: summary(v) for k, v in times.items()}
            for k in heads:
                row[f"{k}/backward_ms"] = row[f"{k}/forward_backward"]["ms_median"] - row[f"{k}/forward"]["ms_median"]
            pair_elems = float(B * T) * (B * N) * D
            row["expnegl2/forward_lane_ops"] = 2 * pair_elems
            row["expnegl2/backward_lane_ops"] = 6 * pair_elems
            row["expnegl2/forward_valu_ideal_ms"] = 2 * pair_elems / VALU_LANE_OPS_PER_S * 1e3
            row["expnegl2/backward_valu_ideal_ms"] = 6 * pair_elems / VALU_LANE_OPS_PER_S * 1e3
            row["expnegl2/forward_share_of_valu_peak"] = row["expnegl2/forward_valu_ideal_ms"] / row["expnegl2/forward"]["ms_median"]
            row["expnegl2/backward_share_of_valu_peak"] = row["expnegl2/backward_valu_ideal_ms"] / row["expnegl2/backward_ms"]
            row["torch_over_expnegl2_forward"] = row["torch_fp32/forward"]["ms_median"] / row["expnegl2/forward"]["ms_median"]
            row["torch_over_expnegl2_forward_backward"] = (row["torch_fp32/forward_backward"]["ms_median"]
                                                           / row["expnegl2/forward_backward"]["ms_median"])
            row["max_abs_diff_expnegl2_vs_torch_fp32"] = diff
            res[f"B={B},N={N}"] = row
            del audio, text, dout
            torch.cuda.empty_cache()
    return res


def bench_step(a, dev):
    from oracle import tag_oracle as O
    from texttoaudiogrounding_amd.losses import ClipBceLoss, MaxMarginRankingLoss, MultipleLossSum
    from texttoaudiogrounding_amd.models import align, audio_encoder, audio_text_model, match, sim_pooling, text_encoder
    from texttoaudiogrounding_amd.runner import WeakPhraseRunner
    torch.manual_seed(0)
    B, N, L = a.step_B, 8, 6
    with_align = audio_text_model.MultiTextBiEncoderWithAlign(
        audio_encoder.Cnn8Rnn(32000), text_encoder.EmbeddingAgg(5221, 512), match.DotProduct(), align.ExpNegL2(),
        sim_pooling.AudioMeanTextMean(), 512, ["text"])
    plain = audio_text_model.MultiTextBiEncoder(audio_encoder.Cnn8Rnn(32000), text_encoder.EmbeddingAgg(5221, 512),
                                                match.DotProduct(), 512, ["text"])
    both = MultipleLossSum(["clip", "sentence"], [1, 1], clip=ClipBceLoss(), sentence=MaxMarginRankingLoss(sim_key="sentence_sim"))
    runners = {"plain": WeakPhraseRunner(plain, loss_fn=ClipBceLoss(), device=dev),
               "with_align": WeakPhraseRunner(with_align, loss_fn=both, device=dev)}
    b = O.synthetic_batch(B, 320000, seed=99, ragged=True)
    g = torch.Generator().manual_seed(1)
    nums = torch.randint(1, 5, (B,), generator=g)
    batch = {"waveform": b["waveform"].to(dev), "waveform_len": b["waveform_len"],
             "text": torch.randint(2, 5221, (B, N, L), generator=g).to(dev), "text_len": torch.full((B, N), float(L), device=dev),
             "label": (torch.arange(N)[None, :] < nums[:, None]).float().to(dev)}

    def step(name):
        return runners[name].train_step(dict(batch))

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
    res["ratio_with_align_over_plain"] = res["with_align"]["ms_median"] / res["plain"]["ms_median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["kernel", "step"], default="kernel")
    ap.add_argument("--B", type=int, nargs="+", default=[32, 64])
    ap.add_argument("--N", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--step-B", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("with_align_bench.py needs the GPU: the HIP path has no CPU fallback")
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
