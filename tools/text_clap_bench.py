#!/usr/bin/env python3
"""The trainable LAION-CLAP text tower (LaionClapEncoder, csrc/text_clap.hip + tag_gemm + csrc/text_attn.hip), timed with device
events, everything alternated in one process.  Prints one JSON object.

--mode op (default): the encoder alone at RoBERTa-base shape (12 layers, hidden 768, 12 heads, FFN 3072, projection 512) on
  R = --R phrases of L = --L tokens, dropouts 0: forward (no_grad) and forward + backward of a fixed linear objective, against the
  SAME layer stack written in plain torch (F.embedding / F.linear / F.layer_norm / softmax / F.gelu) and run eagerly on the same
  GPU in fp32 in the same harness.  Reports ms for both, the ratio, and the achieved share of the fp32 MFMA peak computed from
  6 x (dense parameters) x M FLOP for forward + backward (2 x for the forward), M = R L token rows.
--mode step: BiEncoder(Cnn8Rnn, LaionClapEncoder, DotProduct, add_proj) through StrongRunner.train_step at B x 10 s, with the
  tower trainable and frozen, against the same step with EmbeddingAgg(5221, 512).

    python tools/text_clap_bench.py [--mode op|step] [--R 512] [--L 12] [--rounds 5] [--iters 5] [--B 64] [--steps 3] [--out F.json]

Per-kernel times: a separate profiler run with few iterations, e.g.
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/text_clap_bench.py --rounds 1 --iters 2 --no-eager
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_FP32_MFMA = 157.3           # TFLOP/s (v_mfma_f32_32x32x2_f32), as bench.py


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


def _time_alternating(fns, rounds, iters, warm=2):
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n in fns}
    for _ in range(rounds):
        for n, fn in fns.items():
            times[n].append(timed(fn, iters))
    return {n: summary(t) for n, t in times.items()}


def eager_forward(st, ids, mask, heads, eps=1e-12, pad_id=1):
    """The same layer stack in plain torch (Hugging Face's eager arithmetic), on whatever device st lives on."""
    import math
    import torch.nn.functional as F
    g = lambda k: st["model." + k]                               # noqa: E731
    R, L = ids.shape
    m = ids.ne(pad_id).long()
    pos = torch.cumsum(m, 1) * m + pad_id
    h = F.embedding(ids, g("embeddings.word_embeddings.weight"), padding_idx=pad_id) + g("embeddings.token_type_embeddings.weight")[0] \
        + F.embedding(pos, g("embeddings.position_embeddings.weight"), padding_idx=pad_id)
    D = h.shape[-1]
    h = F.layer_norm(h, (D,), g("embeddings.LayerNorm.weight"), g("embeddings.LayerNorm.bias"), eps)
    dh = D // heads
    add = (1.0 - mask.to(h.dtype))[:, None, None, :] * torch.finfo(h.dtype).min
    layers = 1 + max(int(k.split(".")[3]) for k in st if k.startswith("model.encoder.layer."))
    for l in range(layers):
        p = f"encoder.layer.{l}."
        lin = lambda x, n: F.linear(x, g(p + n + ".weight"), g(p + n + ".bias"))              # noqa: E731
        q, k, v = (lin(h, "attention.self." + n).view(R, L, heads, dh).transpose(1, 2) for n in ("query", "key", "value"))
        w = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(dh) + add, dim=-1)
        a = lin(torch.matmul(w, v).transpose(1, 2).reshape(R, L, D), "attention.output.dense")
        h = F.layer_norm(h + a, (D,), g(p + "attention.output.LayerNorm.weight"), g(p + "attention.output.LayerNorm.bias"), eps)
        f = lin(F.gelu(lin(h, "intermediate.dense")), "output.dense")
        h = F.layer_norm(h + f, (D,), g(p + "output.LayerNorm.weight"), g(p + "output.LayerNorm.bias"), eps)
    pooled = torch.tanh(F.linear(h[:, 0], g("pooler.dense.weight"), g("pooler.dense.bias")))

    def proj(x):
        x = F.relu(F.linear(x, st["projection.linear1.weight"], st["projection.linear1.bias"]))
        return F.linear(x, st["projection.linear2.weight"], st["projection.linear2.bias"])
    return proj(h), F.normalize(proj(pooled), dim=-1)


def bench_op(a, dev):
    from oracle import clap_text_oracle as C
    from texttoaudiogrounding_amd import dispatch
    from texttoaudiogrounding_amd.models.hf_modeling_grounding import CLAP_TEXT_DEFAULTS
    from texttoaudiogrounding_amd.models.text_encoder import LaionClapEncoder
    cfg = dict(CLAP_TEXT_DEFAULTS, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    enc = LaionClapEncoder(None, cfg)
    enc.load_state_dict(C.init_text_state(seed=5))
    enc = enc.to(dev).train()
    ids, mask = C.synthetic_tokens(a.R, a.L, seed=2)
    ids, mask = ids.to(dev), mask.to(dev)
    g = torch.Generator().manual_seed(1)
    wt, ws = torch.randn(a.R, a.L, 512, generator=g).to(dev), torch.randn(a.R, 512, generator=g).to(dev)
    st = {k: v.detach().clone().requires_grad_(True) for k, v in enc.named_parameters()}
    batch = {"input_ids": ids, "attention_mask": mask}

    def hip_fwd():
        with torch.no_grad():
            enc(batch)

    def hip_fwd_bwd():
        enc.zero_grad(set_to_none=True)
        o = enc(batch)
        ((o["token_emb"] * wt).sum() + (o["seq_emb"] * ws).sum()).backward()

    def eager_fwd():
        with torch.no_grad():
            eager_forward(st, ids, mask, 12)

    def eager_fwd_bwd():
        for v in st.values():
            v.grad = None
        tok, seq = eager_forward(st, ids, mask, 12)
        ((tok * wt).sum() + (seq * ws).sum()).backward()

    fns = {"hip_forward": hip_fwd, "hip_forward_backward": hip_fwd_bwd}
    if not a.no_eager:
        fns.update(eager_forward=eager_fwd, eager_forward_backward=eager_fwd_bwd)
    r = _time_alternating(fns, a.rounds, a.iters)
    dispatch.check_async_errors()
    M = a.R * a.L
    dense = sum(p.numel() for n, p in enc.named_parameters() if p.dim() == 2 and "embeddings" not in n)
    r["rows_M"], r["dense_parameters"] = M, dense
    r["flop_forward_backward"] = 6.0 * dense * M
    for side in ("hip",) + (() if a.no_eager else ("eager",)):
        r[f"{side}_forward_backward_mfma_frac"] = 6.0 * dense * M / (r[f"{side}_forward_backward"]["ms_median"] * 1e-3) / 1e12 / PEAK_FP32_MFMA
        r[f"{side}_forward_mfma_frac"] = 2.0 * dense * M / (r[f"{side}_forward"]["ms_median"] * 1e-3) / 1e12 / PEAK_FP32_MFMA
    if not a.no_eager:
        # agreement of the two stacks on the outputs (accuracy against fp64 is the tests' business: tests/test_gpu_text_clap.py)
        with torch.no_grad():
            o = enc(batch)
            tok, seq = eager_forward(st, ids, mask, 12)
        r["max_rel_output_diff_hip_vs_eager"] = {"token_emb": float((o["token_emb"] - tok).abs().max() / tok.abs().max()),
                                                 "seq_emb": float((o["seq_emb"] - seq).abs().max() / seq.abs().max())}
        for p in ("forward", "forward_backward"):
            r[f"ratio_hip_over_eager_{p}"] = r[f"hip_{p}"]["ms_median"] / r[f"eager_{p}"]["ms_median"]
    return {f"op_R{a.R}_L{a.L}": r}


def bench_step(a, dev):
    from oracle import clap_text_oracle as C
    from oracle import tag_oracle as O
    from texttoaudiogrounding_amd.models import audio_encoder, audio_text_model, match, text_encoder
    from texttoaudiogrounding_amd.models.hf_modeling_grounding import CLAP_TEXT_DEFAULTS
    from texttoaudiogrounding_amd.runner import StrongRunner
    torch.manual_seed(0)
    cfg = dict(CLAP_TEXT_DEFAULTS, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)

    def bi(te, freeze=False):
        return StrongRunner(audio_text_model.BiEncoder(audio_encoder.Cnn8Rnn(32000), te, match.DotProduct(), 512, add_proj=True,
                                                       freeze_text_encoder=freeze), device=dev)
    runners = {"clap_trainable": bi(text_encoder.LaionClapEncoder(None, cfg)),
               "clap_frozen": bi(text_encoder.LaionClapEncoder(None, cfg), True), "agg": bi(text_encoder.EmbeddingAgg(5221, 512))}
    batch = O.synthetic_batch(a.B, 320000, seed=99, ragged=True)
    ids, mask = C.synthetic_tokens(a.B, a.L, seed=2)
    batch.update(input_ids=ids, attention_mask=mask)
    batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}

    def strong(n):
        return lambda: runners[n].train_step({k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()})

    r = _time_alternating({n: strong(n) for n in runners}, a.rounds, a.steps)
    for n in ("clap_trainable", "clap_frozen"):
        r[f"{n}_minus_agg_ms"] = r[n]["ms_median"] - r["agg"]["ms_median"]
        r[f"ratio_{n}_over_agg"] = r[n]["ms_median"] / r["agg"]["ms_median"]
    return {f"strong_step_B{a.B}_L{a.L}": r}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["op", "step"], default="op")
    ap.add_argument("--R", type=int, default=512)
    ap.add_argument("--L", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = bench_op(a, dev) if a.mode == "op" else bench_step(a, dev)
    res["config"] = vars(a)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
