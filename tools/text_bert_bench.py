#!/usr/bin/env python3
"""The BERT text encoders (Bert / SentenceBert, csrc/text_bert.hip + the encoder stack of the CLAP tower) and the phrase embedder,
timed with device events, the legs alternated in one process, medians over rounds.  Prints one JSON object.

--mode embed (default): --N synthetic phrases (32768), token counts drawn from a fixed seeded distribution over 3 ... 16
  ([CLS] and [SEP] included), all-MiniLM-L6-v2's shape, forward-only through utils.text_embed.PhraseEmbedder (sorted by token
  count, batches padded to their own longest phrase).  Legs: ``bucketed`` (the embedder); ``padded16`` (the same tower on fixed
  batches of the same padded size in input order, every phrase padded to 16 tokens); and, when ``transformers`` imports,
  ``hf_eager`` (``BertModel`` eager fp32 + the masked mean + normalize on the same GPU on the SAME bucketed batches).  Tokenising
  is outside the timed region; the host-to-device copies of the batches and the device-to-host copy of the result are inside.
--mode op: forward and forward + backward of ``Bert`` at BERT-base shape on R = --R phrases x L = --L tokens, dropouts 0, against
  the SAME layer stack written in plain torch and run eagerly on the same GPU in fp32 (the counterpart of
  tools/text_clap_bench.py --mode op).
--mode step: BiEncoder(Cnn8Rnn, Bert, DotProduct, add_proj) through StrongRunner.train_step at B x 10 s, trainable and frozen,
  against the same step with EmbeddingAgg(5221, 512) (the harness of tools/text_clap_bench.py --mode step).

    python tools/text_bert_bench.py [--mode embed|op|step] [--N 32768] [--batch_tokens 16384] [--R 512] [--L 12] [--rounds 5]
        [--iters 5] [--B 64] [--steps 3] [--no-eager] [--out F.json]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.text_clap_bench import PEAK_FP32_MFMA, _time_alternating  # noqa: E402


class SyntheticTokenizer:
    """Phrases are strings of integers: the token ids between [CLS] = 101 and [SEP] = 102."""
    pad_token_id = 0

    def __call__(self, texts, truncation=True, max_length=64, padding=False):
        rows = [([101] + [int(w) for w in t.split()])[:max_length - 1] + [102] for t in texts]
        return {"input_ids": rows, "token_type_ids": [[0] * len(r) for r in rows]}


def synthetic_phrases(n, vocab, seed=7, lo=3, hi=16):
    """n phrases whose token counts ([CLS] / [SEP] included) follow a fixed seeded distribution over lo ... hi that peaks at 5 - 6
    tokens, like sound-event phrases."""
    rng = np.random.RandomState(seed)
    counts = np.arange(lo, hi + 1)
    p = np.exp(-0.5 * ((counts - 5.5) / 2.5) ** 2) + 0.02
    lens = rng.choice(counts, size=n, p=p / p.sum())
    return [" ".join(str(x) for x in rng.randint(1000, vocab, size=k - 2)) for k in lens], lens


def eager_bert(st, ids, tps, mask, heads, eps=1e-12):
    """BertModel's layer stack in plain torch on whatever device st lives on -> the last hidden state (R, L, D)."""
    import torch.nn.functional as F
    g = lambda k: st["model." + k]                               # noqa: E731
    R, L = ids.shape
    h = F.embedding(ids, g("embeddings.word_embeddings.weight"), padding_idx=0) \
        + F.embedding(tps, g("embeddings.token_type_embeddings.weight")) + g("embeddings.position_embeddings.weight")[:L]
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
    return h


def bench_embed(a, dev):
    from texttoaudiogrounding_amd import dispatch
    from texttoaudiogrounding_amd.models.text_encoder import MINILM_DEFAULTS, SentenceBert
    from texttoaudiogrounding_amd.utils.text_embed import PhraseEmbedder
    torch.manual_seed(0)
    enc = SentenceBert(None, dict(MINILM_DEFAULTS)).to(dev).eval()
    emb = PhraseEmbedder(enc, SyntheticTokenizer(), batch_tokens=a.batch_tokens, max_length=16)
    phrases, lens = synthetic_phrases(a.N, MINILM_DEFAULTS["vocab_size"])
    ids, types = emb.tokenize(phrases)
    plan = emb.plan([len(x) for x in ids], a.batch_tokens)
    bucketed = [emb.batch(ids, types, index) for index in plan]
    per = max(1, a.batch_tokens // 16)
    fixed = []
    for i in range(0, a.N, per):
        b = emb.batch(ids, types, list(range(i, min(i + per, a.N))))
        pad = 16 - b["input_ids"].shape[1]
        fixed.append({k: torch.nn.functional.pad(v, (0, pad)) for k, v in b.items()})

    def run(batches, model):
        out = []
        with torch.no_grad():
            for b in batches:
                out.append(model(b))
        return torch.cat(out).cpu()

    fns = {"bucketed": lambda: run(bucketed, lambda b: enc(b)["seq_emb"]), "padded16": lambda: run(fixed, lambda b: enc(b)["seq_emb"])}
    r = {"phrases": a.N, "token_count_mean": float(np.mean(lens)), "batches_bucketed": len(bucketed), "batches_padded16": len(fixed),
         "padded_tokens_bucketed": int(sum(b["input_ids"].numel() for b in bucketed)),
         "padded_tokens_padded16": int(sum(b["input_ids"].numel() for b in fixed)), "valid_tokens": int(np.sum(lens))}
    hf = None
    if not a.no_eager:
        try:
            from transformers import BertConfig, BertModel
            hc = BertConfig(**MINILM_DEFAULTS)
            hc._attn_implementation = "eager"
            hf = BertModel(hc, add_pooling_layer=False)
            hf.load_state_dict({k[len("model."):]: v for k, v in enc.state_dict().items()
                                if k.startswith("model.") and "pooler" not in k}, strict=False)
            hf = hf.to(dev).eval()
        except Exception as e:                              # noqa: BLE001
            r["hf_eager"] = f"not measured ({type(e).__name__}: {e})"
    if hf is not None:
        def hf_model(b):
            b = {k: v.to(dev) for k, v in b.items()}
            tok = hf(**b).last_hidden_state
            m = b["attention_mask"].unsqueeze(-1).to(tok.dtype)
            return torch.nn.functional.normalize((tok * m).sum(1) / m.sum(1).clamp_min(1e-9), dim=-1)
        fns["hf_eager"] = lambda: run(bucketed, hf_model)
    r.update(_time_alternating(fns, a.rounds, 1, warm=1))
    dispatch.check_async_errors()
    order = torch.as_tensor([i for index in plan for i in index])
    got = run(bucketed, lambda b: enc(b)["seq_emb"])
    ref = run(fixed, lambda b: enc(b)["seq_emb"])[order]
    r["max_abs_diff_bucketed_vs_padded16"] = float((got - ref).abs().max())
    if hf is not None:
        r["max_abs_diff_bucketed_vs_hf_eager"] = float((got - run(bucketed, hf_model)).abs().max())
    for n in fns:
        r[f"phrases_per_s_{n}"] = a.N / (r[n]["ms_median"] * 1e-3)
        if n != "bucketed":
            r[f"ratio_bucketed_over_{n}"] = r["bucketed"]["ms_median"] / r[n]["ms_median"]
    return {f"embed_N{a.N}": r}


def bench_op(a, dev):
    from texttoaudiogrounding_amd import dispatch
    from texttoaudiogrounding_amd.models.text_encoder import BERT_DEFAULTS, Bert
    torch.manual_seed(0)
    cfg = dict(BERT_DEFAULTS, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    enc = Bert(None, cfg).to(dev).train()
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(1000, cfg["vocab_size"], (a.R, a.L), generator=g)
    klen = torch.randint(3, a.L + 1, (a.R,), generator=g)
    mask = (torch.arange(a.L)[None, :] < klen[:, None]).long()
    ids = ids * mask
    tps = torch.zeros_like(ids)
    ids, tps, mask = ids.to(dev), tps.to(dev), mask.to(dev)
    D = cfg["hidden_size"]
    wt, ws = torch.randn(a.R, a.L, D, generator=g).to(dev), torch.randn(a.R, D, generator=g).to(dev)
    st = {k: v.detach().clone().requires_grad_(True) for k, v in enc.named_parameters() if k.startswith("model.") and "pooler" not in k}
    batch = {"input_ids": ids, "token_type_ids": tps, "attention_mask": mask}

    def hip_fwd():
        with torch.no_grad():
            enc(batch)

    def hip_fwd_bwd():
        enc.zero_grad(set_to_none=True)
        o = enc(batch)
        ((o["token_emb"] * wt).sum() + (o["seq_emb"] * ws).sum()).backward()

    def eager_fwd():
        with torch.no_grad():
            eager_bert(st, ids, tps, mask, 12)

    def eager_fwd_bwd():
        for v in st.values():
            v.grad = None
        tok = eager_bert(st, ids, tps, mask, 12)
        ((tok * wt).sum() + (tok[:, 0] * ws).sum()).backward()

    fns = {"hip_forward": hip_fwd, "hip_forward_backward": hip_fwd_bwd}
    if not a.no_eager:
        fns.update(eager_forward=eager_fwd, eager_forward_backward=eager_fwd_bwd)
    r = _time_alternating(fns, a.rounds, a.iters)
    dispatch.check_async_errors()
    M = a.R * a.L
    dense = sum(p.numel() for n, p in st.items() if p.dim() == 2 and "embeddings" not in n)
    r["rows_M"], r["dense_parameters"] = M, dense
    for side in ("hip",) + (() if a.no_eager else ("eager",)):
        r[f"{side}_forward_backward_mfma_frac"] = 6.0 * dense * M / (r[f"{side}_forward_backward"]["ms_median"] * 1e-3) / 1e12 / PEAK_FP32_MFMA
        r[f"{side}_forward_mfma_frac"] = 2.0 * dense * M / (r[f"{side}_forward"]["ms_median"] * 1e-3) / 1e12 / PEAK_FP32_MFMA
    if not a.no_eager:
        with torch.no_grad():
            o = enc(batch)
            tok = eager_bert(st, ids, tps, mask, 12)
        r["max_rel_output_diff_hip_vs_eager"] = float((o["token_emb"] - tok).abs().max() / tok.abs().max())
        for p in ("forward", "forward_backward"):
            r[f"ratio_hip_over_eager_{p}"] = r[f"hip_{p}"]["ms_median"] / r[f"eager_{p}"]["ms_median"]
    return {f"op_R{a.R}_L{a.L}": r}


def bench_step(a, dev):
    from oracle import tag_oracle as O
    from texttoaudiogrounding_amd.models import audio_encoder, audio_text_model, match, text_encoder
    from texttoaudiogrounding_amd.runner import StrongRunner
    torch.manual_seed(0)
    cfg = dict(text_encoder.BERT_DEFAULTS, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)

    def bi(te, freeze=False):
        return StrongRunner(audio_text_model.BiEncoder(audio_encoder.Cnn8Rnn(32000), te, match.DotProduct(), 512, add_proj=True,
                                                       freeze_text_encoder=freeze), device=dev)
    runners = {"bert_trainable": bi(text_encoder.Bert(None, cfg)), "bert_frozen": bi(text_encoder.Bert(None, cfg), True),
               "agg": bi(text_encoder.EmbeddingAgg(5221, 512))}
    batch = O.synthetic_batch(a.B, 320000, seed=99, ragged=True)
    g = torch.Generator().manual_seed(2)
    klen = torch.randint(3, a.L + 1, (a.B,), generator=g)
    mask = (torch.arange(a.L)[None, :] < klen[:, None]).long()
    ids = torch.randint(1000, cfg["vocab_size"], (a.B, a.L), generator=g) * mask
    batch.update(input_ids=ids, token_type_ids=torch.zeros_like(ids), attention_mask=mask)
    batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}

    def strong(n):
        return lambda: runners[n].train_step({k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()})

    r = _time_alternating({n: strong(n) for n in runners}, a.rounds, a.steps)
    for n in ("bert_trainable", "bert_frozen"):
        r[f"{n}_minus_agg_ms"] = r[n]["ms_median"] - r["agg"]["ms_median"]
        r[f"ratio_{n}_over_agg"] = r[n]["ms_median"] / r["agg"]["ms_median"]
    return {f"strong_step_B{a.B}_L{a.L}": r}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["embed", "op", "step"], default="embed")
    ap.add_argument("--N", type=int, default=32768)
    ap.add_argument("--batch_tokens", type=int, default=16384)
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
    res = {"embed": bench_embed, "op": bench_op, "step": bench_step}[a.mode](a, dev)
    res["config"] = vars(a)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
