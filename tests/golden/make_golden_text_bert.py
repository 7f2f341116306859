#!/usr/bin/env python3
"""tests/golden/text_bert.npz (+ text_bert_mean_norm.npz, text_bert_mean.npz: one file per case): the REAL Hugging Face
``BertModel`` the reference's models.text_encoder.Bert / SentenceBert wrap
(models/text_encoder.py:271-308) on the tiny configuration tests/text_bert_ref.TINY (hidden 64, 4 heads, 2 layers, FFN 160, vocab
120, 72 positions, 2 types, pad id 0, dropouts 0), forward AND backward of the fixed weighted objective over token_emb and seq_emb
(tests/text_bert_ref.objective), for the three cases of tests/text_bert_ref.CASES -- [CLS], mean + normalize, mean -- in fp64 and
in fp32.  The poolings on top of the module are sentence-transformers' ``Pooling`` / ``Normalize`` written out (the masked mean
``sum(h * mask) / clamp(sum(mask), 1e-9)`` and ``F.normalize``).  Arrays only:

* the inputs (input_ids, token_type_ids, attention_mask), the state-dict keys and shapes of the module under ``model.``, and per
  case the quantity names, the fp64 outputs and every parameter gradient, and per quantity the fp32 run's deviation from fp64
  relative to the tensor's largest entry;
* parameters are drawn from a seed (tests/text_bert_ref.draw_state) and NOT stored.

Asserts first that the restatement tests/text_bert_ref.py reproduces the module in fp64 to 1e-12 on every quantity, that the pad
row of the word table receives exactly zero gradient and that the pooler receives none.  Needs ``transformers``."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import text_bert_ref as R  # noqa: E402

import transformers  # noqa: E402
from transformers import BertConfig, BertModel  # noqa: E402

CFG, FX = R.TINY, R.FIXTURE
hf_cfg = BertConfig(**CFG)
hf_cfg._attn_implementation = "eager"
st = R.draw_state(CFG, FX["state_seed"])
ids, tps, mask = R.draw_inputs(FX["R"], FX["L"], FX["input_seed"], CFG["vocab_size"], CFG["type_vocab_size"], CFG["pad_token_id"])
assert int(mask.sum(-1).min()) == 2 and int(mask.sum(-1).max()) == FX["L"] and int(tps.max()) == 1
_softmax = torch.nn.functional.softmax


def _softmax_keep_dtype(x, dim=None, _stacklevel=3, dtype=None):
    # the eager attention may upcast its softmax to fp32 (meant for half precision): in the fp64 run no stage may round to fp32
    return _softmax(x, dim=dim, dtype=torch.float64 if x.dtype == torch.float64 else dtype)


def run_module(dtype, mode, norm):
    bert = BertModel(hf_cfg, add_pooling_layer=True).train()             # dropouts are 0: train and eval compute the same thing
    missing = bert.load_state_dict({k[len("model."):]: v for k, v in st.items()}, strict=False)
    assert not missing.unexpected_keys and set(missing.missing_keys) <= {"embeddings.position_ids", "embeddings.token_type_ids"}
    bert = bert.to(dtype)
    torch.nn.functional.softmax = _softmax_keep_dtype
    try:
        tok = bert(input_ids=ids, token_type_ids=tps, attention_mask=mask).last_hidden_state
        if mode == 0:
            seq = tok[:, 0]
        else:
            m = mask.unsqueeze(-1).expand(tok.size()).to(tok.dtype)
            seq = torch.sum(tok * m, 1) / torch.clamp(m.sum(1), min=1e-9)
        if norm == 1:
            seq = torch.nn.functional.normalize(seq, p=2, dim=1)
        wt, ws = R.objective_weights(*tok.shape, FX["objective_seed"], dtype)
        R.objective(tok, seq, wt, ws).backward()
    finally:
        torch.nn.functional.softmax = _softmax
    got = {"token_emb": tok.detach(), "seq_emb": seq.detach()}
    for k, p in bert.named_parameters():
        if k.startswith("pooler."):
            assert p.grad is None, k
        else:
            got["dmodel." + k] = p.grad
    return got, {"model." + k: v for k, v in bert.state_dict().items()}


names = R.param_names(CFG["num_hidden_layers"])
out = {"input_ids": ids.numpy().astype(np.int16), "token_type_ids": tps.numpy().astype(np.int8),
       "attention_mask": mask.numpy().astype(np.int8), "cases": np.array(list(R.CASES)),
       "transformers_version": np.array(transformers.__version__)}
for case, (mode, norm) in R.CASES.items():
    g64, sd = run_module(torch.float64, mode, norm)
    g32, _ = run_module(torch.float32, mode, norm)
    assert sorted(g64) == sorted(["token_emb", "seq_emb"] + ["d" + k for k in names]), sorted(g64)
    assert sorted(k for k in sd if not k.endswith("_ids")) == sorted(R.param_names(CFG["num_hidden_layers"], True)), list(sd)
    mine = R.results(st, ids, tps, mask, CFG["num_attention_heads"], mode, norm, torch.float64, CFG["layer_norm_eps"],
                     CFG["pad_token_id"], FX["objective_seed"])
    err = {k: R.quantity_err(mine, g64, k) for k in g64}
    print(f"{case}: restatement vs BertModel (fp64), worst {max(err.values()):.2e} ({max(err, key=err.get)})")
    assert max(err.values()) < 1e-12
    k = "dmodel.embeddings.word_embeddings.weight"
    assert float(g64[k][CFG["pad_token_id"]].abs().max()) == 0.0 and float(g64[k].abs().max()) > 0.0
    quantities = sorted(g64)
    out["keys"] = np.array(list(sd))
    out["shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
    out["quantities"] = np.array(quantities)
    out[case + "_f32_dev"] = np.array([R.quantity_err(g32, g64, k) for k in quantities])
    for k in quantities:
        out[f"{case}_f64_{k}"] = g64[k].numpy()
    worst = max(zip(out[case + "_f32_dev"].tolist(), quantities))
    print(f"{case}: module fp32 vs fp64: worst {worst[0]:.2e} ({worst[1]})")
# one file per case: the three sets of fp64 gradients together exceed the size a committed file may have
for case in R.CASES:
    part = {k: v for k, v in out.items() if not any(k.startswith(c + "_f") for c in R.CASES) or k.startswith(case + "_f")}
    path = os.path.join(HERE, "text_bert.npz" if case == "cls" else f"text_bert_{case}.npz")
    np.savez_compressed(path, **part)
    print(f"transformers {transformers.__version__}: wrote {os.path.basename(path)} ({os.path.getsize(path)} bytes)")
