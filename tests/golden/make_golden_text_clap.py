#!/usr/bin/env python3
"""tests/golden/text_clap.npz: the REAL Hugging Face modules the reference's models.text_encoder.LaionClapEncoder wraps
(ClapModel.text_model = ClapTextModel, ClapModel.text_projection = ClapProjectionLayer; models/text_encoder.py:311-327) on the
tiny configuration tests/text_clap_ref.TINY (hidden 64, 4 heads, 2 layers, FFN 160, vocab 120, dropouts 0), forward AND backward
of the fixed weighted objective over token_emb and seq_emb (tests/text_clap_ref.objective), in fp64 and in fp32.  Arrays only:

* the inputs (input_ids, attention_mask), the state-dict keys and shapes of the reference's module (``model.*``,
  ``projection.*``), the quantity names, the fp64 outputs and every parameter gradient, and per quantity the fp32 run's
  deviation from fp64 relative to the tensor's largest entry;
* parameters are drawn from a seed (tests/text_clap_ref.draw_state) and NOT stored.

Asserts first that the restatement tests/text_clap_ref.py reproduces the modules in fp64 to 1e-12 on every quantity, and that the
pad rows of the two padded tables receive exactly zero gradient.  Build container only (needs ``transformers``)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import text_clap_ref as R  # noqa: E402

import transformers  # noqa: E402
from transformers.models.clap.configuration_clap import ClapTextConfig  # noqa: E402
from transformers.models.clap.modeling_clap import ClapProjectionLayer, ClapTextModel  # noqa: E402

CFG, FX = R.TINY, R.FIXTURE
hf_cfg = ClapTextConfig(**CFG)
hf_cfg._attn_implementation = "eager"
st = R.draw_state(CFG, FX["state_seed"])
ids, mask = R.draw_inputs(FX["R"], FX["L"], FX["input_seed"], CFG["vocab_size"], CFG["pad_token_id"])
assert int(mask.sum(-1).min()) == 2 and int(mask.sum(-1).max()) == FX["L"]
_softmax = torch.nn.functional.softmax


def _softmax_keep_dtype(x, dim=None, _stacklevel=3, dtype=None):
    # the eager attention upcasts its softmax to fp32 (meant for half precision): in the fp64 run no stage may round to fp32
    return _softmax(x, dim=dim, dtype=torch.float64 if x.dtype == torch.float64 else dtype)


def run_modules(dtype):
    text = ClapTextModel(hf_cfg, add_pooling_layer=True).train()         # dropouts are 0: train and eval compute the same thing
    proj = ClapProjectionLayer(hf_cfg).train()
    missing = text.load_state_dict({k[len("model."):]: v for k, v in st.items() if k.startswith("model.")}, strict=False)
    assert not missing.unexpected_keys and set(missing.missing_keys) <= {"embeddings.position_ids", "embeddings.token_type_ids"}
    proj.load_state_dict({k[len("projection."):]: v for k, v in st.items() if k.startswith("projection.")}, strict=True)
    text, proj = text.to(dtype), proj.to(dtype)
    torch.nn.functional.softmax = _softmax_keep_dtype
    try:
        o = text(input_ids=ids, attention_mask=mask)
        tok = proj(o.last_hidden_state)
        seq = torch.nn.functional.normalize(proj(o.pooler_output), dim=-1)
        wt, ws = R.objective_weights(*tok.shape, FX["objective_seed"], dtype)
        R.objective(tok, seq, wt, ws).backward()
    finally:
        torch.nn.functional.softmax = _softmax
    got = {"token_emb": tok.detach(), "seq_emb": seq.detach()}
    got.update({"dmodel." + k: p.grad for k, p in text.named_parameters()})
    got.update({"dprojection." + k: p.grad for k, p in proj.named_parameters()})
    sd = {"model." + k: v for k, v in text.state_dict().items()}
    sd.update({"projection." + k: v for k, v in proj.state_dict().items()})
    return got, sd


g64, sd = run_modules(torch.float64)
g32, _ = run_modules(torch.float32)
names = R.param_names(CFG["num_hidden_layers"])
assert sorted(g64) == sorted(["token_emb", "seq_emb"] + ["d" + k for k in names]), sorted(g64)
assert sorted(k for k in sd if not k.endswith("_ids")) == sorted(names), list(sd)     # (registration order differs: sorted)
mine = R.results(st, ids, mask, CFG["num_attention_heads"], torch.float64, CFG["layer_norm_eps"], CFG["pad_token_id"],
                 FX["objective_seed"])
err = {k: R.quantity_err(mine, g64, k) for k in g64}
print(f"transformers {transformers.__version__}: restatement vs ClapTextModel + ClapProjectionLayer (fp64), worst "
      f"{max(err.values()):.2e} ({max(err, key=err.get)})")
assert max(err.values()) < 1e-12
pad = CFG["pad_token_id"]
for k in ("dmodel.embeddings.word_embeddings.weight", "dmodel.embeddings.position_embeddings.weight"):
    assert float(g64[k][pad].abs().max()) == 0.0 and float(g64[k].abs().max()) > 0.0, k

quantities = sorted(g64)
out = {"input_ids": ids.numpy().astype(np.int16), "attention_mask": mask.numpy().astype(np.int8),
       "keys": np.array(list(sd)), "shapes": np.array([",".join(map(str, v.shape)) for v in sd.values()]),
       "quantities": np.array(quantities), "f32_dev": np.array([R.quantity_err(g32, g64, k) for k in quantities]),
       "transformers_version": np.array(transformers.__version__)}
for k in quantities:
    out["f64_" + k] = g64[k].numpy()
worst = max(zip(out["f32_dev"].tolist(), quantities))
print(f"modules fp32 vs fp64: token_emb {R.rel_err(g32['token_emb'], g64['token_emb']):.2e}, seq_emb "
      f"{R.rel_err(g32['seq_emb'], g64['seq_emb']):.2e}, worst {worst[0]:.2e} ({worst[1]})")
path = os.path.join(HERE, "text_clap.npz")
np.savez_compressed(path, **out)
print(f"wrote text_clap.npz ({os.path.getsize(path)} bytes)")
