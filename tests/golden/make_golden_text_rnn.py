#!/usr/bin/env python3
"""tests/golden/text_rnn.npz: the REFERENCE's models.text_encoder.RnnEncoder on seeded cases, arrays only.

* three configurations (tests/text_rnn_ref.CONFIGS: 2 layers bidirectional, 1 layer bidirectional, 2 layers unidirectional):
  token ids and lengths, the parameters (fp32), the state-dict names and shapes, and from the reference in fp64 token_emb,
  seq_emb and every parameter gradient of the fixed random linear objective over both outputs
  (tests/text_rnn_ref.objective_weights); per quantity the reference's own fp32-vs-fp64 deviation relative to the largest
  entry of the tensor.  Asserts that the restatement tests/text_rnn_ref.py equals the reference to 1e-12 in fp64 first.
* one whole-model case: BiEncoder(CrnnEncoder(32000, 256), RnnEncoder(200, 32, 128, 1, 0, True, "GRU"), DotProduct(), 256) in
  eval mode at B = 2 x 1.5 s, weights and inputs drawn by seed (checksums stored, no weight tensors): frame_sim in fp64 and
  the reference's fp32 deviation from it.
Build container only."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import ref_import  # noqa: E402
from tests import text_rnn_ref as R  # noqa: E402

ref_import.install()
from models.text_encoder import RnnEncoder  # noqa: E402  (the reference)
from models.audio_encoder import CrnnEncoder  # noqa: E402
from models.audio_text_model import BiEncoder  # noqa: E402
from models.match import DotProduct  # noqa: E402


def run_reference(cfg, st, text, text_len, dtype):
    model = RnnEncoder(cfg["V"], cfg["E"], cfg["H"], cfg["layers"], 0.0, cfg["dirs"] == 2, "GRU").to(dtype)
    missing = model.load_state_dict({k: v.to(dtype) for k, v in st.items()}, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    model.train()                                         # dropout 0: train and eval compute the same thing
    o = model({"text": text, "text_len": text_len})
    wt, ws = R.objective_weights(cfg, dtype)
    R.objective(o["token_emb"], o["seq_emb"], wt, ws).backward()
    got = {"token_emb": o["token_emb"].detach(), "seq_emb": o["seq_emb"].detach()}
    got.update({"d" + k: p.grad for k, p in model.named_parameters()})
    return model, got


out = {}
for name, cfg in R.CONFIGS.items():
    st = R.draw_params(cfg["V"], cfg["E"], cfg["H"], cfg["layers"], cfg["dirs"], cfg["seed"])
    text, text_len = R.draw_inputs(cfg)
    model, g64 = run_reference(cfg, st, text, text_len, torch.float64)
    _, g32 = run_reference(cfg, st, text, text_len, torch.float32)
    sd = model.state_dict()
    assert list(sd) == R.param_names(cfg["layers"], cfg["dirs"]), list(sd)
    assert model.embed_dim == cfg["H"] * cfg["dirs"]
    mine = R.config_results(cfg, st, text, text_len, torch.float64)
    err = max(R.rel_err(mine[k], g64[k]) for k in g64)
    print(f"{name}: restatement vs reference (fp64) {err:.2e}")
    assert err < 1e-12 and set(mine) == set(g64)
    out[f"{name}_text"] = text.numpy().astype(np.int16)
    out[f"{name}_text_len"] = text_len.numpy().astype(np.int16)
    out[f"{name}_keys"] = np.array(list(sd))
    out[f"{name}_shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
    for k, v in st.items():
        out[f"{name}_param_{k}"] = v.numpy()
    quantities = sorted(g64)
    out[f"{name}_quantities"] = np.array(quantities)
    out[f"{name}_f32_dev"] = np.array([R.rel_err(g32[k], g64[k]) for k in quantities])
    for k in quantities:
        out[f"{name}_f64_{k}"] = g64[k].numpy()
    worst = max(zip(out[f"{name}_f32_dev"].tolist(), quantities))
    print(f"{name}: reference fp32 vs fp64: token_emb {R.rel_err(g32['token_emb'], g64['token_emb']):.2e}, seq_emb "
          f"{R.rel_err(g32['seq_emb'], g64['seq_emb']):.2e}, worst {worst[0]:.2e} ({worst[1]})")

# ---- the whole-model case ----
m = R.MODEL
st = R.model_state()
batch = R.model_batch()


def run_model(dtype):
    model = BiEncoder(CrnnEncoder(32000, 256), RnnEncoder(m["V"], m["E"], m["H"], m["layers"], 0.0, m["dirs"] == 2, "GRU"),
                      DotProduct(), 256).eval()
    missing = model.load_state_dict(st, strict=False)
    assert not missing.unexpected_keys and not missing.missing_keys, missing
    model = model.to(dtype)
    with torch.no_grad():
        o = model({"waveform": batch["waveform"].to(dtype), "waveform_len": torch.as_tensor(batch["waveform_len"]),
                   "text": batch["text"], "text_len": torch.as_tensor(batch["text_len"]), "specaug": False})
    return model, o


model, o64 = run_model(torch.float64)
_, o32 = run_model(torch.float32)
dev = R.rel_err(o32["frame_sim"], o64["frame_sim"])
print(f"model: frame_sim {tuple(o64['frame_sim'].shape)}, length {torch.as_tensor(o64['length']).tolist()}, range "
      f"[{o64['frame_sim'].min().item():.3f}, {o64['frame_sim'].max().item():.3f}]; reference fp32 vs fp64 {dev:.2e}")
out["model_keys"] = np.array([k for k in model.state_dict() if k.startswith("text_encoder.")])
out["model_frame_sim_f64"] = o64["frame_sim"].numpy()
out["model_frame_sim_f32_dev"] = np.array(dev)
out["model_length"] = torch.as_tensor(o64["length"]).long().numpy()
out["model_state_checksum"] = R.state_checksum(st)
out["model_waveform_checksum"] = np.array(R.checksum(batch["waveform"]))
out["model_text"] = batch["text"].numpy().astype(np.int16)
out["model_text_len"] = np.asarray(batch["text_len"]).astype(np.int16)

path = os.path.join(HERE, "text_rnn.npz")
np.savez_compressed(path, **out)
print(f"wrote text_rnn.npz ({os.path.getsize(path)} bytes)")
