#!/usr/bin/env python3
"""tests/golden/text_intra.npz: the REFERENCE's models.text_encoder.IntraAttention on seeded cases, arrays only.

* four configurations (tests/text_intra_ref.CONFIGS; one over EmbeddingAgg, one with max(text_len) < L): token ids and lengths
  (1 and the longest included), the parameters (fp32; the position buffer is asserted equal to the restated table, not stored),
  the state-dict names and shapes, and from the reference with ``pe.dropout.p = 0`` and grad enabled in fp64 token_emb, seq_emb
  and every parameter gradient of the fixed random linear objective over both outputs (tests/text_intra_ref.objective_weights);
  per quantity the reference's own fp32-vs-fp64 deviation relative to the largest entry of the tensor.  Asserts that the
  restatement tests/text_intra_ref.py equals the reference to 1e-12 in fp64 first, that text_len = 0 runs in the reference
  with a finite token_emb (equal to the restatement's) and a NaN seq_emb, and that a 3-D ``text`` raises there.
* one whole-model case: BiEncoder(CrnnEncoder(32000, 256), IntraAttention(EmbeddingLayer(200, 256), 2), DotProduct(), 256) in
  eval mode at B = 2 x 1.5 s, weights and inputs drawn by seed (checksums stored, no weight tensors): frame_sim in fp64 and the
  reference's fp32 deviation from it.
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
from tests import text_intra_ref as R  # noqa: E402

ref_import.install()
from models.text_encoder import EmbeddingAgg, EmbeddingLayer, IntraAttention  # noqa: E402  (the reference)
from models.audio_encoder import CrnnEncoder  # noqa: E402
from models.audio_text_model import BiEncoder  # noqa: E402
from models.match import DotProduct  # noqa: E402


def build(cfg):
    inner = (EmbeddingAgg if cfg["agg"] else EmbeddingLayer)(cfg["V"], cfg["E"])
    model = IntraAttention(inner, cfg["layers"])
    model.pe.dropout.p = 0.0
    return model


def run_reference(cfg, st, text, text_len, dtype):
    model = build(cfg).to(dtype)
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
    st = R.draw_params(cfg["V"], cfg["E"], cfg["seed"], cfg["scale"], cfg["agg"])
    text, text_len = R.draw_inputs(cfg)
    assert int(text_len.max()) == (cfg["L"] - 1 if cfg["short"] else cfg["L"]) and int(text_len.min()) == 1
    fresh = build(cfg)
    assert torch.equal(fresh.pe.pe, st["pe.pe"]), "the restated position table differs from the reference's buffer"
    assert fresh.pe.dropout.p == 0.0 and IntraAttention(EmbeddingLayer(4, 8), 1).pe.dropout.p == 0.2
    assert all(float(getattr(fresh.conv_gru, g).bias.detach().abs().max()) == 0.0 for g in ("reset_gate", "update_gate", "out_gate"))
    model, g64 = run_reference(cfg, st, text, text_len, torch.float64)
    _, g32 = run_reference(cfg, st, text, text_len, torch.float32)
    sd = model.state_dict()
    assert list(sd) == R.state_names(cfg["agg"]), list(sd)
    assert [k for k, _ in model.named_parameters()] == R.param_names(cfg["agg"])
    assert model.embed_dim == cfg["E"] and model.num_layers == cfg["layers"] and model.pooling == "mean"
    mine = R.config_results(cfg, st, text, text_len, torch.float64)
    err = max(R.rel_err(mine[k], g64[k]) for k in g64)
    print(f"{name}: restatement vs reference (fp64) {err:.2e}")
    assert err < 1e-12 and set(mine) == set(g64)
    # text_len = 0: the reference runs; token_emb finite and equal to the restatement's, seq_emb of that row 0/0
    ztext, zlen = R.draw_inputs(cfg, zero=True)
    m64 = build(cfg).double()
    m64.load_state_dict({k: v.double() for k, v in st.items()})
    with torch.no_grad():
        zo = m64({"text": ztext, "text_len": zlen})
    ztok, zseq = R.encoder_forward({k: v.double() for k, v in st.items()}, ztext, zlen, cfg["layers"], agg=cfg["agg"])
    assert torch.isfinite(zo["token_emb"]).all() and R.rel_err(ztok, zo["token_emb"]) < 1e-12
    assert torch.isnan(zo["seq_emb"][0]).all() and torch.isnan(zseq[0]).all() and R.rel_err(zseq[1:], zo["seq_emb"][1:]) < 1e-12
    try:
        m64({"text": text.view(2, -1, cfg["L"]), "text_len": text_len.view(2, -1)})
        raise SystemExit("the reference was expected to raise on a 3-D text")
    except (ValueError, RuntimeError) as e:
        print(f"{name}: reference on a 3-D text raises: {str(e)[:90]}")
    out[f"{name}_text"] = text.numpy().astype(np.int16)
    out[f"{name}_text_len"] = text_len.numpy().astype(np.int16)
    out[f"{name}_keys"] = np.array(list(sd))
    out[f"{name}_shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
    for k in R.param_names(cfg["agg"]):                    # the position buffer is not stored: asserted equal to the restated one above
        out[f"{name}_param_{k}"] = st[k].numpy()
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
    model = BiEncoder(CrnnEncoder(32000, 256), IntraAttention(EmbeddingLayer(m["V"], m["E"]), m["layers"]), DotProduct(), 256).eval()
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

path = os.path.join(HERE, "text_intra.npz")
np.savez_compressed(path, **out)
print(f"wrote text_intra.npz ({os.path.getsize(path)} bytes)")
