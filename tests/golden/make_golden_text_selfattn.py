#!/usr/bin/env python3
"""tests/golden/text_selfattn.npz: the REFERENCE's models.text_encoder.SelfAttention on seeded cases, arrays only.

* three configurations (tests/text_selfattn_ref.CONFIGS): token ids and lengths (1 and L included, max == L: the reference
  raises otherwise), the parameters (fp32; the position buffer is asserted equal to the restated table, not stored), the
  state-dict names and shapes, and from the
  reference with dropout 0 and grad enabled in fp64 token_emb, seq_emb and every parameter gradient of the fixed random linear
  objective over both outputs (tests/text_selfattn_ref.objective_weights); per quantity the reference's own fp32-vs-fp64
  deviation relative to the largest entry of the tensor.  Asserts that the restatement tests/text_selfattn_ref.py equals the
  reference to 1e-12 in fp64 first, and that the reference does raise when max(text_len) < L.
* one whole-model case: BiEncoder(CrnnEncoder(32000, 256), SelfAttention(200, 256, 4, 0.0), DotProduct(), 256) in eval mode at
  B = 2 x 1.5 s, weights and inputs drawn by seed (checksums stored, no weight tensors): frame_sim in fp64 and the reference's
  fp32 deviation from it.
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
from tests import text_selfattn_ref as R  # noqa: E402

ref_import.install()
from models.text_encoder import SelfAttention  # noqa: E402  (the reference)
from models.audio_encoder import CrnnEncoder  # noqa: E402
from models.audio_text_model import BiEncoder  # noqa: E402
from models.match import DotProduct  # noqa: E402


def run_reference(cfg, st, text, text_len, dtype):
    model = SelfAttention(cfg["V"], cfg["E"], cfg["heads"], 0.0).to(dtype)
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
    st = R.draw_params(cfg["V"], cfg["E"], cfg["heads"], cfg["seed"])
    text, text_len = R.draw_inputs(cfg)
    assert int(text_len.max()) == cfg["L"] and int(text_len.min()) == 1
    fresh = SelfAttention(cfg["V"], cfg["E"], cfg["heads"], 0.0)
    assert torch.equal(fresh.pe.pe, st["pe.pe"]), "the restated position table differs from the reference's buffer"
    assert float(fresh.cls_token.detach().abs().max()) == 0.0
    model, g64 = run_reference(cfg, st, text, text_len, torch.float64)
    _, g32 = run_reference(cfg, st, text, text_len, torch.float32)
    sd = model.state_dict()
    assert list(sd) == R.STATE_NAMES, list(sd)
    assert [k for k, _ in model.named_parameters()] == R.PARAM_NAMES
    assert model.embed_dim == cfg["E"]
    mine = R.config_results(cfg, st, text, text_len, torch.float64)
    err = max(R.rel_err(mine[k], g64[k]) for k in g64)
    print(f"{name}: restatement vs reference (fp64) {err:.2e}")
    assert err < 1e-12 and set(mine) == set(g64)
    short_text, short_len = R.draw_inputs(cfg, full=False)
    try:
        model({"text": short_text, "text_len": short_len})
        raise SystemExit("the reference was expected to raise when max(text_len) < L")
    except (AssertionError, RuntimeError) as e:
        print(f"{name}: reference with max(text_len) < L raises: {str(e)[:90]}")
    out[f"{name}_text"] = text.numpy().astype(np.int16)
    out[f"{name}_text_len"] = text_len.numpy().astype(np.int16)
    out[f"{name}_keys"] = np.array(list(sd))
    out[f"{name}_shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
    for k in R.PARAM_NAMES:                                # the position buffer is not stored: asserted equal to the restated one above
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
    model = BiEncoder(CrnnEncoder(32000, 256), SelfAttention(m["V"], m["E"], m["heads"], 0.0), DotProduct(), 256).eval()
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

path = os.path.join(HERE, "text_selfattn.npz")
np.savez_compressed(path, **out)
print(f"wrote text_selfattn.npz ({os.path.getsize(path)} bytes)")
