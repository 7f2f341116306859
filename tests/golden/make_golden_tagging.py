#!/usr/bin/env python3
"""tests/golden/audio_tagging.npz: the REFERENCE's class-mapping baseline (models.audio_text_model.AudioTagging,
losses.ClipBceLoss / MaskedFrameBceLoss / ClipMaskedFrameBceLoss) on seeded cases, arrays only.

* head level: AudioTagging over a stub backbone that returns a given embedding, the four poolings, fp32 and fp64:
  frame_sim, clip_sim, the three losses and the gradients of ClipMaskedFrameBceLoss(0.7) w.r.t. the embedding,
  fc_output.weight and fc_output.bias.  Asserts that the restatement tests/tagging_ref.py equals the reference to 1e-13
  in fp64 before anything is written.
* model level: key lists and shapes of AudioTagging(Cnn8Rnn(32000), 527) and AudioTagging(CrnnEncoder(32000, 256), 300),
  and an eval forward of each at B = 2 x 1.5 s with weights drawn by seed (tests/tagging_ref.py; checksums of the
  weights and inputs are stored, no weight tensors).
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
from tests import tagging_ref as R  # noqa: E402

ref_import.install()
from models.audio_text_model import AudioTagging  # noqa: E402  (the reference)
from models.audio_encoder import Cnn8Rnn, CrnnEncoder  # noqa: E402
from losses import ClipBceLoss, ClipMaskedFrameBceLoss, MaskedFrameBceLoss  # noqa: E402


class StubBackbone(torch.nn.Module):
    def __init__(self, embedding, length):
        super().__init__()
        self.embed_dim = embedding.shape[-1]
        self.embedding, self.length = embedding, length

    def forward(self, input_dict):
        return {"embedding": self.embedding, "length": self.length}


out = {}
case = R.draw_head_case()
B, T, E, C = R.HEAD_SHAPE
out["head_length"] = case["length"].numpy()
for k in ("embedding", "weight", "bias", "strong_label", "weak_label", "strong_label_mask"):
    out[f"head_{k}_checksum"] = np.array(R.checksum(case[k]))
for pooling in R.POOLINGS:
    for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
        x = case["embedding"].to(dt).clone().requires_grad_(True)
        model = AudioTagging(StubBackbone(x, case["length"]), C, pooling).to(dt)
        with torch.no_grad():
            model.fc_output.weight.copy_(case["weight"].to(dt))
            model.fc_output.bias.copy_(case["bias"].to(dt))
        o = model({})
        batch = {"label": case["weak_label"].to(dt), "weak_label": case["weak_label"].to(dt),
                 "strong_label": case["strong_label"].to(dt), "strong_label_mask": case["strong_label_mask"].to(dt)}
        o.update(batch)
        l_clip = ClipBceLoss()(o)
        l_frame = MaskedFrameBceLoss()(o)
        l_mix = ClipMaskedFrameBceLoss(R.FRAME_WEIGHT)(o)
        l_mix.backward()
        got = {"frame_sim": o["frame_sim"].detach(), "clip_sim": o["clip_sim"].detach(), "loss_clip": l_clip.detach(),
               "loss_frame": l_frame.detach(), "loss_mix": l_mix.detach(), "dembedding": x.grad,
               "dweight": model.fc_output.weight.grad, "dbias": model.fc_output.bias.grad}
        mine = R.head_case_results(case, pooling, dt)
        err = max((got[k] - mine[k]).abs().max().item() for k in got)
        print(f"{pooling:15s} {tag}: restatement vs reference {err:.2e}; clip_sim range "
              f"[{got['clip_sim'].min().item():.3f}, {got['clip_sim'].max().item():.3f}], loss {l_mix.item():.6f}")
        assert err < (2e-6 if dt == torch.float32 else 1e-13)
        for k, v in got.items():
            out[f"head_{pooling}_{k}_{tag}"] = v.numpy()
    worst = max((torch.as_tensor(out[f"head_{pooling}_{k}_f32"]).double() - torch.as_tensor(out[f"head_{pooling}_{k}_f64"]))
                .abs().max().item() / max(torch.as_tensor(out[f"head_{pooling}_{k}_f64"]).abs().max().item(), 1e-30)
                for k in got)
    print(f"{pooling:15s} reference fp32 vs fp64, worst relative: {worst:.2e}")

for kind, make in (("cnn8rnn", lambda: Cnn8Rnn(32000)), ("crnn", lambda: CrnnEncoder(32000, 256))):
    cfg = R.MODELS[kind]
    model = AudioTagging(make(), cfg["classes"]).eval()
    sd = model.state_dict()
    out[f"{kind}_keys"] = np.array(list(sd))
    out[f"{kind}_shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
    st = R.model_state(kind)
    missing = model.load_state_dict(st, strict=False)
    assert not missing.unexpected_keys and not missing.missing_keys, missing
    batch = R.model_batch(kind)
    with torch.no_grad():
        o = model({"waveform": batch["waveform"], "waveform_len": torch.as_tensor(batch["waveform_len"]), "specaug": False})
        s64 = {k: (v.double() if v.is_floating_point() else v) for k, v in st.items()}
        ao = R.encoder_forward(kind, s64, batch["waveform"].double(), batch["waveform_len"])
        fo, co = R.head(ao["embedding"], s64["fc_output.weight"], s64["fc_output.bias"], ao["length"], "linear_softmax")
    e = max((o["frame_sim"].double() - fo).abs().max().item(), (o["clip_sim"].double() - co).abs().max().item())
    print(f"{kind}: frame_sim {tuple(o['frame_sim'].shape)}, length {torch.as_tensor(o['length']).tolist()}, clip range "
          f"[{o['clip_sim'].min().item():.3f}, {o['clip_sim'].max().item():.3f}]; reference fp32 vs fp64 oracle {e:.2e}")
    assert e < 1e-4 and torch.equal(torch.as_tensor(o["length"]).long(), torch.as_tensor(ao["length"]).long())
    out[f"{kind}_frame_sim"] = o["frame_sim"].numpy()
    out[f"{kind}_clip_sim"] = o["clip_sim"].numpy()
    out[f"{kind}_length"] = torch.as_tensor(o["length"]).long().numpy()
    out[f"{kind}_state_checksum"] = R.state_checksum(st)
    out[f"{kind}_waveform_checksum"] = np.array(R.checksum(batch["waveform"]))

path = os.path.join(HERE, "audio_tagging.npz")
np.savez_compressed(path, **out)
print(f"wrote audio_tagging.npz ({os.path.getsize(path)} bytes)")
