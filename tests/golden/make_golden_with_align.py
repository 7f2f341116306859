#!/usr/bin/env python3
"""tests/golden/with_align.npz:
(a) the REFERENCE's models.align.ExpNegL2 (models/align.py:34-64) in fp32 at B,T,N,D = 3,5,4,32 with one text row that copies an
    audio frame and one that is twice an audio frame (both score exactly 1.0, finite gradients -- asserted here), beside the
    fp64 twin tests/align_ref.exp_neg_l2 with its gradients for an upstream randn;
(b) the REFERENCE's MultiTextBiEncoderWithAlign (models/audio_text_model.py:232-402) in train() mode on stub encoders that return
    stored arrays, match.DotProduct + ExpNegL2 + AudioMeanTextMean, with MultipleLossSum(ClipBceLoss, MaxMarginRankingLoss(0.1,
    sim_key="sentence_sim")) and the gradients with respect to the audio embedding and the text table, in fp32, beside the fp64 twin
    tests/align_ref.with_align_tail.
Only arrays are stored."""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import ref_import  # noqa: E402
from tests import align_ref as R  # noqa: E402

ref_import.install()
from models.align import ExpNegL2  # noqa: E402  (the reference)
from models.match import DotProduct  # noqa: E402
from models.sim_pooling import AudioMeanTextMean  # noqa: E402
from models.audio_text_model import MultiTextBiEncoderWithAlign  # noqa: E402
from losses import ClipBceLoss, MaxMarginRankingLoss, MultipleLossSum  # noqa: E402

out = {}

# ---------------------------------------------------------------------------------------------------------------- (a)
B, T, N, D = 3, 5, 4, 32
g = torch.Generator().manual_seed(41)
audio = torch.randn(B, T, D, generator=g)
text = torch.randn(B, N, D, generator=g)
text[1, 2] = audio[0, 3]                # a copy of a frame
text[2, 0] = 2.0 * audio[1, 1]          # twice a frame
dout = torch.randn(B, B, T, N, generator=g)
a32, t32 = audio.clone().requires_grad_(True), text.clone().requires_grad_(True)
ref = ExpNegL2()(a32, t32)
assert ref.dtype == torch.float32 and ref.shape == (B, B, T, N)
assert ref[0, 1, 3, 2].item() == 1.0 and ref[1, 2, 1, 0].item() == 1.0
(ref * dout).sum().backward()
assert torch.isfinite(a32.grad).all() and torch.isfinite(t32.grad).all()
a_tw, t_tw = audio.clone().requires_grad_(True), text.clone().requires_grad_(True)
tw32 = R.exp_neg_l2(a_tw, t_tw)
(tw32 * dout).sum().backward()
err = max((tw32 - ref).abs().max().item(), (a_tw.grad - a32.grad).abs().max().item(), (t_tw.grad - t32.grad).abs().max().item())
print(f"(a) twin(fp32) vs reference: {err:.2e}")
assert err < 1e-6
a64, t64 = audio.double().requires_grad_(True), text.double().requires_grad_(True)
tw64 = R.exp_neg_l2(a64, t64)
(tw64 * dout.double()).sum().backward()
out.update(a_audio=audio.numpy(), a_text=text.numpy(), a_dout=dout.numpy(), a_out_ref32=ref.detach().numpy(),
           a_daudio_ref32=a32.grad.numpy(), a_dtext_ref32=t32.grad.numpy(), a_out_f64=tw64.detach().numpy(),
           a_daudio_f64=a64.grad.numpy(), a_dtext_f64=t64.grad.numpy())

# ---------------------------------------------------------------------------------------------------------------- (b)
Bm, Tm, Nm, Dm, V = 3, 7, 4, 32, 11
emb = 0.5 * torch.randn(Bm, Tm, Dm, generator=g)
table = 0.5 * torch.randn(V, Dm, generator=g)
length = torch.tensor([7, 4, 6])
text_ids = torch.randint(0, V, (Bm, Nm, 1), generator=g)
text_len = torch.ones(Bm, Nm, dtype=torch.long)
label = torch.tensor([[1.0, 1, 0, 0], [1, 0, 0, 0], [1, 1, 1, 0]])


class AudioStub(nn.Module):
    embed_dim, downsample_ratio = Dm, 1

    def __init__(self, e):
        super().__init__()
        self.e = nn.Parameter(e.clone())

    def forward(self, d):
        return {"embedding": self.e, "length": length}


class TextStub(nn.Module):
    embed_dim = Dm

    def __init__(self, t):
        super().__init__()
        self.table = nn.Parameter(t.clone())

    def forward(self, d):
        return {"seq_emb": self.table[d["text"][:, 0]]}


model = MultiTextBiEncoderWithAlign(AudioStub(emb), TextStub(table), DotProduct(), ExpNegL2(), AudioMeanTextMean(), Dm, ["text"]).train()
loss_fn = MultipleLossSum(["clip", "sentence"], [1, 1], clip=ClipBceLoss(),
                          sentence=MaxMarginRankingLoss(margin=0.1, sim_key="sentence_sim"))
o = model({"text": text_ids, "text_len": text_len, "label": label, "output_matrix": True})
o["label"] = label
loss = loss_fn(o)
loss.backward()
assert o["sim_matrix"].shape == (Bm, Bm, Tm, 3)
e64, tb64 = emb.double().requires_grad_(True), table.double().requires_grad_(True)
tw = R.with_align_tail(e64, tb64[text_ids.reshape(-1)], length, label.double(), Nm)
l64 = R.clip_plus_sentence_loss(tw, label.double(), 0.1)
l64.backward()
errs = {k: (tw[k].detach().float() - o[k].detach()).abs().max().item() for k in ("frame_sim", "clip_sim", "sentence_sim", "sim_matrix")}
errs.update(loss=abs(l64.item() - loss.item()), demb=(e64.grad.float() - model.audio_encoder.e.grad).abs().max().item(),
            dtable=(tb64.grad.float() - model.text_encoder.table.grad).abs().max().item())
print("(b) twin(fp64) vs reference(fp32):", {k: f"{v:.1e}" for k, v in errs.items()}, f"loss {loss.item():.6f}")
assert max(errs.values()) < 1e-6
out.update(b_emb=emb.numpy(), b_table=table.numpy(), b_length=length.numpy(), b_text=text_ids.numpy(), b_text_len=text_len.numpy(),
           b_label=label.numpy(), b_loss_ref32=np.float32(loss.item()), b_loss_f64=np.float64(l64.item()),
           b_demb_ref32=model.audio_encoder.e.grad.numpy(), b_dtable_ref32=model.text_encoder.table.grad.numpy(),
           b_demb_f64=e64.grad.numpy(), b_dtable_f64=tb64.grad.numpy())
for k in ("frame_sim", "clip_sim", "sentence_sim", "sim_matrix"):
    out[f"b_{k}_ref32"] = o[k].detach().numpy()
    out[f"b_{k}_f64"] = tw[k].detach().numpy()
np.savez_compressed(os.path.join(HERE, "with_align.npz"), **out)
print("wrote with_align.npz")
