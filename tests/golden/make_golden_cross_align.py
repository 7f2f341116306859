#!/usr/bin/env python3
"""tests/golden/cross_align.npz: the REFERENCE's AudioTextCrossAlignByPhrase (models/audio_text_model.py:979-1073) in fp32 with its
CrossAttentionGating, match.DotProduct(text_level="token"), AudioMeanTextMean and MaxMarginRankingLoss(0.1) on stub encoders that
return stored arrays -- B = 3 clips, T = 6 frames with lengths [6, 4, 6], [2, 1, 3] phrases of L = 4 tokens (1 to 4 valid), D = 32
-- with sim_matrix, sim, the loss and its gradients with respect to the audio embedding, the token embeddings and the seven
cross-encoder parameters, beside the fp64 twin tests/cross_align_ref.sim_matrix + the oracle's pooling and loss.
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
from oracle import tag_oracle as O  # noqa: E402
from tests import cross_align_ref as R  # noqa: E402

ref_import.install()
from models.audio_text_model import AudioTextCrossAlignByPhrase  # noqa: E402  (the reference)
from models.cross_encoder import CrossAttentionGating  # noqa: E402
from models.match import DotProduct  # noqa: E402
from models.sim_pooling import AudioMeanTextMean  # noqa: E402
from losses import MaxMarginRankingLoss  # noqa: E402

B, T, L, D = 3, 6, 4, 32
length = torch.tensor([6, 4, 6])
pnum = [2, 1, 3]
P = sum(pnum)
g = torch.Generator().manual_seed(53)
emb = 0.8 * torch.randn(B, T, D, generator=g)
tok = 0.8 * torch.randn(P, L, D, generator=g)
tok_len = torch.tensor([4, 1, 3, 2, 4, 1])
for p in range(P):
    tok[p, tok_len[p]:] = 0.0                         # what EmbeddingLayer leaves at the padding id
MARGIN = 0.1


class AudioStub(nn.Module):
    embed_dim, downsample_ratio = D, 1

    def __init__(self, e):
        super().__init__()
        self.e = nn.Parameter(e.clone())

    def forward(self, d):
        return {"embedding": self.e, "length": length}


class TextStub(nn.Module):
    embed_dim = D

    def __init__(self, t):
        super().__init__()
        self.t = nn.Parameter(t.clone())

    def forward(self, d):
        return {"token_emb": self.t, "seq_emb": self.t.sum(1) / d["text_len"].view(-1, 1)}


torch.manual_seed(7)
cross = CrossAttentionGating(D)
with torch.no_grad():
    cross.attn.v.mul_(0.7)
model = AudioTextCrossAlignByPhrase(AudioStub(emb), TextStub(tok), DotProduct(text_level="token"), AudioMeanTextMean(), D, False,
                                    cross_encoder=cross).train()
o = model({"text_key": "phrases", "phrases": torch.zeros(P, L, dtype=torch.long), "phrases_len": tok_len, "phrases_num": pnum})
loss = MaxMarginRankingLoss(margin=MARGIN)(o)
loss.backward()
assert o["sim_matrix"].shape == (B, B, T, max(pnum)) and o["sim"].shape == (B, B) and o["sim_matrix"].dtype == torch.float32
prm = [dict(cross.named_parameters())[k] for k in R.PARAMS]
ref_grads = [model.audio_encoder.e.grad, model.text_encoder.t.grad] + [p.grad for p in prm]


def twin(dtype, project_first):
    lv = R.leaves([emb, tok, *prm], dtype)
    m = R.sim_matrix(lv[0], lv[1], length, tok_len, pnum, lv[2:], project_first=project_first)
    sim = O.audio_mean_text_mean(m, length, torch.as_tensor(pnum))
    ls = O.max_margin_ranking_loss(sim, MARGIN, 1.0)
    return m.detach(), sim.detach(), ls.detach(), torch.autograd.grad(ls, lv)


for pf in (False, True):
    m, sim, ls, gr = twin(torch.float32, pf)
    errs = dict(sim_matrix=(m - o["sim_matrix"]).abs().max().item(), sim=(sim - o["sim"]).abs().max().item(),
                loss=abs(ls.item() - loss.item()), grads=max((a - b).abs().max().item() for a, b in zip(gr, ref_grads)))
    print(f"twin(fp32, project_first={pf}) vs reference:", {k: f"{v:.1e}" for k, v in errs.items()}, f"loss {loss.item():.6f}")
    assert max(errs.values()) < 1e-6
m64, sim64, l64, g64 = twin(torch.float64, False)
assert l64.item() > 0 and all(gi.abs().max().item() > 0 for gi in g64)

out = dict(emb=emb.numpy(), tok=tok.numpy(), length=length.numpy(), tok_len=tok_len.numpy(), pnum=np.asarray(pnum),
           margin=np.float64(MARGIN), sim_matrix_ref32=o["sim_matrix"].detach().numpy(), sim_ref32=o["sim"].detach().numpy(),
           loss_ref32=np.float32(loss.item()), sim_matrix_f64=m64.numpy(), sim_f64=sim64.numpy(), loss_f64=np.float64(l64.item()))
names = ["emb", "tok"] + [k.replace(".", "_") for k in R.PARAMS]
for k, p in zip(R.PARAMS, prm):
    out["p_" + k.replace(".", "_")] = p.detach().numpy()
for k, gr, g6 in zip(names, ref_grads, g64):
    out[f"d_{k}_ref32"] = gr.numpy()
    out[f"d_{k}_f64"] = g6.numpy()
np.savez_compressed(os.path.join(HERE, "cross_align.npz"), **out)
print("wrote cross_align.npz")
