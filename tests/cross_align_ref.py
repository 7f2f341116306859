"""Plain torch statement of the tail of AudioTextCrossAlignByPhrase (models/audio_text_model.py:1033-1063 in the reference):
audio_emb, token_emb, the lengths and the eight cross-encoder parameters -> sim_matrix (B,B,T,N), in the dtype of its inputs
(fp64 on the CPU = the truth of the tests; fp32 = the yardstick of their tolerance).  Gradients come from autograd.
tests/test_cross_align_cpu.py pins it to the imported reference (tests/golden/cross_align.npz).

``project_first`` chooses the association of the gate's pre-activation z: False = fc_s(attn @ tok) as the reference writes it,
True = attn @ (tok Ws^T) + b_s, the tokens projected once (what csrc/cross_pairs.hip computes).  The two are equal because every
softmax row sums to 1; both are legitimate fp32 evaluations."""
import math

import torch
import torch.nn.functional as F

PARAMS = ("attn.h2attn.weight", "attn.h2attn.bias", "attn.v", "gating.fc_u.weight", "gating.fc_u.bias", "gating.fc_s.weight",
          "gating.fc_s.bias")


def head(u, s, kind="dot", l2norm=False, scale=True):
    """match.DotProduct / match.ExpNegL2 with text_level='token' (models/match.py:16-33, 43-60): one text vector per frame."""
    if l2norm:
        u, s = F.normalize(u, dim=-1), F.normalize(s, dim=-1)
    if kind == "expnegl2":
        return torch.exp(-torch.norm(u - s, dim=-1))
    score = (u * s).sum(-1)
    if scale:
        score = score / math.sqrt(u.size(-1))
    return torch.sigmoid(score).clamp(1e-7, 1.0)


def sim_matrix(audio, tokens, alen, wlen, pnum, prm, scale=True, project_first=False, kind="dot", l2norm=False):
    """audio (B,T,D), tokens (P,L,D), alen (B), wlen (P), pnum (B) with sum P, prm = the seven tensors of PARAMS in order ->
    (B,B,T,N), N = max(pnum): [i,j,t,n] = clip i, frame t against phrase n of clip j; zero where n >= pnum[j].  One clip at a
    time against all P phrases, as the reference loops."""
    w_h, b_h, v, w_u, b_u, w_s, b_s = prm
    B, T, D = audio.shape
    P, L = tokens.shape[:2]
    pnum = [int(n) for n in pnum]
    N = max(pnum)
    alen, wlen = torch.as_tensor(alen), torch.as_tensor(wlen)
    ak = F.linear(tokens, w_h[:, D:], b_h)                                            # (P,L,D)
    km = torch.arange(L)[None, :] < wlen.view(-1, 1)                                  # (P,L)
    tok_s = F.linear(tokens, w_s) if project_first else None
    rows = []
    for i in range(B):
        a = audio[i]                                                                  # (T,D)
        aq = F.linear(a, w_h[:, :D])
        score = (torch.tanh(aq[None, :, None, :] + ak[:, None, :, :]) * v).sum(-1)    # (P,T,L)
        qm = torch.arange(T) < alen[i]
        score = score.masked_fill(~qm[None, :, None], -1e10).masked_fill(~km[:, None, :], -1e10)
        attn = torch.softmax(score, dim=-1)
        c = torch.bmm(attn, tokens)                                                   # (P,T,D)
        z = torch.bmm(attn, tok_s) + b_s if project_first else F.linear(c, w_s, b_s)
        g_u = torch.sigmoid(F.linear(a, w_u, b_u))
        sim_i = head(a[None] * torch.sigmoid(z), c * g_u[None], kind, l2norm, scale)  # (P,T)
        blocks = [F.pad(s.transpose(0, 1), (0, N - s.shape[0])) for s in torch.split(sim_i, pnum, dim=0)]
        rows.append(torch.stack(blocks))
    return torch.stack(rows)


def leaves(tensors, dtype):
    return [t.detach().to(dtype).clone().requires_grad_(True) for t in tensors]


def grads(audio, tokens, alen, wlen, pnum, prm, dout, dtype=torch.float64, **kw):
    """sim_matrix and the gradients of (sim_matrix * dout).sum() with respect to audio, tokens and the seven parameters, in
    ``dtype`` on the CPU: (sim_matrix, [d audio, d tokens, d prm...])."""
    lv = leaves([audio, tokens, *prm], dtype)
    out = sim_matrix(lv[0], lv[1], alen, wlen, pnum, lv[2:], **kw)
    g = torch.autograd.grad((out * dout.to(dtype)).sum(), lv, allow_unused=True)
    return out.detach(), [torch.zeros_like(x) if gi is None else gi for x, gi in zip(lv, g)]
