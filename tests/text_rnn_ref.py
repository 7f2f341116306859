"""Plain-torch restatement of the reference's RnnEncoder (models/text_encoder.py:91-125: EmbeddingLayer -> nn.GRU over the
padded batch -> mean_with_lens) and of one row-local recurrence launch (csrc/text_gru.hip), any dtype.  Used by the CPU and the
GPU tests; tests/golden/make_golden_text_rnn.py asserts that it equals the imported reference to 1e-12 in fp64 before the
fixture tests/golden/text_rnn.npz is written.  Nothing here touches the HIP library."""
import math

import numpy as np
import torch
import torch.nn as nn

# (V, E, H, layers, dirs, R, L): one full 16-row tile + a tail row; H = 8 / 20 (16-byte rows of W_hh, one / two unit tiles with
# a tail) and H = 10 (unaligned rows); lengths include 1 and L
CONFIGS = {
    "l2_bi": dict(V=50, E=16, H=8, layers=2, dirs=2, R=17, L=7, seed=7101),
    "l1_bi": dict(V=50, E=16, H=20, layers=1, dirs=2, R=17, L=7, seed=7102),
    "l2_uni": dict(V=50, E=16, H=10, layers=2, dirs=1, R=17, L=7, seed=7103),
}
# the whole-model case: BiEncoder(CrnnEncoder(32000, 256), RnnEncoder(200, 32, 128, 1, 0, True, "GRU"), DotProduct()), eval
MODEL = dict(V=200, E=32, H=128, layers=1, dirs=2, crnn_seed=61, text_seed=63, batch_seed=65, samples=48000)


def param_names(layers, dirs):
    names = ["embedding.core.weight"]
    for l in range(layers):
        for sfx in ("", "_reverse")[:dirs]:
            names += [f"rnn.{k}_l{l}{sfx}" for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    return names


def draw_params(V, E, H, layers, dirs, seed):
    """fp32 state dict with nn.GRU's default scale (uniform +-1/sqrt(H)); numpy's generator: stable across torch versions."""
    rs = np.random.RandomState(seed)
    k = 1.0 / math.sqrt(H)
    st = {"embedding.core.weight": torch.from_numpy(rs.standard_normal((V, E)).astype(np.float32))}
    for l in range(layers):
        I = E if l == 0 else dirs * H
        for sfx in ("", "_reverse")[:dirs]:
            for name, shape in (("weight_ih", (3 * H, I)), ("weight_hh", (3 * H, H)), ("bias_ih", (3 * H,)), ("bias_hh", (3 * H,))):
                st[f"rnn.{name}_l{l}{sfx}"] = torch.from_numpy(rs.uniform(-k, k, shape).astype(np.float32))
    return st


def draw_inputs(cfg):
    """Token ids (pad id 0 behind text_len) and lengths; the first two rows have length 1 and L."""
    rs = np.random.RandomState(cfg["seed"] + 1)
    R, L, V = cfg["R"], cfg["L"], cfg["V"]
    lens = rs.randint(1, L + 1, R)
    lens[0], lens[1] = 1, L
    text = rs.randint(2, V, (R, L))
    for i in range(R):
        text[i, lens[i]:] = 0
    return torch.from_numpy(text).long(), torch.from_numpy(lens).long()


def objective_weights(cfg, dtype=torch.float64):
    """The fixed random linear objective  sum(token_emb * Wt) + sum(seq_emb * Ws)."""
    rs = np.random.RandomState(cfg["seed"] + 2)
    D = cfg["H"] * cfg["dirs"]
    return (torch.from_numpy(rs.standard_normal((cfg["R"], cfg["L"], D))).to(dtype),
            torch.from_numpy(rs.standard_normal((cfg["R"], D))).to(dtype))


def masked_mean(token_emb, text_len):
    L = token_emb.shape[1]
    mask = (torch.arange(L, device=token_emb.device)[None, :] < text_len.to(token_emb.device)[:, None]).to(token_emb.dtype)
    return (token_emb * mask[..., None]).sum(1) / text_len.to(token_emb.device, token_emb.dtype)[:, None]


def encoder_forward(st, text, text_len, layers, dirs, masks=None, p=0.0):
    """st: state dict (any dtype, tensors may require grad).  masks: per layer but the last a 0/1 keep mask (R, L, dirs*H) applied
    as x * mask / (1 - p) -- nn.GRU's inter-layer dropout with the mask passed in.  -> token_emb, seq_emb."""
    table = st["embedding.core.weight"]
    x = table[text.long().to(table.device)]
    H = st["rnn.weight_hh_l0"].shape[1]
    for l in range(layers):
        gru = nn.GRU(x.shape[-1], H, 1, batch_first=True, bidirectional=dirs == 2).to(device=table.device, dtype=table.dtype)
        named = {f"{k}_l0{sfx}": st[f"rnn.{k}_l{l}{sfx}"] for sfx in ("", "_reverse")[:dirs]
                 for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")}
        x, _ = torch.func.functional_call(gru, named, (x,))
        if masks is not None and l + 1 < layers:
            x = x * masks[l].to(x.dtype) / (1.0 - p)
    return x, masked_mean(x, text_len)


def objective(token_emb, seq_emb, wt, ws):
    return (token_emb * wt.to(token_emb.device, token_emb.dtype)).sum() + (seq_emb * ws.to(seq_emb.device, seq_emb.dtype)).sum()


def config_results(cfg, st, text, text_len, dtype, masks=None, p=0.0):
    """token_emb, seq_emb and every parameter gradient of the fixed objective, in ``dtype`` on the CPU."""
    s = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in st.items()}
    tok, seq = encoder_forward(s, text, text_len, cfg["layers"], cfg["dirs"], masks, p)
    wt, ws = objective_weights(cfg, dtype)
    objective(tok, seq, wt, ws).backward()
    out = {"token_emb": tok.detach(), "seq_emb": seq.detach()}
    out.update({"d" + k: v.grad for k, v in s.items()})
    return out


# ---- one recurrence launch: what tag_text_gru_forward / tag_text_gru_backward compute ----
def recurrence(gi, w_hh, b_hh, text_len=None, keep_gh=False):
    """gi (R, L, dirs, 3H), w_hh (dirs, 3H, H), b_hh (dirs, 3H) -> y (R, L, dirs*H), gates (R, L, dirs, 4H) [r, z, n, gh_n],
    seq_mean (R, dirs*H) or None, hprev (R, L, dirs, H), and with keep_gh the per-step gh tensors [(d, t, gh)] (retain_grad)."""
    R, L, dirs, H3 = gi.shape
    H = H3 // 3
    ys = [[None] * L for _ in range(dirs)]
    gs = [[None] * L for _ in range(dirs)]
    hps = [[None] * L for _ in range(dirs)]
    ghs = []
    for d in range(dirs):
        h = gi.new_zeros(R, H)
        for s in range(L):
            t = s if d == 0 else L - 1 - s
            gh = h @ w_hh[d].t() + b_hh[d]
            if keep_gh:
                if not gh.requires_grad:                  # first step: h0 = 0 and constant weights, nothing upstream records
                    gh = gh.detach().requires_grad_(True)
                gh.retain_grad()
                ghs.append((d, t, gh))
            x = gi[:, t, d]
            r = torch.sigmoid(x[:, :H] + gh[:, :H])
            z = torch.sigmoid(x[:, H:2 * H] + gh[:, H:2 * H])
            n = torch.tanh(x[:, 2 * H:] + r * gh[:, 2 * H:])
            hps[d][t] = h
            h = (1.0 - z) * n + z * h
            ys[d][t] = h
            gs[d][t] = torch.cat([r, z, n, gh[:, 2 * H:]], 1)
    y = torch.stack([torch.cat([ys[d][t] for d in range(dirs)], 1) for t in range(L)], 1)
    gates = torch.stack([torch.stack([gs[d][t] for d in range(dirs)], 1) for t in range(L)], 1)
    hprev = torch.stack([torch.stack([hps[d][t] for d in range(dirs)], 1) for t in range(L)], 1)
    seq = masked_mean(y, text_len) if text_len is not None else None
    return y, gates, seq, hprev, ghs


def recurrence_backward(dy, dseq, text_len, y, gates, w_hh):
    """The backward launch restated step by step -> dgi, dgh (R, L, dirs, 3H), hprev (R, L, dirs, H)."""
    R, L, dirs, H4 = gates.shape
    H = H4 // 4
    dgi = gates.new_zeros(R, L, dirs, 3 * H)
    dgh = gates.new_zeros(R, L, dirs, 3 * H)
    hprev = gates.new_zeros(R, L, dirs, H)
    yv = y.view(R, L, dirs, H)
    for d in range(dirs):
        carry = gates.new_zeros(R, H)
        for s in range(L):
            t = L - 1 - s if d == 0 else s
            tp = t - 1 if d == 0 else t + 1
            r, z, n, ghn = gates[:, t, d].split(H, 1)
            dh = carry.clone()
            if dy is not None:
                dh = dh + dy.view(R, L, dirs, H)[:, t, d]
            if dseq is not None:
                valid = (t < text_len).to(dh.dtype)[:, None]
                dh = dh + valid * dseq.view(R, dirs, H)[:, d] / text_len.to(dh.dtype)[:, None]
            hp = yv[:, tp, d] if s + 1 < L else torch.zeros_like(dh)
            dn_pre = dh * (1.0 - z) * (1.0 - n * n)
            dz_pre = dh * (hp - n) * z * (1.0 - z)
            dr_pre = dn_pre * ghn * r * (1.0 - r)
            dgi[:, t, d] = torch.cat([dr_pre, dz_pre, dn_pre], 1)
            dgh[:, t, d] = torch.cat([dr_pre, dz_pre, dn_pre * r], 1)
            hprev[:, t, d] = hp
            carry = dh * z + dgh[:, t, d] @ w_hh[d]
    return dgi, dgh, hprev


# ---- whole-model case ----
def model_text_state():
    m = MODEL
    return draw_params(m["V"], m["E"], m["H"], m["layers"], m["dirs"], m["text_seed"])


def model_state():
    """fp32 state dict of the whole-model case keyed like BiEncoder's: the oracle's seeded CrnnEncoder + the seeded text encoder."""
    from oracle import tag_oracle as O
    st = dict(O.init_crnn_state(seed=MODEL["crnn_seed"], embed_dim=256))
    st.update({"text_encoder." + k: v for k, v in model_text_state().items()})
    return st


def model_batch():
    from oracle import tag_oracle as O
    return O.synthetic_batch(2, MODEL["samples"], seed=MODEL["batch_seed"], ragged=True, hop=640, vocab_size=MODEL["V"])


def checksum(t):
    t = torch.as_tensor(t).detach().double().flatten()
    return [float(t.sum()), float(t.abs().max()), float(t[:: max(1, t.numel() // 7)][:7].sum())]


def state_checksum(st):
    return np.array([c for k in sorted(st) if st[k].is_floating_point() for c in checksum(st[k])])


def rel_err(got, ref):
    """Largest deviation relative to the largest entry of the reference tensor (the measure of the fixture's recorded figures)."""
    ref = torch.as_tensor(ref).detach().cpu().double()
    return (torch.as_tensor(got).detach().cpu().double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-300)
