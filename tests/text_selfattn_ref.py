"""Plain-torch restatement of the reference's SelfAttention text encoder (models/text_encoder.py:240-268: EmbeddingLayer -> cls
token in front -> + sinusoidal positions -> dropout -> nn.MultiheadAttention with a key-padding mask) and of the attention core
alone (csrc/text_attn.hip), any dtype.  Unlike the reference it is defined for EVERY text_len in [0, L]: the key mask is built
L + 1 wide.  Dropout masks are optional arguments (0/1 keep masks, applied as x * mask / (1 - p)).  Used by the CPU and the GPU
tests; tests/golden/make_golden_text_selfattn.py asserts that it equals the imported reference to 1e-12 in fp64 before the
fixture tests/golden/text_selfattn.npz is written.  Nothing here touches the HIP library."""
import math

import numpy as np
import torch

# (V, E, heads, R, L): head_dim 16 / 16 / 64, several heads and one; lengths include 1 and L
CONFIGS = {
    "e64_h4": dict(V=200, E=64, heads=4, R=48, L=9, seed=8101),
    "e32_h2": dict(V=200, E=32, heads=2, R=16, L=12, seed=8102),
    "e64_h1": dict(V=120, E=64, heads=1, R=8, L=5, seed=8103),
}
# the whole-model case: BiEncoder(CrnnEncoder(32000, 256), SelfAttention(200, 256, 4, 0.0), DotProduct(), 256), eval
MODEL = dict(V=200, E=256, heads=4, crnn_seed=71, text_seed=73, batch_seed=75, samples=48000)

PARAM_NAMES = ["cls_token", "embedding.core.weight", "mha.in_proj_weight", "mha.in_proj_bias", "mha.out_proj.weight",
               "mha.out_proj.bias"]
STATE_NAMES = ["cls_token", "embedding.core.weight", "pe.pe", "mha.in_proj_weight", "mha.in_proj_bias", "mha.out_proj.weight",
               "mha.out_proj.bias"]


def position_table(E, max_len=100):
    """(1, max_len, E) fp32: sin(pos / 10000^(2i/E)) on channel 2i, cos of the same angle on channel 2i + 1."""
    pos = torch.arange(0, max_len).unsqueeze(1)
    div = torch.exp(torch.arange(0, E, 2) * -(math.log(10000.0) / E))
    pe = torch.zeros(max_len, E)
    pe[:, 0::2] = torch.sin(pos * div)
    pe[:, 1::2] = torch.cos(pos * div)
    return pe.unsqueeze(0)


def draw_params(V, E, heads, seed):
    """fp32 state dict (the pe.pe buffer included); numpy's generator: stable across torch versions.  cls_token is drawn NON-zero
    (the module constructs it as zeros, which would leave its gradient path barely exercised) and so are the biases."""
    rs = np.random.RandomState(seed)
    k = 1.0 / math.sqrt(E)
    f = lambda a: torch.from_numpy(a.astype(np.float32))                              # noqa: E731
    return {
        "cls_token": f(0.5 * rs.standard_normal((1, 1, E))),
        "embedding.core.weight": f(rs.standard_normal((V, E))),
        "pe.pe": position_table(E),
        "mha.in_proj_weight": f(rs.uniform(-2 * k, 2 * k, (3 * E, E))),
        "mha.in_proj_bias": f(rs.uniform(-0.2, 0.2, (3 * E,))),
        "mha.out_proj.weight": f(rs.uniform(-k, k, (E, E))),
        "mha.out_proj.bias": f(rs.uniform(-0.2, 0.2, (E,))),
    }


def draw_inputs(cfg, full=True):
    """Token ids (pad id 0 behind text_len) and lengths; the first two rows have length 1 and L (so max(text_len) == L, which the
    reference needs).  full=False: lengths in [0, L - 1] with a 0 in row 0 -- batches the reference cannot run."""
    rs = np.random.RandomState(cfg["seed"] + 1)
    R, L, V = cfg["R"], cfg["L"], cfg["V"]
    if full:
        lens = rs.randint(1, L + 1, R)
        lens[0], lens[1] = 1, L
    else:
        lens = rs.randint(0, L, R)
        lens[0], lens[1] = 0, L - 1
    text = rs.randint(2, V, (R, L))
    for i in range(R):
        text[i, lens[i]:] = 0
    return torch.from_numpy(text).long(), torch.from_numpy(lens).long()


def objective_weights(cfg, dtype=torch.float64):
    """The fixed random linear objective  sum(token_emb * Wt) + sum(seq_emb * Ws)."""
    rs = np.random.RandomState(cfg["seed"] + 2)
    return (torch.from_numpy(rs.standard_normal((cfg["R"], cfg["L"], cfg["E"]))).to(dtype),
            torch.from_numpy(rs.standard_normal((cfg["R"], cfg["E"]))).to(dtype))


def objective(token_emb, seq_emb, wt, ws):
    return (token_emb * wt.to(token_emb.device, token_emb.dtype)).sum() + (seq_emb * ws.to(seq_emb.device, seq_emb.dtype)).sum()


# ---- the attention core: what tag_text_selfattn_forward / tag_text_selfattn_backward compute ----
def core(qkv, klen, heads, attn_mask=None, p=0.0):
    """qkv (R, S, 3E) packed [q|k|v], klen (R) valid keys -> ctx (R, S, E), attn (R, H, S, S) = the softmax weights BEFORE dropout
    (exactly 0 at keys >= klen).  attn_mask: 0/1 keep mask (R, H, S, S)."""
    R, S, E3 = qkv.shape
    E = E3 // 3
    dh = E // heads
    q, k, v = (t.reshape(R, S, heads, dh).transpose(1, 2) for t in qkv.split(E, dim=2))
    scores = (q @ k.transpose(2, 3)) / math.sqrt(dh)
    dead = torch.arange(S, device=qkv.device)[None, :] >= klen.to(qkv.device)[:, None]
    scores = scores.masked_fill(dead[:, None, None, :], float("-inf"))
    attn = torch.softmax(scores, dim=-1)
    w = attn if attn_mask is None else attn * attn_mask.to(attn.dtype) / (1.0 - p)
    ctx = (w @ v).transpose(1, 2).reshape(R, S, E)
    return ctx, attn


def core_backward(qkv, attn, dctx, klen, heads, attn_mask=None, p=0.0):
    """The backward launch restated as explicit formulas -> dqkv (R, S, 3E).  (klen is implied by the zeros of attn.)"""
    R, S, E3 = qkv.shape
    E = E3 // 3
    dh = E // heads
    q, k, v = (t.reshape(R, S, heads, dh).transpose(1, 2) for t in qkv.split(E, dim=2))
    g = dctx.reshape(R, S, heads, dh).transpose(1, 2)
    keep = 1.0 if attn_mask is None else attn_mask.to(attn.dtype) / (1.0 - p)
    dv = (attn * keep).transpose(2, 3) @ g
    da = (g @ v.transpose(2, 3)) * keep
    ds = attn * (da - (attn * da).sum(-1, keepdim=True)) / math.sqrt(dh)
    dq, dk = ds @ k, ds.transpose(2, 3) @ q
    return torch.cat([t.transpose(1, 2).reshape(R, S, E) for t in (dq, dk, dv)], dim=2)


def core_results(qkv, klen, heads, dctx, dtype, attn_mask=None, p=0.0):
    """ctx, attn and dqkv of sum(ctx * dctx), in ``dtype`` on the CPU through plain autograd."""
    x = qkv.detach().to(dtype).clone().requires_grad_(True)
    ctx, attn = core(x, klen, heads, attn_mask, p)
    (ctx * dctx.to(dtype)).sum().backward()
    return dict(ctx=ctx.detach(), attn=attn.detach(), dqkv=x.grad)


# ---- the encoder ----
def encoder_forward(st, text, text_len, heads, pe_mask=None, attn_mask=None, p=0.0):
    """st: state dict (any dtype, tensors may require grad).  pe_mask (R, L+1, E) / attn_mask (R, H, L+1, L+1): 0/1 keep masks of
    the dropout behind the positions and on the attention weights.  -> token_emb (R, L, E), seq_emb (R, E)."""
    table = st["embedding.core.weight"]
    x = table[text.long().to(table.device)]
    R, L, E = x.shape
    x = torch.cat((st["cls_token"].expand(R, -1, -1), x), dim=1) + st["pe.pe"][:, :L + 1].to(x.dtype)
    if pe_mask is not None:
        x = x * pe_mask.to(x.dtype) / (1.0 - p)
    qkv = x @ st["mha.in_proj_weight"].t() + st["mha.in_proj_bias"]
    ctx, _ = core(qkv, text_len.clamp(0, L) + 1, heads, attn_mask, p)
    out = ctx @ st["mha.out_proj.weight"].t() + st["mha.out_proj.bias"]
    return out[:, 1:], out[:, 0]


def config_results(cfg, st, text, text_len, dtype, pe_mask=None, attn_mask=None, p=0.0):
    """token_emb, seq_emb and every parameter gradient of the fixed objective, in ``dtype`` on the CPU."""
    s = {k: v.detach().to(dtype).clone().requires_grad_(k in PARAM_NAMES) for k, v in st.items()}
    tok, seq = encoder_forward(s, text, text_len, cfg["heads"], pe_mask, attn_mask, p)
    wt, ws = objective_weights(cfg, dtype)
    objective(tok, seq, wt, ws).backward()
    out = {"token_emb": tok.detach(), "seq_emb": seq.detach()}
    out.update({"d" + k: s[k].grad for k in PARAM_NAMES})
    return out


# ---- whole-model case ----
def model_text_state():
    m = MODEL
    return draw_params(m["V"], m["E"], m["heads"], m["text_seed"])


def model_state():
    """fp32 state dict of the whole-model case keyed like BiEncoder's: the oracle's seeded CrnnEncoder + the seeded text encoder."""
    from oracle import tag_oracle as O
    st = dict(O.init_crnn_state(seed=MODEL["crnn_seed"], embed_dim=256))
    st.update({"text_encoder." + k: v for k, v in model_text_state().items()})
    return st


def model_batch():
    """The oracle's ragged batch with the token tensor cut to the longest phrase (the reference needs max(text_len) == L)."""
    from oracle import tag_oracle as O
    b = O.synthetic_batch(2, MODEL["samples"], seed=MODEL["batch_seed"], ragged=True, hop=640, vocab_size=MODEL["V"])
    b["text"] = b["text"][:, :int(np.max(b["text_len"]))].contiguous()
    return b


def checksum(t):
    t = torch.as_tensor(t).detach().double().flatten()
    return [float(t.sum()), float(t.abs().max()), float(t[:: max(1, t.numel() // 7)][:7].sum())]


def state_checksum(st):
    """Checksums of the DRAWN weights.  The position buffer is left out: it is computed, not drawn, and fp32 sin / cos / exp
    differ in the last bit between CPUs (vector math libraries), which a 1e-12 comparison would report as another state."""
    return np.array([c for k in sorted(st) if st[k].is_floating_point() and not k.endswith("pe.pe") for c in checksum(st[k])])


def rel_err(got, ref):
    """Largest deviation relative to the largest entry of the reference tensor (the measure of the fixture's recorded figures)."""
    ref = torch.as_tensor(ref).detach().cpu().double()
    return (torch.as_tensor(got).detach().cpu().double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-300)
