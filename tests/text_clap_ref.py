"""Differentiable restatement of the LAION-CLAP text tower as LaionClapEncoder trains it (models/text_encoder.py:311-327 over
Hugging Face's ClapTextModel + ClapProjectionLayer), any dtype, CPU, with INJECTED dropout masks, plus the restatement of every
row kernel of csrc/text_clap.hip.  TEST INFRASTRUCTURE ONLY.  tests/golden/make_golden_text_clap.py asserts the forward and all
parameter gradients equal the real transformers modules in fp64 to 1e-12."""
import math

import torch
import torch.nn.functional as F

#: the tiny configuration of tests/golden/text_clap.npz (dropouts 0; the tests that want dropout pass masks)
TINY = dict(vocab_size=120, hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=160,
            max_position_embeddings=72, projection_dim=32, layer_norm_eps=1e-12, pad_token_id=1, hidden_dropout_prob=0.0,
            attention_probs_dropout_prob=0.0)
FIXTURE = dict(R=5, L=9, state_seed=21, input_seed=3, objective_seed=8)

HEAD = ("embeddings.word_embeddings.weight", "embeddings.token_type_embeddings.weight", "embeddings.position_embeddings.weight",
        "embeddings.LayerNorm.weight", "embeddings.LayerNorm.bias")
LAYER = ("attention.self.query.weight", "attention.self.query.bias", "attention.self.key.weight", "attention.self.key.bias",
         "attention.self.value.weight", "attention.self.value.bias", "attention.output.dense.weight", "attention.output.dense.bias",
         "attention.output.LayerNorm.weight", "attention.output.LayerNorm.bias", "intermediate.dense.weight",
         "intermediate.dense.bias", "output.dense.weight", "output.dense.bias", "output.LayerNorm.weight", "output.LayerNorm.bias")
TAIL = ("model.pooler.dense.weight", "model.pooler.dense.bias", "projection.linear1.weight", "projection.linear1.bias",
        "projection.linear2.weight", "projection.linear2.bias")


def param_names(layers):
    return ["model." + n for n in HEAD] + [f"model.encoder.layer.{l}.{n}" for l in range(layers) for n in LAYER] + list(TAIL)


def param_shapes(cfg):
    D, I, P = cfg["hidden_size"], cfg["intermediate_size"], cfg["projection_dim"]
    head = [(cfg["vocab_size"], D), (1, D), (cfg["max_position_embeddings"], D), (D,), (D,)]
    layer = [(D, D), (D,)] * 4 + [(D,), (D,), (I, D), (I,), (D, I), (D,), (D,), (D,)]
    tail = [(D, D), (D,), (P, D), (P,), (P, P), (P,)]
    return head + layer * cfg["num_hidden_layers"] + tail


def draw_state(cfg, seed, scale=None):
    """Seeded fp32 parameters by name (no index buffers): N(0, scale^2), scale ~ 1.5 / sqrt(fan_in) for matrices so that every
    stage matters, LayerNorm weights 1 + N(0, 0.1^2), the pad rows of the two padded tables zero as nn.Embedding leaves them."""
    g = torch.Generator().manual_seed(seed)
    st = {}
    for name, shape in zip(param_names(cfg["num_hidden_layers"]), param_shapes(cfg)):
        if "LayerNorm.weight" in name:
            st[name] = 1.0 + 0.1 * torch.randn(*shape, generator=g)
        elif "embeddings" in name and len(shape) == 2:
            st[name] = 0.5 * torch.randn(*shape, generator=g)
        elif len(shape) == 2:
            st[name] = torch.randn(*shape, generator=g) * ((scale or 1.5) / math.sqrt(shape[1]))
        else:
            st[name] = 0.1 * torch.randn(*shape, generator=g)
    for name in ("model.embeddings.word_embeddings.weight", "model.embeddings.position_embeddings.weight"):
        st[name][cfg["pad_token_id"]] = 0.0
    return st


def draw_inputs(R, L, seed, vocab=120, pad_id=1):
    """RoBERTa-style rows <s> ... </s> right-padded with pad_id: row 0 full, row 1 cut down to its first TWO tokens (when R > 1),
    the others of length 2 ... L; ids drawn from a few values so that they repeat within and across rows."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((R, L), pad_id, dtype=torch.long)
    mask = torch.zeros(R, L, dtype=torch.long)
    pool = torch.randint(3, vocab, (max(4, (R * L) // 3),), generator=g)
    for r in range(R):
        n = L if r == 0 else (2 if r == 1 else int(torch.randint(2, L + 1, (1,), generator=g)))
        ids[r, 0] = 0
        if n > 2:
            ids[r, 1:n - 1] = pool[torch.randint(0, len(pool), (n - 2,), generator=g)]
        ids[r, n - 1] = 2
        mask[r, :n] = 1
    return ids, mask


def position_ids(ids, pad_id=1):
    m = ids.ne(pad_id).long()
    return torch.cumsum(m, dim=1) * m + pad_id


def rel_err(a, b, scale=None):
    a, b = torch.as_tensor(a).detach().double(), torch.as_tensor(b).detach().double()
    s = b.abs().max() if scale is None else torch.as_tensor(scale).double().abs().max()
    return float((a - b).abs().max() / s.clamp_min(1e-300))


def quantity_err(got, ref, k):
    """Error of quantity k relative to the largest entry of the reference tensor.  The key bias shifts every score of a query row
    by the same amount, so its gradient is ZERO up to rounding (1e-17 in fp64): it is measured against the scale of the query
    bias's gradient, which has the same units."""
    return rel_err(got[k], ref[k], ref[k.replace("key.bias", "query.bias")])


# ---------------------------------------------------------------------------------------------- the row kernels, restated
def ln_forward(x, res, gamma, beta, eps):
    """-> y, xhat, rstd of LayerNorm(x + res) over the last dimension (biased variance, as nn.LayerNorm)."""
    s = x if res is None else x + res
    mean = s.mean(-1, keepdim=True)
    var = ((s - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (s - mean) * rstd
    return xhat * gamma + beta, xhat, rstd.squeeze(-1)


def ln_backward(dy, xhat, rstd, gamma):
    g = dy * gamma
    ds = rstd.unsqueeze(-1) * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True))
    return ds, (dy * xhat).sum(0), dy.sum(0)


def gelu(u):
    return 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0)))


def gelu_backward(u, df):
    cdf = 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)
    return df * (cdf + u * pdf)


def tanh_backward(y, dy):
    return dy * (1.0 - y * y)


def embed_forward(ids, word, type0, pos, gamma, beta, eps, pad_id):
    """-> h (B*L, D), position ids (B*L), xhat, rstd."""
    p = position_ids(ids, pad_id)
    s = word[ids] + type0.reshape(-1) + pos[p]
    y, xhat, rstd = ln_forward(s.reshape(-1, s.shape[-1]), None, gamma, beta, eps)
    return y, p.reshape(-1), xhat, rstd


def embed_backward(dh, xhat, rstd, gamma, ids, pos_ids, V, P, pad_id):
    """-> dword (V, D), dtype0 (1, D), dpos (P, D), dgamma, dbeta; the pad rows of the two tables exactly zero."""
    ds, dg, db = ln_backward(dh, xhat, rstd, gamma)
    D = dh.shape[-1]
    keep = ids.reshape(-1).ne(pad_id).to(ds.dtype).unsqueeze(-1)
    dword = torch.zeros(V, D, dtype=ds.dtype).index_add_(0, ids.reshape(-1), ds * keep)
    dpos = torch.zeros(P, D, dtype=ds.dtype).index_add_(0, pos_ids.reshape(-1), ds * keep)
    return dword, ds.sum(0, keepdim=True), dpos, dg, db


# ---------------------------------------------------------------------------------------------- the whole tower
def _drop(x, mask, p):
    return x if mask is None else x * mask.to(x.dtype).reshape(x.shape) / (1.0 - p)


def forward(st, ids, mask, heads, eps=1e-12, pad_id=1, masks=None, p_hidden=0.0, p_attn=0.0):
    """st: parameters by state-dict name (any dtype).  masks: {"emb": (R*L, D), ("attn", l): (R, H, L, L), ("ao", l): (R*L, D),
    ("out", l): (R*L, D)} keep masks or None.  Keys >= klen = max(mask.sum(-1), 1) are masked.  -> token_emb (R, L, P), seq_emb."""
    masks = masks or {}
    g = lambda k: st["model." + k]                           # noqa: E731
    R, L = ids.shape
    pos = position_ids(ids, pad_id)
    # both tables are nn.Embedding(padding_idx = pad_token_id): the pad row is looked up like any other but receives NO gradient
    h = F.embedding(ids, g("embeddings.word_embeddings.weight"), padding_idx=pad_id) \
        + g("embeddings.token_type_embeddings.weight")[0] \
        + F.embedding(pos, g("embeddings.position_embeddings.weight"), padding_idx=pad_id)
    D = h.shape[-1]
    h = F.layer_norm(h, (D,), g("embeddings.LayerNorm.weight"), g("embeddings.LayerNorm.bias"), eps)
    h = _drop(h, masks.get("emb"), p_hidden)
    dh = D // heads
    klen = mask.sum(-1).clamp(1, L)
    dead = (torch.arange(L)[None, :] >= klen[:, None])[:, None, None, :]
    layers = 1 + max(int(k.split(".")[3]) for k in st if k.startswith("model.encoder.layer."))
    for l in range(layers):
        p = f"encoder.layer.{l}."
        lin = lambda x, n: F.linear(x, g(p + n + ".weight"), g(p + n + ".bias"))                 # noqa: E731
        q, k, v = (lin(h, "attention.self." + n).view(R, L, heads, dh).transpose(1, 2) for n in ("query", "key", "value"))
        s = (torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(dh)).masked_fill(dead, float("-inf"))
        w = _drop(torch.softmax(s, dim=-1), masks.get(("attn", l)), p_attn)
        a = torch.matmul(w, v).transpose(1, 2).reshape(R, L, D)
        a = _drop(lin(a, "attention.output.dense"), masks.get(("ao", l)), p_hidden)
        h = F.layer_norm(h + a, (D,), g(p + "attention.output.LayerNorm.weight"), g(p + "attention.output.LayerNorm.bias"), eps)
        f = lin(gelu(lin(h, "intermediate.dense")), "output.dense")
        f = _drop(f, masks.get(("out", l)), p_hidden)
        h = F.layer_norm(h + f, (D,), g(p + "output.LayerNorm.weight"), g(p + "output.LayerNorm.bias"), eps)
    pooled = torch.tanh(F.linear(h[:, 0], g("pooler.dense.weight"), g("pooler.dense.bias")))

    def proj(x):
        x = F.relu(F.linear(x, st["projection.linear1.weight"], st["projection.linear1.bias"]))
        return F.linear(x, st["projection.linear2.weight"], st["projection.linear2.bias"])
    return proj(h), F.normalize(proj(pooled), dim=-1)


def objective_weights(R, L, P, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(R, L, P, generator=g).to(dtype), torch.randn(R, P, generator=g).to(dtype)


def objective(tok, seq, wt, ws):
    return (tok * wt).sum() + 3.0 * (seq * ws).sum()


def results(st, ids, mask, heads, dtype, eps=1e-12, pad_id=1, seed=8, masks=None, p_hidden=0.0, p_attn=0.0, wt=None, ws=None):
    """token_emb, seq_emb and d<name> for every parameter of the objective, run in ``dtype`` on the CPU."""
    s = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in st.items()}
    tok, seq = forward(s, ids, mask, heads, eps, pad_id, masks, p_hidden, p_attn)
    if wt is None:
        wt, ws = objective_weights(*tok.shape, seed, dtype)
    objective(tok, seq, wt.to(dtype), ws.to(dtype)).backward()
    out = {"token_emb": tok.detach(), "seq_emb": seq.detach()}
    out.update({"d" + k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in s.items()})
    return out


def bound(dev):
    """The rule of tests/test_gpu_text_rnn.py: 5e-6 of the tensor's largest entry where the reference's own fp32 deviation is
    below 1.25e-6, else 4 x that deviation."""
    return 5e-6 if dev < 1.25e-6 else 4.0 * dev
