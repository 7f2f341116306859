"""Differentiable restatement of BERT as Bert / SentenceBert train it (models/text_encoder.py:271-308 over Hugging Face's
BertModel): BertEmbeddings, the post-LayerNorm stack, the two sentence poolings and the three normalisations; any dtype, CPU, with
INJECTED dropout masks, plus the restatement of every kernel of csrc/text_bert.hip.  TEST INFRASTRUCTURE ONLY.
tests/golden/make_golden_text_bert.py asserts the forward and all parameter gradients equal the real transformers module in fp64
to 1e-12."""
import math

import torch
import torch.nn.functional as F

from tests.text_clap_ref import HEAD, LAYER, _drop, bound, gelu, ln_backward, ln_forward, rel_err  # noqa: F401

#: the tiny configuration of tests/golden/text_bert.npz (dropouts 0; the tests that want dropout pass masks)
TINY = dict(vocab_size=120, hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=160,
            max_position_embeddings=72, type_vocab_size=2, layer_norm_eps=1e-12, pad_token_id=0, hidden_dropout_prob=0.0,
            attention_probs_dropout_prob=0.0)
#: all-MiniLM-L6-v2's shape with a small vocabulary
MINILM = dict(vocab_size=300, hidden_size=384, num_hidden_layers=6, num_attention_heads=12, intermediate_size=1536,
              max_position_embeddings=72, type_vocab_size=2, layer_norm_eps=1e-12, pad_token_id=0, hidden_dropout_prob=0.0,
              attention_probs_dropout_prob=0.0)
FIXTURE = dict(R=5, L=9, state_seed=31, input_seed=5, objective_seed=12)
#: the fixture's cases: name -> (pooling mode, normalisation)
CASES = {"cls": (0, 0), "mean_norm": (1, 1), "mean": (1, 0)}
POOLER = ("model.pooler.dense.weight", "model.pooler.dense.bias")


def param_names(layers, pooler=False):
    return (["model." + n for n in HEAD] + [f"model.encoder.layer.{l}.{n}" for l in range(layers) for n in LAYER]
            + (list(POOLER) if pooler else []))


def param_shapes(cfg, pooler=False):
    D, I = cfg["hidden_size"], cfg["intermediate_size"]
    head = [(cfg["vocab_size"], D), (cfg["type_vocab_size"], D), (cfg["max_position_embeddings"], D), (D,), (D,)]
    layer = [(D, D), (D,)] * 4 + [(D,), (D,), (I, D), (I,), (D, I), (D,), (D,), (D,)]
    return head + layer * cfg["num_hidden_layers"] + ([(D, D), (D,)] if pooler else [])


def draw_state(cfg, seed, scale=None, pooler=True):
    """Seeded fp32 parameters by name: N(0, scale^2), scale ~ 1.5 / sqrt(fan_in) for matrices so that every stage matters,
    LayerNorm weights 1 + N(0, 0.1^2), the pad row of the word table zero as nn.Embedding leaves it."""
    g = torch.Generator().manual_seed(seed)
    st = {}
    for name, shape in zip(param_names(cfg["num_hidden_layers"], pooler), param_shapes(cfg, pooler)):
        if "LayerNorm.weight" in name:
            st[name] = 1.0 + 0.1 * torch.randn(*shape, generator=g)
        elif "embeddings" in name and len(shape) == 2:
            st[name] = 0.5 * torch.randn(*shape, generator=g)
        elif len(shape) == 2:
            st[name] = torch.randn(*shape, generator=g) * ((scale or 1.5) / math.sqrt(shape[1]))
        else:
            st[name] = 0.1 * torch.randn(*shape, generator=g)
    st["model.embeddings.word_embeddings.weight"][cfg["pad_token_id"]] = 0.0
    return st


def draw_inputs(R, L, seed, vocab=120, types=2, pad_id=0):
    """BERT-style rows [CLS] ... [SEP] right-padded with pad_id: row 0 full, row 1 cut down to its first TWO tokens (when R > 1),
    the others of length 2 ... L; ids drawn from a few values so that they repeat within and across rows; mixed type ids (the
    second half of every phrase is type 1 ... types - 1, pads type 0).  -> ids, type_ids, mask."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((R, L), pad_id, dtype=torch.long)
    tps = torch.zeros(R, L, dtype=torch.long)
    mask = torch.zeros(R, L, dtype=torch.long)
    pool = torch.randint(3, vocab, (max(4, (R * L) // 3),), generator=g)
    for r in range(R):
        n = L if r == 0 else (2 if r == 1 else int(torch.randint(2, L + 1, (1,), generator=g)))
        ids[r, 0] = 1
        if n > 2:
            ids[r, 1:n - 1] = pool[torch.randint(0, len(pool), (n - 2,), generator=g)]
        ids[r, n - 1] = 2
        if types > 1:
            tps[r, n // 2:n] = 1 + (r % (types - 1))
        mask[r, :n] = 1
    return ids, tps, mask


# ---------------------------------------------------------------------------------------------- the kernels, restated
def embed_forward(ids, type_ids, word, type_tab, pos, gamma, beta, eps):
    """-> h (B*L, D), xhat, rstd; the position of a token is its column."""
    B, L = ids.shape
    t = type_tab[type_ids] if type_ids is not None else type_tab[0]
    s = word[ids] + t + pos[:L]
    return ln_forward(s.reshape(-1, s.shape[-1]), None, gamma, beta, eps)


def embed_backward(dh, xhat, rstd, gamma, ids, type_ids, V, T, P, pad_id):
    """-> dword (V, D), dtype (T, D), dpos (P, D), dgamma, dbeta; row pad_id of dword exactly zero, pads count in dtype, dpos."""
    ds, dg, db = ln_backward(dh, xhat, rstd, gamma)
    B, L = ids.shape
    D = dh.shape[-1]
    keep = ids.reshape(-1).ne(pad_id).to(ds.dtype).unsqueeze(-1)
    dword = torch.zeros(V, D, dtype=ds.dtype).index_add_(0, ids.reshape(-1), ds * keep)
    tt = type_ids.reshape(-1) if type_ids is not None else torch.zeros(B * L, dtype=torch.long)
    dtype_ = torch.zeros(T, D, dtype=ds.dtype).index_add_(0, tt, ds)
    dpos = torch.zeros(P, D, dtype=ds.dtype)
    dpos[:L] = ds.view(B, L, D).sum(0)
    return dword, dtype_, dpos, dg, db


def pool(h, klen, mode, norm):
    """h (R, L, D), klen (R) -> seq (R, D), raw (R, D): differentiable."""
    R, L, D = h.shape
    if mode == 0:
        raw = h[:, 0]
    else:
        m = (torch.arange(L)[None, :] < klen[:, None]).to(h.dtype).unsqueeze(-1)
        raw = (h * m).sum(1) / klen.to(h.dtype).clamp_min(1e-9).unsqueeze(-1)
    if norm == 0:
        return raw, raw
    if norm == 1:
        return F.normalize(raw, p=2.0, dim=-1, eps=1e-12), raw
    n = raw.norm(p=2, dim=-1, keepdim=True)
    return raw.div(n + 1e-7).clip(-1e3, 1e3), raw


def pool_backward(dseq, dtok, h, klen, mode, norm):
    """dh of (seq * dseq).sum() + (h * dtok).sum() by autograd."""
    x = h.detach().clone().requires_grad_(True)
    seq, _ = pool(x, klen, mode, norm)
    obj = (seq * dseq).sum() if dseq is not None else x.sum() * 0
    if dtok is not None:
        obj = obj + (x * dtok).sum()
    obj.backward()
    return x.grad


# ---------------------------------------------------------------------------------------------- the whole encoder
def layer(st, prefix, h, dead, heads, eps, masks, l, p_hidden, p_attn):
    R, L, D = h.shape
    dh = D // heads
    lin = lambda x, n: F.linear(x, st[prefix + n + ".weight"], st[prefix + n + ".bias"])                 # noqa: E731
    q, k, v = (lin(h, "attention.self." + n).view(R, L, heads, dh).transpose(1, 2) for n in ("query", "key", "value"))
    s = (torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(dh)).masked_fill(dead, float("-inf"))
    w = _drop(torch.softmax(s, dim=-1), masks.get(("attn", l)), p_attn)
    a = torch.matmul(w, v).transpose(1, 2).reshape(R, L, D)
    a = _drop(lin(a, "attention.output.dense"), masks.get(("ao", l)), p_hidden)
    h = F.layer_norm(h + a, (D,), st[prefix + "attention.output.LayerNorm.weight"], st[prefix + "attention.output.LayerNorm.bias"], eps)
    f = lin(gelu(lin(h, "intermediate.dense")), "output.dense")
    f = _drop(f, masks.get(("out", l)), p_hidden)
    return F.layer_norm(h + f, (D,), st[prefix + "output.LayerNorm.weight"], st[prefix + "output.LayerNorm.bias"], eps)


def forward(st, ids, type_ids, mask, heads, mode, norm, eps=1e-12, pad_id=0, masks=None, p_hidden=0.0, p_attn=0.0):
    """st: parameters by state-dict name (any dtype; the pooler's are not read).  masks: {"emb": (R*L, D), ("attn", l): (R, H, L, L),
    ("ao", l), ("out", l): (R*L, D)} keep masks or None.  Keys >= klen = max(mask.sum(-1), 1) are masked.
    -> token_emb (R, L, D) the last hidden state, seq_emb (R, D)."""
    masks = masks or {}
    g = lambda k: st["model." + k]                           # noqa: E731
    R, L = ids.shape
    tt = type_ids if type_ids is not None else torch.zeros_like(ids)
    h = F.embedding(ids, g("embeddings.word_embeddings.weight"), padding_idx=pad_id) \
        + F.embedding(tt, g("embeddings.token_type_embeddings.weight")) + g("embeddings.position_embeddings.weight")[:L]
    D = h.shape[-1]
    h = F.layer_norm(h, (D,), g("embeddings.LayerNorm.weight"), g("embeddings.LayerNorm.bias"), eps)
    h = _drop(h, masks.get("emb"), p_hidden)
    klen = mask.sum(-1)
    dead = (torch.arange(L)[None, :] >= klen.clamp(1, L)[:, None])[:, None, None, :]
    layers = 1 + max(int(k.split(".")[3]) for k in st if k.startswith("model.encoder.layer."))
    for l in range(layers):
        h = layer(st, f"model.encoder.layer.{l}.", h, dead, heads, eps, masks, l, p_hidden, p_attn)
    seq, _ = pool(h, klen, mode, norm)
    return h, seq


def objective_weights(R, L, D, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(R, L, D, generator=g).to(dtype), torch.randn(R, D, generator=g).to(dtype)


def objective(tok, seq, wt, ws):
    return (tok * wt).sum() + 3.0 * (seq * ws).sum()


def results(st, ids, type_ids, mask, heads, mode, norm, dtype, eps=1e-12, pad_id=0, seed=12, masks=None, p_hidden=0.0, p_attn=0.0):
    """token_emb, seq_emb and d<name> for every parameter of the objective, run in ``dtype`` on the CPU."""
    s = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in st.items()}
    tok, seq = forward(s, ids, type_ids, mask, heads, mode, norm, eps, pad_id, masks, p_hidden, p_attn)
    wt, ws = objective_weights(*tok.shape, seed, dtype)
    objective(tok, seq, wt, ws).backward()
    out = {"token_emb": tok.detach(), "seq_emb": seq.detach()}
    out.update({"d" + k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in s.items()})
    return out


def quantity_err(got, ref, k):
    """Error of quantity k relative to the largest entry of the reference tensor; the key bias's gradient is zero up to rounding
    and is measured against the scale of the query bias's gradient (tests/text_clap_ref.quantity_err)."""
    return rel_err(got[k], ref[k], ref[k.replace("key.bias", "query.bias")])
