"""Plain-torch restatement of the reference's IntraAttention text encoder (models/text_encoder.py:147-237: per layer the unscaled
score drop(x + pe) drop(x + pe)^T with cells outside the phrase FILLED WITH 1e-10, softmax over all L cells, message = attn @ x,
then the shared ConvGRUCell on [message ; x]) and of the kernels alone (csrc/text_intra.hip: the core and the cell's element-wise
steps, forward and explicit-formula backward), any dtype.  Defined for every text_len in [0, L] and for leading dimensions.
Dropout masks are optional arguments (0/1 keep masks, applied as (x + pe) * mask / (1 - p)).  Used by the CPU and the GPU tests;
tests/golden/make_golden_text_intra.py asserts that it equals the imported reference to 1e-12 in fp64 before the fixture
tests/golden/text_intra.npz is written.  Nothing here touches the HIP library."""
import math

import numpy as np
import torch

from tests.text_selfattn_ref import checksum, position_table, rel_err, state_checksum  # noqa: F401

DEAD = 1e-10

# (V, E, R, L, layers); scale: the table's standard deviation; agg: EmbeddingAgg as the inner module; short: max(text_len) < L
CONFIGS = {
    "e64_n2": dict(V=200, E=64, R=48, L=9, layers=2, scale=1.0, agg=False, short=False, seed=9101),
    "e32_n1": dict(V=200, E=32, R=16, L=12, layers=1, scale=0.5, agg=False, short=False, seed=9102),
    "e64_n3": dict(V=120, E=64, R=8, L=5, layers=3, scale=0.2, agg=False, short=True, seed=9103),
    "e16_agg": dict(V=40, E=16, R=6, L=7, layers=2, scale=0.5, agg=True, short=False, seed=9104),
}
# the whole-model case: BiEncoder(CrnnEncoder(32000, 256), IntraAttention(EmbeddingLayer(200, 256), 2), DotProduct(), 256), eval
MODEL = dict(V=200, E=256, layers=2, scale=0.2, crnn_seed=81, text_seed=83, batch_seed=85, samples=48000)

GATE_NAMES = ["conv_gru.reset_gate.weight", "conv_gru.reset_gate.bias", "conv_gru.update_gate.weight", "conv_gru.update_gate.bias",
              "conv_gru.out_gate.weight", "conv_gru.out_gate.bias"]


def table_name(agg=False):
    return "embedding.embedding.core.weight" if agg else "embedding.core.weight"


def param_names(agg=False):
    return [table_name(agg)] + GATE_NAMES


def state_names(agg=False):
    return [table_name(agg), "pe.pe"] + GATE_NAMES


def draw_params(V, E, seed, scale=1.0, agg=False):
    """fp32 state dict (the pe.pe buffer included); numpy's generator: stable across torch versions.  The biases are drawn
    NON-zero (the module constructs them as zeros, which would leave their paths idle), the gate weights at +-1/sqrt(2E).
    Every value is rounded to an fp16-representable fp32 number: 13 zero mantissa bits keep the compressed fixture small."""
    rs = np.random.RandomState(seed)
    k = 1.0 / math.sqrt(2 * E)
    f = lambda a: torch.from_numpy(a.astype(np.float16).astype(np.float32))           # noqa: E731
    st = {table_name(agg): f(scale * rs.standard_normal((V, E))), "pe.pe": position_table(E)}
    for g in ("reset_gate", "update_gate", "out_gate"):
        st[f"conv_gru.{g}.weight"] = f(rs.uniform(-k, k, (E, 2 * E)))
        st[f"conv_gru.{g}.bias"] = f(rs.uniform(-0.2, 0.2, (E,)))
    return st


def draw_inputs(cfg, zero=False):
    """Token ids (pad id 0 behind text_len) and lengths; the first two rows have length 1 and L (L - 1 in a ``short``
    configuration, where max(text_len) < L).  zero=True: a 0 in row 0 -- what the reference turns into a 0/0 seq_emb."""
    rs = np.random.RandomState(cfg["seed"] + 1)
    R, L, V = cfg["R"], cfg["L"], cfg["V"]
    top = L - 1 if cfg["short"] else L
    lens = rs.randint(1, top + 1, R)
    lens[0], lens[1] = 1, top
    if zero:
        lens[0] = 0
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


def valid_cells(text_len, L):
    """(R, L, L) bool: query AND key inside the phrase."""
    inside = torch.arange(L, device=text_len.device)[None, :] < text_len.clamp(0, L)[:, None]
    return inside[:, :, None] & inside[:, None, :]


# ---- the attention core: what tag_text_intra_forward / tag_text_intra_backward compute ----
def _dropped(x, pe, mask, p):
    v = x + pe[:x.shape[1]].to(x.dtype)
    return v if mask is None else v * mask.to(x.dtype) / (1.0 - p)


def core(x, pe, text_len, mask_a=None, mask_b=None, p=0.0):
    """x (R, L, E), pe (>= L, E), text_len (R) -> message (R, L, E), attn (R, L, L) = the softmax output, dead cells included.
    mask_a / mask_b: 0/1 keep masks (R, L, E) of the two dropouts behind the positions."""
    L = x.shape[1]
    a, b = _dropped(x, pe, mask_a, p), _dropped(x, pe, mask_b, p)
    score = (a @ b.transpose(1, 2)).masked_fill(~valid_cells(text_len.to(x.device), L), DEAD)
    attn = torch.softmax(score, dim=2)
    return attn @ x, attn


def core_backward(dmsg, x, pe, attn, text_len, mask_a=None, mask_b=None, p=0.0):
    """The backward launch restated as explicit formulas -> dx (R, L, E)."""
    L = x.shape[1]
    a, b = _dropped(x, pe, mask_a, p), _dropped(x, pe, mask_b, p)
    dattn = dmsg @ x.transpose(1, 2)
    ds = attn * (dattn - (attn * dattn).sum(-1, keepdim=True))
    ds = ds.masked_fill(~valid_cells(text_len.to(x.device), L), 0.0)
    da, db = ds @ b, ds.transpose(1, 2) @ a
    ka = 1.0 if mask_a is None else mask_a.to(x.dtype) / (1.0 - p)
    kb = 1.0 if mask_b is None else mask_b.to(x.dtype) / (1.0 - p)
    return attn.transpose(1, 2) @ dmsg + da * ka + db * kb


def core_results(x, pe, text_len, dmsg, dtype, mask_a=None, mask_b=None, p=0.0):
    """message, attn and dx of sum(message * dmsg), in ``dtype`` on the CPU through plain autograd."""
    xx = x.detach().to(dtype).clone().requires_grad_(True)
    msg, attn = core(xx, pe.to(dtype), text_len, mask_a, mask_b, p)
    (msg * dmsg.to(dtype)).sum().backward()
    return dict(message=msg.detach(), attn=attn.detach(), dx=xx.grad)


# ---- the ConvGRUCell: what the gate GEMMs and tag_convgru_* compute ----
def masked_mean(x, text_len):
    """mean_with_lens: the sum over the first text_len positions divided by text_len (0/0 for an empty phrase)."""
    L = x.shape[1]
    inside = (torch.arange(L, device=x.device)[None, :] < text_len.to(x.device)[:, None]).to(x.dtype)
    return (x * inside[:, :, None]).sum(1) / text_len.to(x.device, x.dtype)[:, None]


def cell_elementwise(u_pre, r_pre, x):
    """tag_convgru_gates_forward: -> u, r, x * r."""
    u, r = torch.sigmoid(u_pre), torch.sigmoid(r_pre)
    return u, r, x * r


def cell_update(o_pre, u, x):
    """tag_convgru_update_forward without the mean: -> o, xnew."""
    o = torch.tanh(o_pre)
    return o, x * (1 - u) + o * u


def cell_update_backward(dnew, dseq, text_len, x, u, o):
    """tag_convgru_update_backward: x, u, o (R, L, E); dnew (R, L, E) or None, dseq (R, E) or None -> do_pre, du_pre, dx."""
    R, L, _ = x.shape
    g = torch.zeros_like(x) if dnew is None else dnew.clone()
    if dseq is not None:
        inside = torch.arange(L, device=x.device)[None, :] < text_len.to(x.device)[:, None]
        share = (dseq / text_len.to(x.device, x.dtype)[:, None])[:, None, :]           # 0/0 for an empty phrase: never added
        g = g + torch.where(inside[:, :, None], share, torch.zeros_like(share))
    return g * u * (1 - o * o), g * (o - x) * u * (1 - u), g * (1 - u)


def cell_gates_backward(dxr, x, r, dx):
    """tag_convgru_gates_backward: -> dr_pre, dx + dxr * r."""
    return dxr * x * r * (1 - r), dx + dxr * r


def cell(msg, x, st):
    """ConvGRUCell.forward(message, x) (models/text_encoder.py:180-188)."""
    cat = torch.cat([msg, x], dim=-1)
    u_pre = cat @ st["conv_gru.update_gate.weight"].t() + st["conv_gru.update_gate.bias"]
    r_pre = cat @ st["conv_gru.reset_gate.weight"].t() + st["conv_gru.reset_gate.bias"]
    u, r, xr = cell_elementwise(u_pre, r_pre, x)
    o_pre = torch.cat([msg, xr], dim=-1) @ st["conv_gru.out_gate.weight"].t() + st["conv_gru.out_gate.bias"]
    return cell_update(o_pre, u, x)[1]


# ---- the encoder ----
def layers_forward(x, text_len, st, layers, masks=None, p=0.0):
    """What torch.ops.tag.text_intra computes: x (R, L, E) embedded tokens -> token_emb, seq_emb.  masks: per layer a pair of
    0/1 keep masks (R, L, E), or None."""
    pe = st["pe.pe"][0]
    for l in range(layers):
        ma, mb = masks[l] if masks is not None else (None, None)
        msg, _ = core(x, pe, text_len, ma, mb, p)
        x = cell(msg, x, st)
    return x, masked_mean(x, text_len)


def encoder_forward(st, text, text_len, layers, masks=None, p=0.0, agg=False):
    """st: state dict (any dtype, tensors may require grad); text (..., L), text_len (...).  -> token_emb (..., L, E),
    seq_emb (..., E)."""
    table = st[table_name(agg)]
    lead = tuple(text.shape[:-1])
    x = table[text.long().reshape(-1, text.shape[-1]).to(table.device)]
    tok, seq = layers_forward(x, torch.as_tensor(text_len).reshape(-1), st, layers, masks, p)
    return tok.reshape(*lead, *tok.shape[1:]), seq.reshape(*lead, seq.shape[-1])


def config_results(cfg, st, text, text_len, dtype, masks=None, p=0.0, layers=None):
    """token_emb, seq_emb and every parameter gradient of the fixed objective, in ``dtype`` on the CPU."""
    names = param_names(cfg["agg"])
    s = {k: v.detach().to(dtype).clone().requires_grad_(k in names) for k, v in st.items()}
    tok, seq = encoder_forward(s, text, text_len, cfg["layers"] if layers is None else layers, masks, p, cfg["agg"])
    wt, ws = objective_weights(cfg, dtype)
    objective(tok, seq, wt, ws).backward()
    out = {"token_emb": tok.detach(), "seq_emb": seq.detach()}
    out.update({"d" + k: (s[k].grad if s[k].grad is not None else torch.zeros_like(s[k])) for k in names})
    return out


# ---- whole-model case ----
def model_text_state():
    m = MODEL
    return draw_params(m["V"], m["E"], m["text_seed"], m["scale"])


def model_state():
    """fp32 state dict of the whole-model case keyed like BiEncoder's: the oracle's seeded CrnnEncoder + the seeded text encoder."""
    from oracle import tag_oracle as O
    st = dict(O.init_crnn_state(seed=MODEL["crnn_seed"], embed_dim=256))
    st.update({"text_encoder." + k: v for k, v in model_text_state().items()})
    return st


def model_batch():
    """The oracle's ragged batch, the token tensor as the oracle pads it."""
    from oracle import tag_oracle as O
    return O.synthetic_batch(2, MODEL["samples"], seed=MODEL["batch_seed"], ragged=True, hop=640, vocab_size=MODEL["V"])
