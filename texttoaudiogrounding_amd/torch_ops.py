"""``torch.library`` registration of the hot-path kernels (namespace ``tag``) -- the op list SURVEY.md section 8(b) asks a
native replacement to export, with schemas, fake (meta) kernels for shape inference / tracing and autograd formulas, on top
of the SAME C ABI (libtag_hip.so through ctypes, texttoaudiogrounding_amd.lib): PyTorch sees these as first-class operators
(``torch.ops.tag.logmel`` ...).  They are the FRONT door: the reference-shaped modules call them (models/match.py ->
``frame_match``, models/align.py -> ``align_dot``, losses.py -> ``frame_bce``, models/text_encoder.py -> ``embed_mean``,
models/panns.py ConvBlock.forward -> ``conv3x3_bn_relu_pool``, utils/eval_util.py -> ``segments``).  Every formula exists
once: an operator's forward / backward body is a plain function of ``ops.py`` (``ops.match_forward`` / ``ops.match_backward``
...).  The fused encoders are operators too (``tag::cnn8rnn_encoder`` / ``tag::crnn_encoder``, round 4): they wrap the engine
of ``ops.py`` (``ops.Cnn8RnnFunction`` / ``ops.CrnnFunction`` never materialise the intermediate activations and write
parameter gradients straight into the flat buffer -- per-step state that travels beside the operator, see below);
``ops.EmbedMeanFunction`` (the direct-gradient scatter) is the one autograd node the modules still apply directly.

    import texttoaudiogrounding_amd.torch_ops          # registers torch.ops.tag.*

Every op takes contiguous fp32 device tensors on the current stream and raises on CPU tensors (no fallback).  Backward passes
are ops themselves (``tag::*_backward``), so a graph captured through these operators contains only ``tag::`` nodes for the
path.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch
from torch import Tensor
from torch.library import custom_op, register_autograd

from . import dispatch as _dispatch
from . import engine, ops

__all__ = ["OP_NAMES"]


# ------------------------------------------------------------------------------------------------ F1/F2 log-mel
@custom_op("tag::logmel", mutates_args=())
def logmel(waveform: Tensor, n_fft: int, win_length: int, hop: int, window: Tensor, fb: Tensor) -> Tensor:
    """(B,S) -> (B, S//hop + 1, n_mels) dB log-mel, time-major (rows F1/F2)."""
    return ops.logmel(waveform, n_fft, win_length, hop, window, fb)


@logmel.register_fake
def _(waveform, n_fft, win_length, hop, window, fb):
    return waveform.new_empty(waveform.shape[0], waveform.shape[1] // hop + 1, fb.shape[1])


# ------------------------------------------------------------------------------------------------ A1 conv 3x3
@custom_op("tag::conv3x3", mutates_args=())
def conv3x3(x: Tensor, weight: Tensor, prologue: int, scale: Optional[Tensor], shift: Optional[Tensor]) -> Tensor:
    """y = conv3x3(prologue(x)), channels-last (B,H,W,Cin) x (Cout,Cin,3,3) -> (B,H,W,Cout); prologue 1 folds the producer's
    BatchNorm + ReLU (relu(x * scale + shift)) into the operand load."""
    wf, _ = ops.pack_conv_weight(weight, want_dgrad=False, W=x.shape[2])
    return ops.conv3x3(x, wf, weight.shape[0], prologue, scale, shift)


@conv3x3.register_fake
def _(x, weight, prologue, scale, shift):
    return x.new_empty(x.shape[0], x.shape[1], x.shape[2], weight.shape[0])


@custom_op("tag::conv3x3_dgrad", mutates_args=())
def conv3x3_dgrad(dy: Tensor, weight: Tensor) -> Tensor:
    """Gradient of conv3x3 (prologue 0) with respect to its input: (B,H,W,Cout) -> (B,H,W,Cin)."""
    _, wd = ops.pack_conv_weight(weight, want_dgrad=True, W=dy.shape[2])
    return ops.conv3x3(dy, wd, weight.shape[1])


@conv3x3_dgrad.register_fake
def _(dy, weight):
    return dy.new_empty(dy.shape[0], dy.shape[1], dy.shape[2], weight.shape[1])


@custom_op("tag::conv3x3_wgrad", mutates_args=())
def conv3x3_wgrad(x: Tensor, dy: Tensor, prologue: int, scale: Optional[Tensor], shift: Optional[Tensor]) -> Tensor:
    """Weight gradient (Cout,Cin,3,3) of y = conv3x3(prologue(x))."""
    return ops.conv3x3_wgrad(x, dy, prologue, scale, shift)


@conv3x3_wgrad.register_fake
def _(x, dy, prologue, scale, shift):
    return x.new_empty(dy.shape[3], x.shape[3], 3, 3)


def _conv_setup(ctx, inputs, output):
    x, weight, prologue, scale, shift = inputs
    if prologue != 0 and (x.requires_grad or (scale is not None and scale.requires_grad)):
        raise RuntimeError("tag::conv3x3: the autograd formula covers prologue = 0 (the fused BatchNorm prologue is "
                           "differentiated by ops.Cnn8RnnFunction, which owns the batch statistics)")
    ctx.save_for_backward(x, weight)
    ctx.pro = (prologue, scale, shift)


def _conv_backward(ctx, dy):
    x, weight = ctx.saved_tensors
    prologue, scale, shift = ctx.pro
    dy = dy.contiguous()
    dx = torch.ops.tag.conv3x3_dgrad(dy, weight) if ctx.needs_input_grad[0] else None
    dw = torch.ops.tag.conv3x3_wgrad(x, dy, prologue, scale, shift) if ctx.needs_input_grad[1] else None
    return dx, dw, None, None, None


register_autograd("tag::conv3x3", _conv_backward, setup_context=_conv_setup)


# ------------------------------------------------------------------------------------------------ A1 conv3x3 -> BN -> ReLU (-> pool)
@custom_op("tag::conv3x3_bn_relu_pool", mutates_args=())
def conv3x3_bn_relu_pool(x: Tensor, weight: Tensor, gamma: Tensor, beta: Tensor, running_mean: Tensor, running_var: Tensor,
                         training: bool, momentum: float, eps: float, ph: int, pw: int,
                         pool: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """One stage of ConvBlock.forward (models/panns.py:46-62), channels-last: relu(bn(conv3x3(x))) then pooling with kernel =
    stride = (ph, pw) (1,1 = none); pool 0 'avg+max' | 2 'avg' | 3 'max'.  x (B,H,W,Cin) with Cin = 1 or a multiple of 32,
    weight (Cout,Cin,3,3).  Functional (an operator with an autograd formula may not mutate its inputs): train mode uses the
    batch statistics and RETURNS the updated running statistics, which the caller copies into the BatchNorm buffers.
    -> (out (B,H/ph,W/pw,Cout), y = raw conv output, mean, invstd, scale, shift, new_running_mean, new_running_var)."""
    rm, rv = running_mean.clone(), running_var.clone()
    out, y, st = ops.conv_bn_relu_pool_forward(x, weight, gamma, beta, rm, rv, training, momentum, eps, ph, pw, pool)
    mean = st.mean.clone() if not training else st.mean           # eval: st.mean IS rm (no aliased outputs)
    return out, y, mean, st.invstd, st.scale, st.shift, rm, rv


@conv3x3_bn_relu_pool.register_fake
def _(x, weight, gamma, beta, running_mean, running_var, training, momentum, eps, ph, pw, pool):
    B, H, W, _ = x.shape
    C = weight.shape[0]
    v = lambda: x.new_empty(C)
    return x.new_empty(B, H // ph, W // pw, C), x.new_empty(B, H, W, C), v(), v(), v(), v(), v(), v()


@custom_op("tag::conv3x3_bn_relu_pool_backward", mutates_args=())
def conv3x3_bn_relu_pool_backward(dout: Tensor, x: Tensor, weight: Tensor, y: Tensor, mean: Tensor, invstd: Tensor, scale: Tensor,
                                  shift: Tensor, gamma: Tensor, training: bool, ph: int, pw: int, pool: int,
                                  need_dx: bool) -> List[Tensor]:
    """-> [dx (empty (0,) tensor when not needed), dweight, dgamma, dbeta]."""
    st = ops.BNStat()
    st.mean, st.invstd, st.scale, st.shift, st.train = mean, invstd, scale, shift, bool(training)
    dx, dw, dg, db = ops.conv_bn_relu_pool_backward(dout, x, weight, y, st, gamma, ph, pw, pool, need_dx)
    return [dx if dx is not None else x.new_empty(0), dw, dg, db]


@conv3x3_bn_relu_pool_backward.register_fake
def _(dout, x, weight, y, mean, invstd, scale, shift, gamma, training, ph, pw, pool, need_dx):
    return [torch.empty_like(x) if need_dx else x.new_empty(0), torch.empty_like(weight), torch.empty_like(gamma),
            torch.empty_like(gamma)]


def _cbrp_setup(ctx, inputs, output):
    x, weight, gamma, _beta, _rm, _rv, training, _mom, _eps, ph, pw, pool = inputs
    _out, y, mean, invstd, scale, shift, _rm, _rv = output
    ctx.save_for_backward(x, weight, y, mean, invstd, scale, shift, gamma)
    ctx.cfg = (training, ph, pw, pool)


def _cbrp_backward(ctx, dout, *_unused):
    x, weight, y, mean, invstd, scale, shift, gamma = ctx.saved_tensors
    training, ph, pw, pool = ctx.cfg
    dx, dw, dg, db = torch.ops.tag.conv3x3_bn_relu_pool_backward(dout.contiguous(), x, weight, y, mean, invstd, scale, shift, gamma,
                                                                 training, ph, pw, pool, ctx.needs_input_grad[0])
    return (dx if ctx.needs_input_grad[0] else None, dw, dg, db, None, None, None, None, None, None, None, None)


register_autograd("tag::conv3x3_bn_relu_pool", _cbrp_backward, setup_context=_cbrp_setup)


# ------------------------------------------------------------------------------------------------ A4 BiGRU
@custom_op("tag::gru_bidir", mutates_args=())
def gru_bidir(x: Tensor, w_ih: Tensor, w_hh: Tensor, b_ih: Tensor, b_hh: Tensor, w_ih_r: Tensor, w_hh_r: Tensor,
              b_ih_r: Tensor, b_hh_r: Tensor) -> Tuple[Tensor, Tensor]:
    """nn.GRU(I, H, bidirectional=True, batch_first=True), h0 = 0: x (B,T,I) -> y (B,T,2H) and the saved gates (B,T,2,4H)."""
    B, T, I = x.shape
    y, sv = ops.gru_bidir_forward(x.reshape(B * T, I), [w_ih, w_hh, b_ih, b_hh, w_ih_r, w_hh_r, b_ih_r, b_hh_r], B, T, True)
    return y, sv["gates"]


@gru_bidir.register_fake
def _(x, w_ih, w_hh, b_ih, b_hh, w_ih_r, w_hh_r, b_ih_r, b_hh_r):
    B, T, _ = x.shape
    H = w_hh.shape[1]
    return x.new_empty(B, T, 2 * H), x.new_empty(B, T, 2, 4 * H)


@custom_op("tag::gru_bidir_backward", mutates_args=())
def gru_bidir_backward(dy: Tensor, x: Tensor, y: Tensor, gates: Tensor, w_ih: Tensor, w_hh: Tensor, w_ih_r: Tensor,
                       w_hh_r: Tensor) -> List[Tensor]:
    """-> [dx, dw_ih, dw_hh, db_ih, db_hh, dw_ih_r, dw_hh_r, db_ih_r, db_hh_r]."""
    B, T, I = x.shape
    H = w_hh.shape[1]
    sv = dict(Hh=H, y=y, gates=gates, w_ih=torch.cat([w_ih, w_ih_r], 0), w_hh=torch.stack([w_hh, w_hh_r], 0).contiguous())
    dx, g = ops.gru_bidir_backward(dy.contiguous(), x.reshape(B * T, I), sv)
    return [dx.view(B, T, I)] + [t.clone() for t in g]          # bias slices share storage: operators may not return aliases


@gru_bidir_backward.register_fake
def _(dy, x, y, gates, w_ih, w_hh, w_ih_r, w_hh_r):
    H = w_hh.shape[1]
    b = x.new_empty(3 * H)
    return [torch.empty_like(x), torch.empty_like(w_ih), torch.empty_like(w_hh), b, torch.empty_like(b),
            torch.empty_like(w_ih_r), torch.empty_like(w_hh_r), torch.empty_like(b), torch.empty_like(b)]


def _gru_setup(ctx, inputs, output):
    x, w_ih, w_hh, _, _, w_ih_r, w_hh_r, _, _ = inputs
    ctx.save_for_backward(x, output[0], output[1], w_ih, w_hh, w_ih_r, w_hh_r)


def _gru_backward(ctx, dy, _dgates):
    x, y, gates, w_ih, w_hh, w_ih_r, w_hh_r = ctx.saved_tensors
    g = torch.ops.tag.gru_bidir_backward(dy, x, y, gates, w_ih, w_hh, w_ih_r, w_hh_r)
    return tuple(g)


register_autograd("tag::gru_bidir", _gru_backward, setup_context=_gru_setup)


# ------------------------------------------------------------------------------------------------ T1/T2 embedding + mean
@custom_op("tag::embed_mean", mutates_args=())
def embed_mean(table: Tensor, text: Tensor, text_len: Tensor) -> Tuple[Tensor, Tensor]:
    """nn.Embedding gather + mean over the valid tokens: -> seq_emb (B,D), token_emb (B,L,D)."""
    return ops.embed_mean_forward(table, text, text_len, True)


@embed_mean.register_fake
def _(table, text, text_len):
    B, L = text.shape
    return table.new_empty(B, table.shape[1]), table.new_empty(B, L, table.shape[1])


@custom_op("tag::embed_mean_backward", mutates_args=())
def embed_mean_backward(dseq: Optional[Tensor], dtok: Optional[Tensor], text: Tensor, text_len: Tensor, V: int, D: int) -> Tensor:
    """Deterministic scatter of the seq_emb / token_emb gradients into a zeroed (V,D) table gradient."""
    return ops.embed_mean_backward_into(torch.zeros(V, D, device=text.device, dtype=torch.float32), dseq, dtok, text, text_len)


@embed_mean_backward.register_fake
def _(dseq, dtok, text, text_len, V, D):
    return torch.empty(V, D, device=text.device, dtype=torch.float32)


def _embed_setup(ctx, inputs, output):
    table, text, text_len = inputs
    ctx.save_for_backward(text, text_len)
    ctx.vd = tuple(table.shape)


def _embed_backward(ctx, dseq, dtok):
    text, text_len = ctx.saved_tensors
    return torch.ops.tag.embed_mean_backward(dseq, dtok, text, text_len, ctx.vd[0], ctx.vd[1]), None, None


register_autograd("tag::embed_mean", _embed_backward, setup_context=_embed_setup)


# ------------------------------------------------------------------------------------------------ T3 text GRU
def _tgru_saved(x, tok, saved, params, dirs, layers, drop_p, seed):
    """The per-layer state ops.text_gru_backward expects, from what the operator returned: saved = the gates of every layer,
    then the hidden states of every layer but the last (the last layer's are token_emb); a deeper layer's input is the
    (dropped) output of the layer below, replayed from its seed."""
    R, L, _ = x.shape
    ys = list(saved[layers:]) + [tok]
    out, inp = [], x.reshape(R * L, -1)
    for l in range(layers):
        w_ih, w_hh, _, _ = _dispatch._text_gru_layer_params(list(params), l, dirs)
        out.append(dict(x=inp, y=ys[l], gates=saved[l], w_ih=w_ih, w_hh=w_hh))
        inp = ys[l].reshape(R * L, -1)
        if drop_p > 0.0 and l + 1 < layers:
            inp = _dispatch.text_gru_dropout(inp, drop_p, _dispatch.text_gru_dropout_seed(seed, l), backward=False)
    return out


@custom_op("tag::text_gru", mutates_args=())
def text_gru(x: Tensor, text_len: Tensor, params: List[Tensor], dirs: int, layers: int, drop_p: float,
             seed: int) -> Tuple[Tensor, Tensor, List[Tensor]]:
    """nn.GRU(E, H, layers, batch_first=True, bidirectional = dirs == 2), h0 = 0, over ALL padded positions of x (R, L, E), then
    the mean over the valid tokens (models/text_encoder.py:119-123): -> token_emb (R, L, dirs*H), seq_emb (R, dirs*H) and the
    saved state (gates (R, L, dirs, 4H) per layer, then the hidden states of every layer but the last).  params: nn.GRU's
    flat weights.  drop_p > 0 applies the inter-layer dropout (the caller passes 0 in eval mode) with the keep mask of ``seed``."""
    tok, seq, saved = ops.text_gru_forward(x, text_len, list(params), dirs, layers, True, drop_p, seed)
    return tok, seq, [sv["gates"] for sv in saved] + [sv["y"] for sv in saved[:-1]]


@text_gru.register_fake
def _(x, text_len, params, dirs, layers, drop_p, seed):
    R, L, _ = x.shape
    H = params[1].shape[1]
    return (x.new_empty(R, L, dirs * H), x.new_empty(R, dirs * H),
            [x.new_empty(R, L, dirs, 4 * H) for _ in range(layers)] + [x.new_empty(R, L, dirs * H) for _ in range(layers - 1)])


@custom_op("tag::text_gru_backward", mutates_args=())
def text_gru_backward(dtok: Optional[Tensor], dseq: Optional[Tensor], x: Tensor, text_len: Tensor, tok: Tensor,
                      saved: List[Tensor], params: List[Tensor], dirs: int, layers: int, drop_p: float, seed: int,
                      need: List[bool], need_dx: bool) -> List[Tensor]:
    """-> [dx] + one gradient per parameter; an entry that is not needed (need[i] / need_dx False) is an empty tensor."""
    sv = _tgru_saved(x, tok, saved, params, dirs, layers, drop_p, seed)
    dx, g = ops.text_gru_backward(dtok, dseq, text_len, sv, dirs, drop_p, seed, need=list(need), need_dx=need_dx)
    none = lambda: x.new_empty(0)                                                    # noqa: E731
    return [dx.clone() if dx is not None else none()] + [t.clone() if t is not None else none() for t in g]


@text_gru_backward.register_fake
def _(dtok, dseq, x, text_len, tok, saved, params, dirs, layers, drop_p, seed, need, need_dx):
    return [torch.empty_like(x) if need_dx else x.new_empty(0)] + [torch.empty_like(p) if n else x.new_empty(0)
                                                                    for p, n in zip(params, need)]


def _tgru_setup(ctx, inputs, output):
    x, text_len, params, dirs, layers, drop_p, seed = inputs
    tok, _, saved = output
    ctx.save_for_backward(x, text_len, tok, *saved, *params)
    ctx.meta = (dirs, layers, drop_p, seed, len(saved))
    ctx.need = [bool(p.requires_grad) for p in params]
    ctx.need_dx = bool(x.requires_grad)


def _tgru_backward(ctx, dtok, dseq, _dsaved):
    dirs, layers, drop_p, seed, ns = ctx.meta
    x, text_len, tok = ctx.saved_tensors[:3]
    saved, params = list(ctx.saved_tensors[3:3 + ns]), list(ctx.saved_tensors[3 + ns:])
    if dtok is not None:
        dtok = dtok.contiguous()
    if dseq is not None:
        dseq = dseq.contiguous()
    g = torch.ops.tag.text_gru_backward(dtok, dseq, x, text_len, tok, saved, params, dirs, layers, drop_p, seed, ctx.need,
                                        ctx.need_dx)
    return (g[0] if ctx.need_dx else None, None, [t if n else None for t, n in zip(g[1:], ctx.need)], None, None, None, None)


register_autograd("tag::text_gru", _tgru_backward, setup_context=_tgru_setup)


# ------------------------------------------------------------------------------------------------ T4 text self-attention
@custom_op("tag::text_selfattn", mutates_args=())
def text_selfattn(tok: Tensor, text_len: Tensor, pe: Tensor, params: List[Tensor], heads: int, drop_p: float,
                  seed: int) -> Tuple[Tensor, List[Tensor]]:
    """SelfAttention behind its embedding (models/text_encoder.py:263-268): tok (R, L, E) embedded tokens, text_len (R) int64,
    pe (>= L+1, E) positions, params = [cls_token, mha.in_proj_weight, mha.in_proj_bias, mha.out_proj.weight,
    mha.out_proj.bias] -> out (R, L+1, E) (row 0 = seq_emb, rows 1.. = token_emb) and the saved state [x, qkv, attn, ctx, klen].
    drop_p > 0 (the caller passes 0 in eval mode): dropout behind the positions and on the attention weights, keep masks of
    ops.text_selfattn_dropout_seeds(seed)."""
    out, sv = ops.text_selfattn_forward(tok, text_len, pe, *params, heads, True, drop_p, seed)
    return out, [sv["x"], sv["qkv"], sv["attn"], sv["ctx"], sv["klen"]]


@text_selfattn.register_fake
def _(tok, text_len, pe, params, heads, drop_p, seed):
    R, L, E = tok.shape
    S = L + 1
    return (tok.new_empty(R, S, E), [tok.new_empty(R, S, E), tok.new_empty(R * S, 3 * E), tok.new_empty(R, heads, S, S),
                                     tok.new_empty(R, S, E), text_len.new_empty(R)])


@custom_op("tag::text_selfattn_backward", mutates_args=())
def text_selfattn_backward(dout: Tensor, saved: List[Tensor], params: List[Tensor], heads: int, drop_p: float, seed: int,
                           need: List[bool], need_dtok: bool) -> List[Tensor]:
    """-> [dtok] + one gradient per parameter; an entry that is not needed (need[i] / need_dtok False) is an empty tensor."""
    x, qkv, attn, ctx, klen = saved
    sv = dict(x=x, qkv=qkv, attn=attn, ctx=ctx, klen=klen, w_in=params[1].contiguous(), w_out=params[3].contiguous())
    dtok, g = ops.text_selfattn_backward(dout, sv, heads, drop_p, seed, need=list(need), need_dtok=need_dtok)
    none = lambda: dout.new_empty(0)                                                 # noqa: E731
    return [dtok if dtok is not None else none()] + [t.view(p.shape) if t is not None else none() for t, p in zip(g, params)]


@text_selfattn_backward.register_fake
def _(dout, saved, params, heads, drop_p, seed, need, need_dtok):
    R, S, E = dout.shape
    return [dout.new_empty(R, S - 1, E) if need_dtok else dout.new_empty(0)] + [torch.empty_like(p) if n else dout.new_empty(0)
                                                                               for p, n in zip(params, need)]


def _tsa_setup(ctx, inputs, output):
    tok, text_len, pe, params, heads, drop_p, seed = inputs
    _, saved = output
    ctx.save_for_backward(*saved, *params)
    ctx.meta = (heads, drop_p, seed, len(saved))
    ctx.need = [bool(p.requires_grad) for p in params]
    ctx.need_dtok = bool(tok.requires_grad)


def _tsa_backward(ctx, dout, _dsaved):
    heads, drop_p, seed, ns = ctx.meta
    saved, params = list(ctx.saved_tensors[:ns]), list(ctx.saved_tensors[ns:])
    g = torch.ops.tag.text_selfattn_backward(dout.contiguous(), saved, params, heads, drop_p, seed, ctx.need, ctx.need_dtok)
    return (g[0] if ctx.need_dtok else None, None, None, [t if n else None for t, n in zip(g[1:], ctx.need)], None, None, None)


register_autograd("tag::text_selfattn", _tsa_backward, setup_context=_tsa_setup)


# ------------------------------------------------------------------------------------------------ T5 text intra-attention
_TIA_PER_LAYER = ("msg", "attn", "u", "r", "o", "xr")


def _tia_saved(x, saved, layers):
    """The per-layer state ops.text_intra_backward expects, from what the operator returned: six tensors per layer, then the
    input of every layer but the first (the first layer's is the operator's input)."""
    R, L, E = x.shape
    n = len(_TIA_PER_LAYER)
    xs = [x.reshape(R * L, E)] + list(saved[n * layers:])
    return [dict(zip(_TIA_PER_LAYER, saved[n * l: n * (l + 1)]), x=xs[l]) for l in range(layers)]


@custom_op("tag::text_intra", mutates_args=())
def text_intra(x: Tensor, text_len: Tensor, pe: Tensor, params: List[Tensor], layers: int, drop_p: float,
               seed: int) -> Tuple[Tensor, Tensor, List[Tensor]]:
    """IntraAttention behind its embedding (models/text_encoder.py:213-237): x (R, L, E) embedded tokens, text_len (R) int64,
    pe (>= L, E) positions, params = conv_gru's [reset_gate.weight, reset_gate.bias, update_gate.weight, update_gate.bias,
    out_gate.weight, out_gate.bias], the SAME cell applied ``layers`` >= 1 times -> token_emb (R, L, E), seq_emb (R, E) and the
    saved state (message, attn, u, r, o, x * r per layer, then the input of every layer but the first).  drop_p > 0 (the
    caller passes 0 in eval mode): two independent dropouts behind the positions per layer, keep masks of
    ops.text_intra_dropout_seeds(seed, layers)."""
    tok, seq, saved = ops.text_intra_forward(x, text_len, pe, *params, layers, True, drop_p, seed)
    return tok, seq, [sv[k] for sv in saved for k in _TIA_PER_LAYER] + [sv["x"] for sv in saved[1:]]


@text_intra.register_fake
def _(x, text_len, pe, params, layers, drop_p, seed):
    R, L, E = x.shape
    per = [x.new_empty(R * L, E), x.new_empty(R, L, L)] + [x.new_empty(R * L, E) for _ in range(4)]
    return (x.new_empty(R, L, E), x.new_empty(R, E),
            [torch.empty_like(t) for _ in range(layers) for t in per] + [x.new_empty(R * L, E) for _ in range(layers - 1)])


@custom_op("tag::text_intra_backward", mutates_args=())
def text_intra_backward(dtok: Optional[Tensor], dseq: Optional[Tensor], x: Tensor, text_len: Tensor, pe: Tensor,
                        saved: List[Tensor], params: List[Tensor], layers: int, drop_p: float, seed: int, need: List[bool],
                        need_dx: bool) -> List[Tensor]:
    """-> [dx] + one gradient per parameter; an entry that is not needed (need[i] / need_dx False) is an empty tensor."""
    sv = _tia_saved(x, saved, layers)
    dx, g = ops.text_intra_backward(dtok, dseq, text_len, pe, sv, params[0], params[2], params[4], drop_p, seed, need=list(need),
                                    need_dx=need_dx)
    none = lambda: x.new_empty(0)                                                    # noqa: E731
    return [dx if dx is not None else none()] + [t if t is not None else none() for t in g]


@text_intra_backward.register_fake
def _(dtok, dseq, x, text_len, pe, saved, params, layers, drop_p, seed, need, need_dx):
    return [torch.empty_like(x) if need_dx else x.new_empty(0)] + [torch.empty_like(p) if n else x.new_empty(0)
                                                                    for p, n in zip(params, need)]


def _tia_setup(ctx, inputs, output):
    x, text_len, pe, params, layers, drop_p, seed = inputs
    _, _, saved = output
    ctx.save_for_backward(x, text_len, pe, *saved, *params)
    ctx.meta = (layers, drop_p, seed, len(saved))
    ctx.need = [bool(p.requires_grad) for p in params]
    ctx.need_dx = bool(x.requires_grad)


def _tia_backward(ctx, dtok, dseq, _dsaved):
    layers, drop_p, seed, ns = ctx.meta
    x, text_len, pe = ctx.saved_tensors[:3]
    saved, params = list(ctx.saved_tensors[3:3 + ns]), list(ctx.saved_tensors[3 + ns:])
    if dtok is None and dseq is None:
        return (None,) * 7
    if dtok is not None:
        dtok = dtok.contiguous()
    if dseq is not None:
        dseq = dseq.contiguous()
    g = torch.ops.tag.text_intra_backward(dtok, dseq, x, text_len, pe, saved, params, layers, drop_p, seed, ctx.need, ctx.need_dx)
    return (g[0] if ctx.need_dx else None, None, None, [t if n else None for t, n in zip(g[1:], ctx.need)], None, None, None)


register_autograd("tag::text_intra", _tia_backward, setup_context=_tia_setup)


# ------------------------------------------------------------------------------------------------ T6 LAION-CLAP text tower
_TCL_HEAD, _TCL_LAYER = _dispatch.TEXT_CLAP_SAVED_HEAD, _dispatch.TEXT_CLAP_SAVED_LAYER


def _tcl_saved(saved, params, layers):
    """The state ops.text_clap_backward expects, from what the operator returned: seven tensors of the embedding block and the
    tail, then eleven per layer; the packed q|k|v weights are formed again from the three parameters."""
    nh, nl = len(_TCL_HEAD), len(_TCL_LAYER)
    st = dict(zip(_TCL_HEAD, saved[:nh]))
    st["layers"] = []
    for l in range(layers):
        sv = dict(zip(_TCL_LAYER, saved[nh + nl * l: nh + nl * (l + 1)]))
        b = 5 + 16 * l
        sv["wqkv"] = torch.cat((params[b], params[b + 2], params[b + 4]), 0)
        st["layers"].append(sv)
    return st


@custom_op("tag::text_clap", mutates_args=())
def text_clap(input_ids: Tensor, attention_mask: Tensor, params: List[Tensor], heads: int, eps: float, pad_id: int,
              p_hidden: float, p_attn: float, seed: int, need_grad: bool) -> Tuple[Tensor, Tensor, List[Tensor]]:
    """LaionClapEncoder.forward (models/text_encoder.py:320-327): input_ids, attention_mask (R, L) int64, params in the order of
    ops.text_clap_param_names -> token_emb (R, L, P), seq_emb (R, P) and the saved state (ops.TEXT_CLAP_SAVED_HEAD, then
    ops.TEXT_CLAP_SAVED_LAYER per layer; empty when need_grad is False: a frozen tower, eval, no_grad).  p_hidden / p_attn > 0
    (the caller passes 0 in eval mode): Hugging Face's four dropout sites, keep masks of ops.text_clap_dropout_seeds(seed, layers)."""
    tok, seq, st = ops.text_clap_forward(input_ids, attention_mask, list(params), heads, eps, pad_id, need_grad, p_hidden, p_attn, seed)
    if st is None:
        return tok, seq, []
    st = dict(st, seq_raw=st["seq_raw"].clone())                  # token_emb and seq_raw are two views of one buffer
    return tok, seq, [st[k] for k in _TCL_HEAD] + [sv[k] for sv in st["layers"] for k in _TCL_LAYER]


def _tcl_dims(input_ids, params, heads):
    R, L = input_ids.shape
    D, I, P = params[0].shape[1], params[5 + 10].shape[0], params[-4].shape[0]
    return R, L, D, I, P


@text_clap.register_fake
def _(input_ids, attention_mask, params, heads, eps, pad_id, p_hidden, p_attn, seed, need_grad):
    R, L, D, I, P = _tcl_dims(input_ids, params, heads)
    M = R * L
    x = params[0]
    out = (x.new_empty(R, L, P), x.new_empty(R, P))
    if not need_grad:
        return (*out, [])
    head = [input_ids.new_empty(M), input_ids.new_empty(R), x.new_empty(M, D), x.new_empty(M), x.new_empty(M + R, D),
            x.new_empty(M + R, P), x.new_empty(R, P)]
    per = [x.new_empty(M, D), x.new_empty(M, 3 * D), x.new_empty(R, heads, L, L), x.new_empty(M, D), x.new_empty(M, D), x.new_empty(M),
           x.new_empty(M, D), x.new_empty(M, I), x.new_empty(M, I), x.new_empty(M, D), x.new_empty(M)]
    layers = _dispatch.text_clap_layers(len(params))
    return (*out, head + [torch.empty_like(t) for _ in range(layers) for t in per])


@custom_op("tag::text_clap_backward", mutates_args=())
def text_clap_backward(dtok: Optional[Tensor], dseq: Optional[Tensor], input_ids: Tensor, saved: List[Tensor], params: List[Tensor],
                       heads: int, pad_id: int, p_hidden: float, p_attn: float, seed: int, need: List[bool]) -> List[Tensor]:
    """-> one gradient per parameter; an entry that is not needed (need[i] False) is an empty tensor."""
    st = _tcl_saved(list(saved), list(params), _dispatch.text_clap_layers(len(params)))
    g = ops.text_clap_backward(dtok, dseq, input_ids, st, list(params), heads, pad_id, p_hidden, p_attn, seed, need=list(need))
    return [t.view(p.shape) if t is not None else p.new_empty(0) for t, p in zip(g, params)]


@text_clap_backward.register_fake
def _(dtok, dseq, input_ids, saved, params, heads, pad_id, p_hidden, p_attn, seed, need):
    return [torch.empty_like(p) if n else p.new_empty(0) for p, n in zip(params, need)]


def _tcl_setup(ctx, inputs, output):
    input_ids, _, params, heads, _, pad_id, p_hidden, p_attn, seed, _ = inputs
    _, _, saved = output
    ctx.save_for_backward(input_ids, *saved, *params)
    ctx.meta = (heads, pad_id, p_hidden, p_attn, seed, len(saved))
    ctx.need = [bool(p.requires_grad) for p in params]


def _tcl_backward(ctx, dtok, dseq, _dsaved):
    heads, pad_id, p_hidden, p_attn, seed, ns = ctx.meta
    input_ids = ctx.saved_tensors[0]
    saved, params = list(ctx.saved_tensors[1:1 + ns]), list(ctx.saved_tensors[1 + ns:])
    if (dtok is None and dseq is None) or not any(ctx.need):
        return (None,) * 10
    if ns == 0:
        raise RuntimeError("tag::text_clap ran with need_grad = False: nothing was saved for a backward pass")
    if dtok is not None:
        dtok = dtok.contiguous()
    if dseq is not None:
        dseq = dseq.contiguous()
    g = torch.ops.tag.text_clap_backward(dtok, dseq, input_ids, saved, params, heads, pad_id, p_hidden, p_attn, seed, ctx.need)
    return (None, None, [t if n else None for t, n in zip(g, ctx.need)], None, None, None, None, None, None, None)


register_autograd("tag::text_clap", _tcl_backward, setup_context=_tcl_setup)


# ------------------------------------------------------------------------------------------------ T7 BERT / SentenceBert
_TBT_HEAD = _dispatch.TEXT_BERT_SAVED_HEAD


def _tbt_saved(saved, params, layers):
    """The state ops.text_bert_backward expects, from what the operator returned: four tensors of the embedding block and the
    pooling, then eleven per layer; the packed q|k|v weights are formed again from the three parameters."""
    nh, nl = len(_TBT_HEAD), len(_TCL_LAYER)
    st = dict(zip(_TBT_HEAD, saved[:nh]))
    st["layers"] = []
    for l in range(layers):
        sv = dict(zip(_TCL_LAYER, saved[nh + nl * l: nh + nl * (l + 1)]))
        b = 5 + 16 * l
        sv["wqkv"] = torch.cat((params[b], params[b + 2], params[b + 4]), 0)
        st["layers"].append(sv)
    return st


@custom_op("tag::text_bert", mutates_args=())
def text_bert(input_ids: Tensor, token_type_ids: Optional[Tensor], attention_mask: Tensor, params: List[Tensor], heads: int,
              eps: float, pad_id: int, pool_mode: int, norm: int, p_hidden: float, p_attn: float, seed: int,
              need_grad: bool) -> Tuple[Tensor, Tensor, List[Tensor]]:
    """Bert.forward / SentenceBert.forward (models/text_encoder.py:281-308): input_ids, attention_mask (R, L) int64,
    token_type_ids the same or None, params in the order of ops.text_bert_param_names -> token_emb (R, L, D) the last hidden state,
    seq_emb (R, D) pooled (0 [CLS], 1 masked mean) and normalised (0 none, 1 F.normalize, 2 the retrieval model's, forward-only),
    and the saved state (ops.TEXT_BERT_SAVED_HEAD, then ops.TEXT_CLAP_SAVED_LAYER per layer; empty when need_grad is False)."""
    tok, seq, st = ops.text_bert_forward(input_ids, token_type_ids, attention_mask, list(params), heads, eps, pad_id, pool_mode, norm,
                                         need_grad, p_hidden, p_attn, seed)
    if st is None:
        return tok, seq, []
    if st["raw"] is seq:
        st = dict(st, raw=seq.clone())                            # an operator may not return one tensor twice
    return tok, seq, [st[k] for k in _TBT_HEAD] + [sv[k] for sv in st["layers"] for k in _TCL_LAYER]


@text_bert.register_fake
def _(input_ids, token_type_ids, attention_mask, params, heads, eps, pad_id, pool_mode, norm, p_hidden, p_attn, seed, need_grad):
    R, L = input_ids.shape
    D, I = params[0].shape[1], params[5 + 10].shape[0]
    M = R * L
    x = params[0]
    out = (x.new_empty(R, L, D), x.new_empty(R, D))
    if not need_grad:
        return (*out, [])
    head = [input_ids.new_empty(R), x.new_empty(M, D), x.new_empty(M), x.new_empty(R, D)]
    per = [x.new_empty(M, D), x.new_empty(M, 3 * D), x.new_empty(R, heads, L, L), x.new_empty(M, D), x.new_empty(M, D), x.new_empty(M),
           x.new_empty(M, D), x.new_empty(M, I), x.new_empty(M, I), x.new_empty(M, D), x.new_empty(M)]
    layers, _ = _dispatch.text_bert_layers(len(params))
    return (*out, head + [torch.empty_like(t) for _ in range(layers) for t in per])


@custom_op("tag::text_bert_backward", mutates_args=())
def text_bert_backward(dtok: Optional[Tensor], dseq: Optional[Tensor], input_ids: Tensor, token_type_ids: Optional[Tensor],
                       saved: List[Tensor], params: List[Tensor], heads: int, pad_id: int, pool_mode: int, norm: int,
                       p_hidden: float, p_attn: float, seed: int, need: List[bool]) -> List[Tensor]:
    """-> one gradient per parameter; an entry that is not needed (need[i] False, the pooler's always) is an empty tensor."""
    st = _tbt_saved(list(saved), list(params), _dispatch.text_bert_layers(len(params))[0])
    g = ops.text_bert_backward(dtok, dseq, input_ids, token_type_ids, st, list(params), heads, pad_id, pool_mode, norm, p_hidden,
                               p_attn, seed, need=list(need))
    return [t.view(p.shape) if t is not None else p.new_empty(0) for t, p in zip(g, params)]


@text_bert_backward.register_fake
def _(dtok, dseq, input_ids, token_type_ids, saved, params, heads, pad_id, pool_mode, norm, p_hidden, p_attn, seed, need):
    return [torch.empty_like(p) if n else p.new_empty(0) for p, n in zip(params, need)]


def _tbt_setup(ctx, inputs, output):
    input_ids, type_ids, _, params, heads, _, pad_id, pool_mode, norm, p_hidden, p_attn, seed, _ = inputs
    _, _, saved = output
    ctx.has_types = type_ids is not None
    ctx.save_for_backward(input_ids, *([type_ids] if ctx.has_types else []), *saved, *params)
    ctx.meta = (heads, pad_id, pool_mode, norm, p_hidden, p_attn, seed, len(saved))
    pooler = _dispatch.text_bert_layers(len(params))[1]
    ctx.need = [bool(p.requires_grad) and not (pooler and i >= len(params) - 2) for i, p in enumerate(params)]


def _tbt_backward(ctx, dtok, dseq, _dsaved):
    heads, pad_id, pool_mode, norm, p_hidden, p_attn, seed, ns = ctx.meta
    t = list(ctx.saved_tensors)
    input_ids = t.pop(0)
    type_ids = t.pop(0) if ctx.has_types else None
    saved, params = t[:ns], t[ns:]
    if (dtok is None and dseq is None) or not any(ctx.need):
        return (None,) * 13
    if ns == 0:
        raise RuntimeError("tag::text_bert ran with need_grad = False: nothing was saved for a backward pass")
    if dtok is not None:
        dtok = dtok.contiguous()
    if dseq is not None:
        dseq = dseq.contiguous()
    g = torch.ops.tag.text_bert_backward(dtok, dseq, input_ids, type_ids, saved, params, heads, pad_id, pool_mode, norm, p_hidden,
                                         p_attn, seed, ctx.need)
    return (None, None, None, [t if n else None for t, n in zip(g, ctx.need)], *([None] * 9))


register_autograd("tag::text_bert", _tbt_backward, setup_context=_tbt_setup)


# ------------------------------------------------------------------------------------------------ M1/M2 frame x phrase heads
@custom_op("tag::frame_match", mutates_args=())
def frame_match(audio: Tensor, text: Tensor, kind: int, l2norm: bool, scale: bool) -> Tensor:
    """kind 0 = match.DotProduct (sigmoid(a.t [/sqrt D]).clamp(1e-7,1)), 1 = match.ExpNegL2 (exp(-||a - t||)): (B,T,D),(B,D) -> (B,T)."""
    return ops.match_forward(audio, text, kind, l2norm, scale)


@frame_match.register_fake
def _(audio, text, kind, l2norm, scale):
    return audio.new_empty(audio.shape[0], audio.shape[1])


@custom_op("tag::frame_match_backward", mutates_args=())
def frame_match_backward(audio: Tensor, text: Tensor, sim: Tensor, dsim: Tensor, kind: int, l2norm: bool,
                         scale: bool) -> Tuple[Tensor, Tensor]:
    return ops.match_backward(audio, text, sim, dsim, kind, l2norm, scale)


@frame_match_backward.register_fake
def _(audio, text, sim, dsim, kind, l2norm, scale):
    return torch.empty_like(audio), torch.empty_like(text)


def _match_setup(ctx, inputs, output):
    audio, text, kind, l2norm, scale = inputs
    ctx.save_for_backward(audio, text, output)
    ctx.cfg = (kind, l2norm, scale)


def _match_backward(ctx, dsim):
    audio, text, sim = ctx.saved_tensors
    da, dt = torch.ops.tag.frame_match_backward(audio, text, sim, dsim, *ctx.cfg)
    return da, dt, None, None, None


register_autograd("tag::frame_match", _match_backward, setup_context=_match_setup)


# ------------------------------------------------------------------------------------------------ M3 align.DotProduct
@custom_op("tag::align_dot", mutates_args=())
def align_dot(audio: Tensor, text: Tensor, l2norm: bool, scaled: bool) -> Tensor:
    """align.DotProduct: (B,T,D),(B,N,D) -> (B,B,T,N) on the MFMA GEMM with the sigmoid/clamp/scatter epilogue."""
    return ops.align_dot(audio, text, l2norm, scaled)


@align_dot.register_fake
def _(audio, text, l2norm, scaled):
    B, T, _ = audio.shape
    return audio.new_empty(B, B, T, text.shape[1])


@custom_op("tag::align_dot_backward", mutates_args=())
def align_dot_backward(audio: Tensor, text: Tensor, out: Tensor, dout: Tensor, l2norm: bool, scaled: bool) -> Tuple[Tensor, Tensor]:
    return ops.align_dot_backward(audio, text, out, dout, l2norm, scaled)


@align_dot_backward.register_fake
def _(audio, text, out, dout, l2norm, scaled):
    return torch.empty_like(audio), torch.empty_like(text)


def _align_setup(ctx, inputs, output):
    audio, text, l2norm, scaled = inputs
    ctx.save_for_backward(audio, text, output)
    ctx.cfg = (l2norm, scaled)


def _align_backward(ctx, dout):
    audio, text, out = ctx.saved_tensors
    da, dt = torch.ops.tag.align_dot_backward(audio, text, out, dout, *ctx.cfg)
    return da, dt, None, None


register_autograd("tag::align_dot", _align_backward, setup_context=_align_setup)


# ------------------------------------------------------------------------------------------------ align.ExpNegL2
@custom_op("tag::align_expnegl2", mutates_args=())
def align_expnegl2(audio: Tensor, text: Tensor) -> Tensor:
    """align.ExpNegL2: (B,T,D),(B,N,D) -> (B,B,T,N) = exp(-||normalize(audio) - normalize(text)||), tiled VALU kernel."""
    return ops.align_expnegl2(audio, text)


@align_expnegl2.register_fake
def _(audio, text):
    B, T, _ = audio.shape
    return audio.new_empty(B, B, T, text.shape[1])


@custom_op("tag::align_expnegl2_backward", mutates_args=())
def align_expnegl2_backward(audio: Tensor, text: Tensor, dout: Tensor) -> Tuple[Tensor, Tensor]:
    return ops.align_expnegl2_backward(audio, text, dout)


@align_expnegl2_backward.register_fake
def _(audio, text, dout):
    return torch.empty_like(audio), torch.empty_like(text)


def _expnegl2_setup(ctx, inputs, output):
    audio, text = inputs
    ctx.save_for_backward(audio, text)


def _expnegl2_backward(ctx, dout):
    audio, text = ctx.saved_tensors
    return torch.ops.tag.align_expnegl2_backward(audio, text, dout)


register_autograd("tag::align_expnegl2", _expnegl2_backward, setup_context=_expnegl2_setup)


# ------------------------------------------------------------------------------------------------ L1 frame BCE
@custom_op("tag::frame_bce", mutates_args=())
def frame_bce(frame_sim: Tensor, label: Tensor, length: Tensor, Tt: int) -> Tensor:
    """FrameBceLoss over the first Tt frames, masked by clamp(length, 1, Tt): -> 0-dim loss."""
    return ops.frame_bce_forward(frame_sim, label, length, Tt)


@frame_bce.register_fake
def _(frame_sim, label, length, Tt):
    return frame_sim.new_empty(())


@custom_op("tag::frame_bce_backward", mutates_args=())
def frame_bce_backward(frame_sim: Tensor, label: Tensor, length: Tensor, Tt: int, dloss: Tensor) -> Tensor:
    return ops.frame_bce_backward(frame_sim, label, length, Tt, dloss)


@frame_bce_backward.register_fake
def _(frame_sim, label, length, Tt, dloss):
    return torch.empty_like(frame_sim)


def _bce_setup(ctx, inputs, output):
    frame_sim, label, length, Tt = inputs
    ctx.save_for_backward(frame_sim, label, length)
    ctx.Tt = Tt


def _bce_backward(ctx, dloss):
    frame_sim, label, length = ctx.saved_tensors
    return torch.ops.tag.frame_bce_backward(frame_sim, label, length, ctx.Tt, dloss), None, None, None


register_autograd("tag::frame_bce", _bce_backward, setup_context=_bce_setup)


# ------------------------------------------------------------------------------------------------ AudioTagging head + masked BCE
@custom_op("tag::tagging_head", mutates_args=())
def tagging_head(embedding: Tensor, weight: Tensor, bias: Tensor, length: Tensor, mode: int) -> Tuple[Tensor, Tensor, Tensor]:
    """AudioTagging.forward below the encoder (models/audio_text_model.py:441-453): sigmoid(embedding @ weight^T + bias)
    (B,T,C), its pooling over the frames < length[b] (mode: ops.POOL_MODES) (B,C), and aux (B,C) for the backward."""
    return ops.tagging_head_forward(embedding, weight, bias, length, mode)


@tagging_head.register_fake
def _(embedding, weight, bias, length, mode):
    B, T, _ = embedding.shape
    C = weight.shape[0]
    return embedding.new_empty(B, T, C), embedding.new_empty(B, C), embedding.new_empty(B, C)


@custom_op("tag::tagging_head_backward", mutates_args=())
def tagging_head_backward(embedding: Tensor, weight: Tensor, prob: Tensor, clip: Tensor, aux: Tensor, length: Tensor, mode: int,
                          dprob: Optional[Tensor], dclip: Optional[Tensor]) -> Tuple[Tensor, Tensor, Tensor]:
    """-> (dembedding, dweight, dbias)."""
    return ops.tagging_head_backward(embedding.contiguous(), weight.contiguous(), prob, clip, aux, length, mode, dprob, dclip)


@tagging_head_backward.register_fake
def _(embedding, weight, prob, clip, aux, length, mode, dprob, dclip):
    return torch.empty_like(embedding), torch.empty_like(weight), weight.new_empty(weight.shape[0])


def _taghead_setup(ctx, inputs, output):
    embedding, weight, _bias, length, mode = inputs
    prob, clip, aux = output
    ctx.save_for_backward(embedding, weight, prob, clip, aux, length)
    ctx.mode = mode
    ctx.set_materialize_grads(False)


def _taghead_backward(ctx, dprob, dclip, _daux):
    embedding, weight, prob, clip, aux, length = ctx.saved_tensors
    if dprob is None and dclip is None:
        return None, None, None, None, None
    dx, dw, db = torch.ops.tag.tagging_head_backward(embedding, weight, prob, clip, aux, length, ctx.mode, dprob, dclip)
    return dx, dw, db, None, None


register_autograd("tag::tagging_head", _taghead_backward, setup_context=_taghead_setup)


@custom_op("tag::masked_frame_bce", mutates_args=())
def masked_frame_bce(frame_sim: Tensor, label: Tensor, length: Tensor, cls_mask: Optional[Tensor]) -> Tensor:
    """MaskedFrameBceLoss (losses.py:157-170) over frame_sim / label (B,Tt,C) (views truncated in time are read in place),
    frames < clamp(length, 1, Tt), classes weighted by cls_mask (B,C) (None = all ones): -> 0-dim loss."""
    return ops.masked_frame_bce_forward(frame_sim, label, length, cls_mask)


@masked_frame_bce.register_fake
def _(frame_sim, label, length, cls_mask):
    return frame_sim.new_empty(())


@custom_op("tag::masked_frame_bce_backward", mutates_args=())
def masked_frame_bce_backward(frame_sim: Tensor, label: Tensor, length: Tensor, cls_mask: Optional[Tensor],
                              dloss: Tensor) -> Tensor:
    return ops.masked_frame_bce_backward(frame_sim, label, length, cls_mask, dloss)


@masked_frame_bce_backward.register_fake
def _(frame_sim, label, length, cls_mask, dloss):
    return frame_sim.new_empty(frame_sim.shape)


def _mbce_setup(ctx, inputs, output):
    frame_sim, label, length, cls_mask = inputs
    ctx.save_for_backward(frame_sim, label, length, cls_mask)


def _mbce_backward(ctx, dloss):
    frame_sim, label, length, cls_mask = ctx.saved_tensors
    return torch.ops.tag.masked_frame_bce_backward(frame_sim, label, length, cls_mask, dloss), None, None, None


register_autograd("tag::masked_frame_bce", _mbce_backward, setup_context=_mbce_setup)


# ------------------------------------------------------------------------------------------------ contrastive objectives
# ``tag::infonce`` / ``tag::triplet`` / ``tag::milnce`` return the 0-dim loss alone.  Their forward kernel also fills a small
# workspace (row / column log-sum-exp, or argmax) that makes the backward ONE elementwise launch; it reaches ``setup_context``
# through a one-slot hand-over, like the saved state of the encoder operators below, and the backward operator takes it as an
# optional argument.  A backward that was traced (torch.compile / AOTAutograd: fake tensors, no hand-over) passes None and the
# backward refills the workspace with one extra forward launch: the same result either way.
_CONTRASTIVE_WS = [None]


def _hand_over(loss, ws):
    _CONTRASTIVE_WS[0] = (ws, loss.data_ptr())
    return loss


def _take_ws(ctx, output):
    """The workspace of the forward that produced ``output`` -- not a leftover of an earlier forward whose setup_context never
    ran (no input needed a gradient), and nothing at all for a traced (fake) output."""
    slot, _CONTRASTIVE_WS[0] = _CONTRASTIVE_WS[0], None
    ctx.ws = slot[0] if slot is not None and type(output) is Tensor and output.data_ptr() == slot[1] else None


@custom_op("tag::infonce", mutates_args=())
def infonce(sim: Tensor, tau: float) -> Tensor:
    """InfoNceLoss (losses.py:267-281) on the (n,n) clip-versus-caption matrix: symmetric cross-entropy of sim / tau against
    the diagonal -> 0-dim loss."""
    return _hand_over(*ops.infonce_forward(sim, tau))


@infonce.register_fake
def _(sim, tau):
    return sim.new_empty(())


@custom_op("tag::infonce_backward", mutates_args=())
def infonce_backward(sim: Tensor, tau: float, dloss: Tensor, ws: Optional[Tensor]) -> Tensor:
    return ops.infonce_backward(sim, tau, dloss, ws)


@infonce_backward.register_fake
def _(sim, tau, dloss, ws):
    return sim.new_empty(sim.shape)


def _infonce_setup(ctx, inputs, output):
    sim, ctx.tau = inputs
    ctx.save_for_backward(sim)
    _take_ws(ctx, output)


def _infonce_backward(ctx, dloss):
    (sim,) = ctx.saved_tensors
    return torch.ops.tag.infonce_backward(sim, ctx.tau, dloss, ctx.ws), None


register_autograd("tag::infonce", _infonce_backward, setup_context=_infonce_setup)


@custom_op("tag::triplet", mutates_args=())
def triplet(sim: Tensor, mode: int, margin: float, s_index: Optional[Tensor], a_index: Optional[Tensor]) -> Tensor:
    """Max (mode 0) / Weighted (1) / Random (2) TripletLoss (losses.py:285-417) on the (n,n) matrix -> 0-dim loss.  s_index /
    a_index: device int32 (n) draws of the random mode (ops.TRIPLET_MODES names the modes)."""
    return _hand_over(*ops.triplet_forward(sim, mode, margin, s_index, a_index))


@triplet.register_fake
def _(sim, mode, margin, s_index, a_index):
    return sim.new_empty(())


@custom_op("tag::triplet_backward", mutates_args=())
def triplet_backward(sim: Tensor, mode: int, margin: float, s_index: Optional[Tensor], a_index: Optional[Tensor], dloss: Tensor,
                     ws: Optional[Tensor]) -> Tensor:
    return ops.triplet_backward(sim, mode, margin, s_index, a_index, dloss, ws)


@triplet_backward.register_fake
def _(sim, mode, margin, s_index, a_index, dloss, ws):
    return sim.new_empty(sim.shape)


def _triplet_setup(ctx, inputs, output):
    sim, ctx.mode, ctx.margin, s_index, a_index = inputs
    ctx.save_for_backward(sim, s_index, a_index)
    _take_ws(ctx, output)


def _triplet_backward(ctx, dloss):
    sim, s_index, a_index = ctx.saved_tensors
    return torch.ops.tag.triplet_backward(sim, ctx.mode, ctx.margin, s_index, a_index, dloss, ctx.ws), None, None, None, None


register_autograd("tag::triplet", _triplet_backward, setup_context=_triplet_setup)


@custom_op("tag::milnce", mutates_args=())
def milnce(clip_sim: Tensor, label: Tensor, tau: float) -> Tensor:
    """MilNceLoss (losses.py:46-56) on clip_sim / label (B,N): mean_b[LSE_n(c / tau) - LSE_n(c * l / tau)] -> 0-dim loss;
    label gets no gradient."""
    return _hand_over(*ops.milnce_forward(clip_sim, label, tau))


@milnce.register_fake
def _(clip_sim, label, tau):
    return clip_sim.new_empty(())


@custom_op("tag::milnce_backward", mutates_args=())
def milnce_backward(clip_sim: Tensor, label: Tensor, tau: float, dloss: Tensor, ws: Optional[Tensor]) -> Tensor:
    return ops.milnce_backward(clip_sim, label, tau, dloss, ws)


@milnce_backward.register_fake
def _(clip_sim, label, tau, dloss, ws):
    return clip_sim.new_empty(clip_sim.shape)


def _milnce_setup(ctx, inputs, output):
    clip_sim, label, ctx.tau = inputs
    ctx.save_for_backward(clip_sim, label)
    _take_ws(ctx, output)


def _milnce_backward(ctx, dloss):
    clip_sim, label = ctx.saved_tensors
    return torch.ops.tag.milnce_backward(clip_sim, label, ctx.tau, dloss, ctx.ws), None, None


register_autograd("tag::milnce", _milnce_backward, setup_context=_milnce_setup)


# ------------------------------------------------------------------------------------------------ clip-level BCE objectives
@custom_op("tag::clip_bce", mutates_args=())
def clip_bce(clip_sim: Tensor, label: Tensor, aux: Optional[Tensor], mode: int, c0: float, c1: float, c2: float) -> Tensor:
    """Focal (mode 0) / FreqWeight (1) / Symmetric (2) / OriginSymmetric (3) / PriorAdjusted (4) ClipBceLoss
    (losses.py:59-143) on clip_sim / label (B,N) -> 0-dim loss.  aux (B,N): the weight of mode 1, the prior of mode 4
    (ops.CLIP_BCE_MODES names the modes; include/tag_hip.h lists what c0, c1, c2 mean in each)."""
    return ops.clip_bce_forward(clip_sim, label, aux, mode, c0, c1, c2)


@clip_bce.register_fake
def _(clip_sim, label, aux, mode, c0, c1, c2):
    return clip_sim.new_empty(())


@custom_op("tag::clip_bce_backward", mutates_args=())
def clip_bce_backward(clip_sim: Tensor, label: Tensor, aux: Optional[Tensor], mode: int, c0: float, c1: float, c2: float,
                      dloss: Tensor) -> Tensor:
    return ops.clip_bce_backward(clip_sim, label, aux, mode, c0, c1, c2, dloss)


@clip_bce_backward.register_fake
def _(clip_sim, label, aux, mode, c0, c1, c2, dloss):
    return clip_sim.new_empty(clip_sim.shape)


def _clip_bce_setup(ctx, inputs, output):
    clip_sim, label, aux, ctx.mode, ctx.c0, ctx.c1, ctx.c2 = inputs
    ctx.has_aux = aux is not None
    ctx.save_for_backward(clip_sim, label, *([aux] if ctx.has_aux else []))


def _clip_bce_backward(ctx, dloss):
    clip_sim, label = ctx.saved_tensors[:2]
    aux = ctx.saved_tensors[2] if ctx.has_aux else None
    dclip = torch.ops.tag.clip_bce_backward(clip_sim, label, aux, ctx.mode, ctx.c0, ctx.c1, ctx.c2, dloss)
    return dclip, None, None, None, None, None, None


register_autograd("tag::clip_bce", _clip_bce_backward, setup_context=_clip_bce_setup)


# ------------------------------------------------------------------------------------------------ the fused audio encoders
# ``tag::cnn8rnn_encoder`` / ``tag::crnn_encoder``: log-mel -> conv stack -> (fc1) -> BiGRU as ONE operator each (rows F1-F3,
# A1-A4), what models/audio_encoder.py Cnn8Rnn.forward / CrnnEncoder.forward call -- the hot 97 % of the step goes through the
# operator registry like the heads do.  The operator wraps the engine of ops.py (ops.Cnn8RnnFunction / ops.CrnnFunction: the
# same forward / backward bodies, called with a plain context object): that engine keeps per-step state no functional
# operator could return cheaply (GBs of raw conv outputs saved for backward, dropout seeds, the direct-gradient sinks of the
# flat buffer, the weight-gradient side stream), so the saved state travels from the forward kernel to ``setup_context`` through
# a one-slot hand-over and the module (eps / momentum / dropout probabilities / frozen flags) is named by a token.  All four
# encoder operators go through _enc_forward / _enc_setup / _enc_backward; the early-fusion ones (``tag::cross_cnn8rnn`` /
# ``tag::cross_cdur``) pass their text terms ahead of the parameters and cut the gradient list apart again (_cross_backward).
# EAGER-ONLY: the fake kernels serve shape inference (opcheck, meta tensors); a backward traced by torch.compile / AOTAutograd has
# no saved state and raises a clear error (_enc_backward).  A second backward through one forward (retain_graph) raises its own.
import weakref

_ENC_MODULES = weakref.WeakValueDictionary()          # token -> nn.Module
_ENC_HANDOVER = [None]                                # saved state of the forward that just ran -> its setup_context


def encoder_token(mod) -> int:
    """Registers ``mod`` (Cnn8Rnn / CrnnEncoder) for the encoder operators and returns its token."""
    tok = id(mod)
    _ENC_MODULES[tok] = mod
    return tok


class _EncCtx:
    """What ops.Cnn8RnnFunction.forward / .backward expect of their ctx (``augment``: see ops.Cnn8RnnFunction)."""

    def __init__(self, needs, augment=None):
        self.needs_input_grad = needs
        self.saved = None
        self.augment = augment


def _enc_forward(engine, waveform, params, module_token, need_grad, augment=None, texts=()):
    """``texts``: the differentiable per-clip text terms of an early-fusion node, passed ahead of its parameters."""
    mod = _ENC_MODULES[module_token]
    ctx = _EncCtx((False, False) + tuple(bool(need_grad and t.requires_grad) for t in (*texts, *params)), augment)
    y = engine.forward(ctx, waveform, mod, *texts, *params)
    _ENC_HANDOVER[0] = (engine, ctx) if need_grad else None
    return y


def _enc_setup(ctx, inputs, output):
    ctx.enc, _ENC_HANDOVER[0] = _ENC_HANDOVER[0], None
    ctx.enc_consumed = False
    # backward returns one entry per argument of the CALL: the dispatcher drops trailing optional arguments left at their
    # default (None), while ``inputs`` here has them filled in
    n = len(inputs)
    while n > 4 and inputs[n - 1] is None:
        n -= 1
    ctx.n_args = n


def _enc_backward(ctx, dy):
    if ctx.enc is None:
        if getattr(ctx, "enc_consumed", False):
            raise RuntimeError("tag encoder operator: second backward through the same forward (retain_graph=True): the saved "
                               "activations (GBs of raw conv outputs) are released by the first backward -- run the forward again")
        raise RuntimeError("tag encoder operator: backward without saved state.  The operator is EAGER-ONLY: its saved state is "
                           "handed from the forward kernel to setup_context out of band, which torch.compile / AOTAutograd "
                           "tracing (fake tensors) cannot reproduce; call it in eager mode with need_grad=True under autograd")
    engine, ectx = ctx.enc
    ctx.enc = None
    ctx.enc_consumed = True
    grads = engine.backward(ectx, dy.contiguous())            # (None, None, *parameter gradients)
    return (None, list(grads[2:])) + (None,) * (ctx.n_args - 2)


def _cross_backward(ctx, dy):
    """_enc_backward of an early-fusion operator (waveform, texts, params, ...): the node's flat gradient list is cut into the
    six text terms and the parameters."""
    flat = _enc_backward(ctx, dy)[1]
    return (None, flat[:6], flat[6:]) + (None,) * (ctx.n_args - 3)


def _enc_fake_frames(mod, waveform):
    return (waveform.shape[1] // mod.hop_length + 1) // mod.downsample_ratio


@custom_op("tag::cnn8rnn_encoder", mutates_args=())
def cnn8rnn_encoder(waveform: Tensor, params: List[Tensor], module_token: int, need_grad: bool,
                    specaug_stripes: Optional[Tensor] = None, mixup_lambda: Optional[Tensor] = None) -> Tensor:
    """Cnn8Rnn.forward of models/audio_encoder.py:88-227: waveform (B,S) -> embedding (B, T', 512).  params in
    Cnn8Rnn._flat_params() order.  In train mode the BatchNorm running statistics of the MODULE named by the token are updated
    as nn.BatchNorm2d updates its buffers: module state, not operator arguments (torch.library refuses an autograd formula on an
    operator that declares mutated arguments).

    specaug_stripes: device int32 (B, n_time + n_freq, 2) [bgn, width] of SpecAugmentation.draw (the first n_time =
    module.spec_augmenter.time_dropper.stripes_num rows along frames); mixup_lambda: device fp32 (B,), B even -> embedding of
    B/2 clips (models/audio_encoder.py:192-200).  Both are applied as given: the module decides when (train mode)."""
    augment = None
    if specaug_stripes is not None or mixup_lambda is not None:
        mod = _ENC_MODULES[module_token]
        n_time = mod.spec_augmenter.time_dropper.stripes_num if specaug_stripes is not None else 0
        augment = (specaug_stripes, n_time, mixup_lambda)
    return _enc_forward(ops.Cnn8RnnFunction, waveform, params, module_token, need_grad, augment)


@cnn8rnn_encoder.register_fake
def _(waveform, params, module_token, need_grad, specaug_stripes=None, mixup_lambda=None):
    mod = _ENC_MODULES[module_token]
    B = waveform.shape[0] // 2 if mixup_lambda is not None else waveform.shape[0]
    return waveform.new_empty(B, _enc_fake_frames(mod, waveform), mod.embed_dim)


register_autograd("tag::cnn8rnn_encoder", _enc_backward, setup_context=_enc_setup)


@custom_op("tag::crnn_encoder", mutates_args=())
def crnn_encoder(waveform: Tensor, params: List[Tensor], module_token: int, need_grad: bool) -> Tensor:
    """CrnnEncoder.forward of models/audio_encoder.py:16-86: waveform (B,S) -> embedding (B, T', embed_dim)."""
    return _enc_forward(ops.CrnnFunction, waveform, params, module_token, need_grad)


@crnn_encoder.register_fake
def _(waveform, params, module_token, need_grad):
    mod = _ENC_MODULES[module_token]
    return waveform.new_empty(waveform.shape[0], _enc_fake_frames(mod, waveform), 2 * mod.gru.hidden_size)


register_autograd("tag::crnn_encoder", _enc_backward, setup_context=_enc_setup)


@custom_op("tag::cross_cnn8rnn", mutates_args=())
def cross_cnn8rnn(waveform: Tensor, texts: List[Tensor], params: List[Tensor], module_token: int, need_grad: bool,
                  specaug_stripes: Optional[Tensor] = None) -> Tensor:
    """CrossCnn8_Rnn.forward of models/audio_text_model.py:785-840 below its text encoder: waveform (B,S) -> frame_sim
    (B, T', 1) before the optional x4 upsampling.  texts = [conv_block1..4.fc_text(e), fc1_text(e), rnn_text(e)] (B, C);
    params in CrossCnn8_Rnn._flat_params() order.  BatchNorm running statistics: module state, as tag::cnn8rnn_encoder.
    specaug_stripes: as tag::cnn8rnn_encoder (no mixup: the reference's cannot run, see CrossCnn8_Rnn)."""
    augment = None
    if specaug_stripes is not None:
        augment = (specaug_stripes, _ENC_MODULES[module_token].spec_augmenter.time_dropper.stripes_num, None)
    return _enc_forward(ops.CrossCnn8RnnFunction, waveform, params, module_token, need_grad, augment, texts)


@cross_cnn8rnn.register_fake
def _(waveform, texts, params, module_token, need_grad, specaug_stripes=None):
    mod = _ENC_MODULES[module_token]
    return waveform.new_empty(waveform.shape[0], _enc_fake_frames(mod, waveform), 1)


register_autograd("tag::cross_cnn8rnn", _cross_backward, setup_context=_enc_setup)


@custom_op("tag::cross_cdur", mutates_args=())
def cross_cdur(waveform: Tensor, texts: List[Tensor], params: List[Tensor], module_token: int, need_grad: bool) -> Tensor:
    """CrossCDur.forward of models/audio_text_model.py:539-568 below its text encoder: waveform (B,S) -> frame_sim (B, T')
    before the optional x4 upsampling.  texts = [block1..5.fc_text(e), fc_text(e)] (B, C); params in
    CrossCDur._flat_params() order.  BatchNorm running statistics: module state, as tag::crnn_encoder."""
    return _enc_forward(ops.CrossCDurFunction, waveform, params, module_token, need_grad, texts=texts)


@cross_cdur.register_fake
def _(waveform, texts, params, module_token, need_grad):
    mod = _ENC_MODULES[module_token]
    return waveform.new_empty(waveform.shape[0], (waveform.shape[1] // mod.hop_length + 1) // mod.interpolate_ratio)


register_autograd("tag::cross_cdur", _cross_backward, setup_context=_enc_setup)


def stage_to_device(t, device, dtype):
    """A small host table (stripes, mixup lambda) -> ``device`` through pinned memory, non-blocking (a pageable host->device
    copy waits for the stream to drain: the host would stall mid-step, runner.py stages the lengths the same way)."""
    t = torch.as_tensor(t).to(dtype)
    if t.device == torch.device(device):
        return t.contiguous()
    if t.is_cuda:
        return t.to(device).contiguous()
    return t.contiguous().pin_memory().to(device, non_blocking=True)


def run_encoder(op, mod, waveform, params, *augment):
    """Front door of the two encoder modules: calls ``op`` with the caller's grad mode made visible to the engine (inside an
    operator grad mode is always off) and the module's token.  ``augment``: the trailing optional operator arguments
    (tag::cnn8rnn_encoder: specaug_stripes, mixup_lambda)."""
    need = torch.is_grad_enabled() and any(p.requires_grad for p in params)
    prev, engine._RECORDING = engine._RECORDING, torch.is_grad_enabled()
    try:
        return op(waveform, list(params), encoder_token(mod), need, *augment)
    finally:
        engine._RECORDING = prev
        # setup_context has taken the saved state by now; if it was skipped (the dispatcher decided that no input needs a
        # gradient) the slot must not keep GBs of activations alive until the next forward
        _ENC_HANDOVER[0] = None


# ------------------------------------------------------------------------------------------------ P1 segments
@custom_op("tag::segments", mutates_args=())
def segments(frame_sim: Tensor, thresholds: Tensor, window_size: int, n_connect: int) -> Tuple[Tensor, Tensor]:
    """binarize -> median filter -> connect clusters -> contiguous regions for every (clip, threshold):
    regions (B,NT,ceil(T/2),2) int64 rows [onset, offset), counts (B,NT) int32."""
    return ops.segments(frame_sim, thresholds, window_size, n_connect)


@segments.register_fake
def _(frame_sim, thresholds, window_size, n_connect):
    B, T = frame_sim.shape
    NT = thresholds.numel()
    return (torch.empty(B, NT, (T + 1) // 2, 2, device=frame_sim.device, dtype=torch.int64),
            torch.empty(B, NT, device=frame_sim.device, dtype=torch.int32))


OP_NAMES = ["logmel", "conv3x3", "conv3x3_dgrad", "conv3x3_wgrad", "conv3x3_bn_relu_pool", "conv3x3_bn_relu_pool_backward",
            "gru_bidir", "gru_bidir_backward", "embed_mean", "embed_mean_backward", "frame_match", "frame_match_backward",
            "align_dot", "align_dot_backward", "align_expnegl2", "align_expnegl2_backward", "frame_bce", "frame_bce_backward",
            "segments", "cnn8rnn_encoder", "crnn_encoder",
            "cross_cnn8rnn", "cross_cdur", "tagging_head", "tagging_head_backward", "masked_frame_bce",
            "masked_frame_bce_backward", "text_gru", "text_gru_backward", "text_selfattn", "text_selfattn_backward", "infonce",
            "infonce_backward", "triplet", "triplet_backward", "milnce", "milnce_backward", "text_intra", "text_intra_backward",
            "clip_bce", "clip_bce_backward", "text_clap", "text_clap_backward", "text_bert", "text_bert_backward"]
