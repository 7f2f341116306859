"""Learned text encoders: the word-embedding bag EmbeddingAgg, the recurrent RnnEncoder, the IntraAttention encoder with its
ConvGRUCell, the SelfAttention encoder, the BERT encoders Bert and SentenceBert and the trainable LAION-CLAP tower LaionClapEncoder (mirror
of models/text_encoder.py:14-43,61-327 in the reference)."""
import json
import math
import os
import warnings
from collections.abc import Mapping
from typing import Dict

import numpy as np
import torch
import torch.nn as nn

from .. import ops
from .. import torch_ops  # noqa: F401  (registers torch.ops.tag.*)
from .utils import init_weights


def _ids_to_device(text, table):
    """Token ids as the kernels take them (int64, contiguous, on the table's device).  Ids still on the host (what the
    reference's collate function hands over) are checked right here, and an id outside the table raises at once like
    nn.Embedding (models/text_encoder.py:39); device-resident ids are checked by the kernel, which can only raise a sticky
    flag: ops.check_async_errors() (StrongRunner.loss_value, segments_for_thresholds)."""
    text = torch.as_tensor(text)
    if not text.is_cuda and text.numel():
        lo, hi = int(text.min()), int(text.max())
        if lo < 0 or hi >= table.shape[0]:
            raise IndexError(f"index out of range in self: token ids span [{lo}, {hi}], the table has {table.shape[0]} rows")
    return text.long().to(table.device).contiguous()


class EmbeddingLayer(nn.Module):
    def __init__(self, vocab_size: int, embed_dim: int, pretrained_embedding: str = None,
                 freeze_embedding: bool = False):
        super().__init__()
        self.embed_dim = embed_dim
        self.core = nn.Embedding(vocab_size, embed_dim)
        self.apply(init_weights)
        if pretrained_embedding is not None:
            self.load_pretrained_embedding(pretrained_embedding, freeze_embedding)

    def load_pretrained_embedding(self, weight: str, freeze: bool = True):
        w = np.load(weight)
        if w.shape != tuple(self.core.weight.shape):
            raise AssertionError(f"expect embedding with shape {tuple(self.core.weight.shape)} but {w.shape} is given")
        self.core = nn.Embedding.from_pretrained(torch.as_tensor(w, dtype=torch.float), freeze)

    def forward(self, input_dict: Dict):
        """models/text_encoder.py:39-43: ``core(tokens.long())`` for token ids of any shape -> (*tokens.shape, embed_dim); every
        position is looked up, padding included (row 0 of the table).  The gather is the token_emb half of the fused
        gather + mean kernel (``tag_embed_mean_forward``; EmbeddingAgg uses both halves in one launch), its backward the
        deterministic gather of ``tag_embed_tokens_backward``."""
        table = self.core.weight
        text = _ids_to_device(input_dict["text"], table)
        shape = tuple(text.shape)
        ids = text.reshape(-1, shape[-1] if text.dim() > 1 else 1)
        if ids.numel() == 0:
            return table.new_zeros(*shape, table.shape[1])
        lens = torch.full((ids.shape[0],), ids.shape[1], dtype=torch.long, device=table.device)
        if ops.DIRECT_GRADS:
            _, tok = ops.EmbedMeanFunction.apply(table, ids, lens, True)
        else:
            _, tok = torch.ops.tag.embed_mean(table, ids, lens)
        return tok.view(*shape, table.shape[1])


class AttentionPooling(nn.Module):
    """Parameter container with the reference's layout (models/text_encoder.py:46-58): ``fc = Linear(emb_dim, 1)``."""

    def __init__(self, emb_dim):
        super().__init__()
        self.fc = nn.Linear(emb_dim, 1)

    def forward(self, x, lens):
        lens = torch.as_tensor(lens).long().to(x.device).contiguous()
        return ops.AttnPoolFunction.apply(x, lens, self.fc.weight, self.fc.bias)


class EmbeddingAgg(nn.Module):
    def __init__(self, vocab_size, embed_dim, pretrained_embedding: str = None, freeze_embedding: bool = False,
                 aggregation: str = "mean"):
        super().__init__()
        self.embedding = EmbeddingLayer(vocab_size, embed_dim, pretrained_embedding, freeze_embedding)
        self.embed_dim = self.embedding.embed_dim
        self.agg = aggregation
        if aggregation == "attention":
            self.attn = AttentionPooling(embed_dim)
        elif aggregation != "mean":
            raise Exception(f"{aggregation} not supported")            # as the reference (models/text_encoder.py:87-88)

    def forward(self, input_dict):
        table = self.embedding.core.weight
        dev = table.device
        text = _ids_to_device(input_dict["text"], table)
        lens = torch.as_tensor(input_dict["text_len"]).long().to(dev).contiguous()
        if ops.DIRECT_GRADS:          # StrongRunner: scatter the table gradient straight into its flat-gradient rows
            seq, tok = ops.EmbedMeanFunction.apply(table, text, lens, True)
        else:
            seq, tok = torch.ops.tag.embed_mean(table, text, lens)
        if self.agg == "attention":
            seq = self.attn(tok, lens)
        return {"token_emb": tok, "seq_emb": seq}


class RnnEncoder(nn.Module):
    """models/text_encoder.py:91-125: EmbeddingLayer -> nn.GRU(batch_first=True) over the tokens -> mean over the valid tokens.

    ``self.rnn`` is an nn.GRU that only HOLDS the parameters (state-dict keys ``rnn.weight_ih_l0`` ..., torch's default
    init); the recurrence runs in the row-local HIP kernels of csrc/text_gru.hip (``torch.ops.tag.text_gru``).  As in the
    reference the GRU runs UNPACKED over all L padded positions with h0 = 0: pad tokens are looked up like any other (row 0 of
    the table, which therefore receives gradient), the reverse direction starts at the padded end, ``token_emb`` is non-zero
    at padded positions, and the result of a row depends on the batch's padded L.  Only ``seq_emb`` masks: it is the mean
    of ``token_emb`` over the first ``text_len`` positions.

    ``rnn_type`` "GRU" is implemented; "RNN" and "LSTM" raise NotImplementedError (the HIP path has no eager fallback).
    Inter-layer dropout (train mode, num_layers > 1, dropout > 0) uses the project's counter-based keep mask
    (``tag_dropout_mask``), seeded from torch's global generator like the audio encoders' dropouts (ops.new_seed, decorrelated
    per rank by ops.SEED_RANK): the same rule as nn.GRU's, not torch's random stream."""

    def __init__(self, vocab_size, embed_dim, hidden_dim, num_layers, dropout, bidirectional, rnn_type, pooling="mean"):
        super().__init__()
        self.embedding = EmbeddingLayer(vocab_size, embed_dim)
        assert rnn_type in ("RNN", "GRU", "LSTM")
        if rnn_type != "GRU":
            raise NotImplementedError(f"RnnEncoder: rnn_type {rnn_type!r} has no HIP kernel (only \"GRU\"); there is no eager fallback")
        self.rnn = nn.GRU(input_size=embed_dim, hidden_size=hidden_dim, num_layers=num_layers, batch_first=True,
                          dropout=dropout, bidirectional=bidirectional)
        self.embed_dim = hidden_dim * (bidirectional + 1)
        self.pooling = pooling

    def forward(self, input_dict):
        x = self.embedding(input_dict)
        lead = tuple(x.shape[:-2])
        x = x.reshape(-1, x.shape[-2], x.shape[-1])
        text_len = torch.as_tensor(input_dict["text_len"]).long().to(x.device).reshape(-1).contiguous()
        rnn = self.rnn
        dirs = 2 if rnn.bidirectional else 1
        params = [getattr(rnn, n) for names in rnn._all_weights for n in names]
        p = float(rnn.dropout) if (self.training and rnn.num_layers > 1) else 0.0
        seed = ops.new_seed() if p > 0.0 else 0
        if ops.DIRECT_GRADS:
            token_emb, seq = ops.TextGruFunction.apply(x, text_len, dirs, rnn.num_layers, p, seed, *params)
        else:
            token_emb, seq, _ = torch.ops.tag.text_gru(x, text_len, params, dirs, rnn.num_layers, p, seed)
        out = {"token_emb": token_emb.view(*lead, *token_emb.shape[1:])}
        if self.pooling == "mean":
            out["seq_emb"] = seq.view(*lead, seq.shape[-1])
        return out


class PositionalEncoding(nn.Module):
    """Buffer container with the reference's layout (models/text_encoder.py:128-144): ``pe`` (1, max_len, d_model), sin on the
    even channels and cos on the odd ones; ``p`` is the dropout behind the positions.  The addition and the dropout run in
    ``tag_text_cls_pe_forward``."""

    def __init__(self, d_model, dropout, max_len=100):
        super().__init__()
        if d_model % 2:
            raise ValueError(f"PositionalEncoding: embed_dim {d_model} is odd; the sin/cos table is defined for even embed_dim only")
        self.p = float(dropout)
        pe = torch.zeros(max_len, d_model)
        position = torch.arange(0, max_len).unsqueeze(1)
        div_term = torch.exp(torch.arange(0, d_model, 2) * -(math.log(10000.0) / d_model))
        pe[:, 0::2] = torch.sin(position * div_term)
        pe[:, 1::2] = torch.cos(position * div_term)
        self.register_buffer("pe", pe.unsqueeze(0))


class ConvGRUCell(nn.Module):
    """Parameter container with the reference's layout and init (models/text_encoder.py:147-163): ``reset_gate``,
    ``update_gate``, ``out_gate`` = Linear(input_size + hidden_size, hidden_size), weights orthogonal, biases zero.  The
    arithmetic (u = sigmoid(W_u [m ; h] + b_u), r likewise, o = tanh(W_o [m ; h * r] + b_o), h <- h (1 - u) + o u) runs in
    ``torch.ops.tag.text_intra``."""

    def __init__(self, input_size, hidden_size, kernel_size=1):
        super().__init__()
        self.input_size = input_size
        self.hidden_size = hidden_size
        self.reset_gate = nn.Linear(input_size + hidden_size, hidden_size)
        self.update_gate = nn.Linear(input_size + hidden_size, hidden_size)
        self.out_gate = nn.Linear(input_size + hidden_size, hidden_size)
        for gate in (self.reset_gate, self.update_gate, self.out_gate):
            nn.init.orthogonal_(gate.weight)
        for gate in (self.reset_gate, self.update_gate, self.out_gate):
            nn.init.constant_(gate.bias, 0.)


class IntraAttention(nn.Module):
    """models/text_encoder.py:191-237: ``embedding`` (any module with ``.embed_dim`` whose forward returns (R, L, E) or a dict
    with "token_emb": EmbeddingLayer, EmbeddingAgg) -> ``num_layers`` times, with the SAME ``conv_gru`` cell (its gradients
    accumulate over the layers): an unscaled dot-product attention of the phrase over itself, whose message and the current
    state go through the cell -> ``token_emb`` = the final state, ``seq_emb`` = its mean over the first ``text_len`` positions.

    ``pe`` and ``conv_gru`` only HOLD the buffer and the parameters (state-dict keys ``embedding...``, ``pe.pe``,
    ``conv_gru.reset_gate.weight / .bias``, ``conv_gru.update_gate...``, ``conv_gru.out_gate...``); the arithmetic runs in
    ``torch.ops.tag.text_intra``: the core and the cell's element-wise steps are the row-local HIP kernels of
    csrc/text_intra.hip, the gate products are tag_gemm calls.  Every quirk of the reference is kept:

    * the score is ``pe(x) @ pe(x)^T`` from TWO separate calls of ``pe``: in train mode two independent dropout masks behind
      the positions, at the FIXED p = 0.2 (not a constructor argument); in eval mode both operands are the same x + pe;
    * the score is unscaled (it reaches the hundreds: |pe_i|^2 = E / 2);
    * cells whose query or key is >= text_len are filled with 1e-10, NOT -inf: dead cells take part in the softmax with a
      score of about 0, a padded query row attends uniformly over all L positions, valid scores that are negative are
      outweighed by the dead cells, and no gradient reaches the score operands through a dead cell;
    * the message is ``attn @ x`` -- x, not x + pe;
    * ``token_emb`` is non-zero at padded positions, and pad tokens are looked up like any other (row 0 of the table, which
      therefore receives gradient); the result of a row depends on the batch's padded L.

    Unlike the reference, ``text`` / ``text_len`` may carry leading dimensions (flattened here, as in the two other encoders;
    the reference raises on a 3-D ``text``).  max(text_len) < L runs, as in the reference.  ``text_len`` 0 gives a finite
    ``token_emb`` (every cell of the row is dead) and ``seq_emb`` = 0/0 = NaN: the masked mean divides by text_len exactly as
    ``tag_embed_mean_forward`` (EmbeddingAgg) does for an empty phrase.  ``num_layers`` 0 returns the embedding and its
    masked mean.

    Dropout (train mode): the project's counter-based keep masks (``tag_dropout_mask``; seeds
    ops.text_intra_dropout_seeds(ops.new_seed(), num_layers), drawn from torch's global generator like the audio encoders'
    dropouts and decorrelated per rank by ops.SEED_RANK): the same rule as nn.Dropout's, not torch's random stream.

    There is no eager fallback: at most 64 tokens, embed_dim even and <= 1024; anything else raises ValueError."""

    MAX_TOKENS = ops.TEXT_INTRA_MAX_L

    def __init__(self, embedding: nn.Module, num_layers: int, pooling: str = "mean") -> None:
        super().__init__()
        if not hasattr(embedding, "embed_dim"):
            raise ValueError(f"IntraAttention: the embedding module {type(embedding).__name__} has no embed_dim attribute")
        ops.text_intra_check(embedding.embed_dim)
        self.embedding = embedding
        self.embed_dim = embedding.embed_dim
        self.pe = PositionalEncoding(self.embed_dim, 0.2)
        self.conv_gru = ConvGRUCell(self.embed_dim, self.embed_dim)
        self.num_layers = num_layers
        self.pooling = pooling

    def forward(self, input_dict):
        n_tok = np.shape(input_dict["text"])[-1]
        if n_tok > self.MAX_TOKENS:                        # before any launch
            raise ValueError(f"IntraAttention: {n_tok} tokens per phrase; the attention kernel serves at most {self.MAX_TOKENS} "
                             "and there is no eager fallback")
        lead = tuple(np.shape(input_dict["text"])[:-1])
        if len(lead) != 1:                                 # the inner module sees the flat (R, L) batch the reference's would
            input_dict = dict(input_dict, text=torch.as_tensor(input_dict["text"]).reshape(-1, n_tok),
                              text_len=torch.as_tensor(input_dict["text_len"]).reshape(-1))
        if self.num_layers < 1:
            out = self._embedding_and_mean(input_dict)
            return {k: v.view(*lead, *v.shape[1:]) for k, v in out.items()}
        x = self.embedding(input_dict)
        if isinstance(x, dict) and "token_emb" in x:
            x = x["token_emb"]
        L, E = x.shape[-2], x.shape[-1]
        x = x.reshape(-1, L, E)
        text_len = torch.as_tensor(input_dict["text_len"]).long().to(x.device).reshape(-1).contiguous()
        g = self.conv_gru
        params = [g.reset_gate.weight, g.reset_gate.bias, g.update_gate.weight, g.update_gate.bias, g.out_gate.weight,
                  g.out_gate.bias]
        p = float(self.pe.p) if self.training else 0.0
        seed = ops.new_seed() if p > 0.0 else 0
        pe = self.pe.pe[0]
        if ops.DIRECT_GRADS:
            tok, seq = ops.TextIntraFunction.apply(x, text_len, pe, self.num_layers, p, seed, *params)
        else:
            tok, seq, _ = torch.ops.tag.text_intra(x, text_len, pe, params, self.num_layers, p, seed)
        out = {"token_emb": tok.view(*lead, L, E)}
        if self.pooling == "mean":
            out["seq_emb"] = seq.view(*lead, E)
        return out

    def _embedding_and_mean(self, input_dict):
        """num_layers = 0: the loop of the reference does not run and its outputs are the embedding and mean_with_lens of it --
        the fused gather + mean launch (``tag_embed_mean_forward``) on the inner module's table."""
        layer = self.embedding if isinstance(self.embedding, EmbeddingLayer) else getattr(self.embedding, "embedding", None)
        if not isinstance(layer, EmbeddingLayer):
            raise NotImplementedError(f"IntraAttention: num_layers = 0 over {type(self.embedding).__name__} has no HIP kernel "
                                      "(served: EmbeddingLayer, EmbeddingAgg); there is no eager fallback")
        table = layer.core.weight
        ids = _ids_to_device(input_dict["text"], table)
        lens = torch.as_tensor(input_dict["text_len"]).long().to(table.device).reshape(-1).contiguous()
        if ops.DIRECT_GRADS:
            seq, tok = ops.EmbedMeanFunction.apply(table, ids, lens, True)
        else:
            seq, tok = torch.ops.tag.embed_mean(table, ids, lens)
        return {"token_emb": tok, "seq_emb": seq} if self.pooling == "mean" else {"token_emb": tok}


class SelfAttention(nn.Module):
    """models/text_encoder.py:240-268: EmbeddingLayer -> learned ``cls_token`` in front -> + sinusoidal positions -> dropout ->
    ONE nn.MultiheadAttention(batch_first=True) over the phrase, keys >= text_len + 1 masked -> ``seq_emb`` = the cls row,
    ``token_emb`` = the remaining rows (contextual).

    ``self.mha`` is an nn.MultiheadAttention that only HOLDS the parameters (state-dict keys ``mha.in_proj_weight`` ...,
    torch's default init); the arithmetic runs in ``torch.ops.tag.text_selfattn``: the two projections are tag_gemm calls, the
    scaled-dot-product core and the input builder are the row-local HIP kernels of csrc/text_attn.hip.  As in the reference
    only KEYS are masked: padded query positions produce output, so ``token_emb`` is non-zero at padded positions, and pad
    tokens are looked up like any other (row 0 of the table, which therefore receives gradient).  ``text_len`` 0 is legal:
    only the cls key is attended.

    Unlike the reference, every ``text_len`` in [0, L] is served: the reference builds its mask max(text_len) + 1 wide and
    nn.MultiheadAttention raises whenever the longest phrase does not fill the padded tensor.

    Dropout (train mode): the same ``dropout`` value acts behind the positions and on the attention weights, with the
    project's counter-based keep masks (``tag_dropout_mask``; seeds ops.text_selfattn_dropout_seeds(ops.new_seed()), drawn
    from torch's global generator like the audio encoders' dropouts and decorrelated per rank by ops.SEED_RANK): the same
    rule as nn.Dropout's, not torch's random stream.

    There is no eager fallback: at most 63 tokens (64 positions with cls), head_dim = embed_dim / num_heads in {16, 32} or a
    multiple of 64, embed_dim even and <= 1024; anything else raises ValueError / NotImplementedError."""

    MAX_TOKENS = ops.TEXT_SELFATTN_MAX_S - 1

    def __init__(self, vocab_size, embed_dim, num_heads, dropout=0.2, pretrained_embedding=None, freeze_embedding=False):
        super().__init__()
        if embed_dim % 2:
            raise ValueError(f"SelfAttention: embed_dim {embed_dim} is odd; the sin/cos position table is defined for even embed_dim only")
        ops.text_selfattn_check(embed_dim, num_heads)
        self.embed_dim = embed_dim
        self.embedding = EmbeddingLayer(vocab_size, embed_dim, pretrained_embedding, freeze_embedding)
        self.pe = PositionalEncoding(embed_dim, dropout)
        self.mha = nn.MultiheadAttention(embed_dim, num_heads, dropout, batch_first=True)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))

    def forward(self, input_dict):
        n_tok = np.shape(input_dict["text"])[-1]
        if n_tok > self.MAX_TOKENS:                        # before any launch
            raise ValueError(f"SelfAttention: {n_tok} tokens per phrase; the attention kernel serves at most {self.MAX_TOKENS} "
                             "(64 positions with the cls token) and there is no eager fallback")
        x = self.embedding(input_dict)
        lead = tuple(x.shape[:-2])
        L, E = x.shape[-2], x.shape[-1]
        x = x.reshape(-1, L, E)
        text_len = torch.as_tensor(input_dict["text_len"]).long().to(x.device).reshape(-1).contiguous()
        mha = self.mha
        params = [self.cls_token, mha.in_proj_weight, mha.in_proj_bias, mha.out_proj.weight, mha.out_proj.bias]
        p = float(self.pe.p) if self.training else 0.0
        seed = ops.new_seed() if p > 0.0 else 0
        pe = self.pe.pe[0]
        if ops.DIRECT_GRADS:
            out = ops.TextSelfAttnFunction.apply(x, text_len, pe, mha.num_heads, p, seed, *params)
        else:
            out, _ = torch.ops.tag.text_selfattn(x, text_len, pe, params, mha.num_heads, p, seed)
        return {"token_emb": out[:, 1:].contiguous().view(*lead, L, E), "seq_emb": out[:, 0].contiguous().view(*lead, E)}


class LaionClapEncoder(nn.Module):
    """models/text_encoder.py:311-327: the text tower of LAION-CLAP -- Hugging Face ``ClapTextModel`` (a RoBERTa-style
    post-LayerNorm encoder) as ``self.model`` and ``ClapProjectionLayer`` as ``self.projection`` -- TRAINABLE:
    ``forward(input_dict)`` reads ``input_ids`` / ``attention_mask`` (what ``datasets.text_tokenizer.HuggingFaceTokenizer``
    returns), of shape (R, L) or with any leading shape (flattened like the other text encoders), and returns
    ``token_emb`` = projection(last_hidden_state) (..., L, P) and ``seq_emb`` = normalize(projection(pooler_output)) (..., P).

    ``model`` and ``projection`` only HOLD the parameters, under Hugging Face's names (state-dict keys ``model.embeddings...``,
    ``model.encoder.layer.N...``, ``model.pooler.dense...``, ``projection.linear1 / linear2...``: a ``ClapModel`` checkpoint's
    ``text_model`` / ``text_projection`` load with ``load_state_dict``; the ``position_ids`` / ``token_type_ids`` index buffers
    are optional there).  The arithmetic runs in ``torch.ops.tag.text_clap``: dense layers on tag_gemm, the attention core of
    csrc/text_attn.hip, the row kernels of csrc/text_clap.hip.  ``models.hf_modeling_grounding.LaionClapEncoder`` stays the
    forward-only inference class.

    ``model_type``: a directory or a name that resolves WITHOUT the network (``local_files_only=True``) -- its weights and
    configuration are copied; otherwise the tower is built from ``CLAP_TEXT_DEFAULTS`` (RoBERTa-base + a 512-d projection)
    updated by ``config``, randomly initialised.  ``embed_dim`` = ``projection_dim``.

    Limits (ValueError before any launch, there is no eager fallback): 2 <= L <= 64 tokens; head_dim 16, 32 or a multiple of 64;
    hidden_size <= 1024.  ``attention_mask`` must be a right-padded PREFIX (ones, then zeros: what a tokenizer with
    ``padding=True`` returns): only its row sums reach the kernel.  A host-resident mask that is not a prefix raises ValueError; a
    device-resident one is NOT read back -- it is trusted.  A row with no valid key attends position 0 only (the attention
    core's clamp) instead of producing NaN.  Padded positions produce ``token_emb`` like any other query, as in Hugging Face.

    Dropout (train mode): Hugging Face's four sites -- behind the embedding LayerNorm, on the attention weights, behind
    ``attention.output.dense`` and behind ``output.dense`` -- at ``hidden_dropout_prob`` / ``attention_probs_dropout_prob`` of the
    configuration (0.1 both, ClapTextConfig's default), with the project's counter-based keep masks (``tag_dropout_mask``; seeds
    ops.text_clap_dropout_seeds(ops.new_seed(), layers), drawn from torch's global generator and decorrelated per rank by
    ops.SEED_RANK): the same rule as nn.Dropout's, not torch's random stream.  With nothing to differentiate
    (``freeze_text_encoder``, eval, ``no_grad``) nothing is saved for a backward pass."""

    MAX_TOKENS = ops.TEXT_CLAP_MAX_L

    def __init__(self, model_type: str = None, config: dict = None):
        super().__init__()
        from .hf_modeling_grounding import CLAP_TEXT_DEFAULTS, _Holder, _text_model
        cfg = dict(CLAP_TEXT_DEFAULTS, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
        pretrained = self._local_pretrained(model_type)
        if pretrained is not None:
            cfg.update(pretrained[0])
        else:
            cfg.update(config or {})
        ops.text_clap_check(cfg["hidden_size"], cfg["num_attention_heads"])
        if cfg["num_hidden_layers"] < 1:
            raise ValueError("LaionClapEncoder: num_hidden_layers must be >= 1")
        self.config = cfg
        self.model_type = model_type
        self.model = _text_model(cfg)
        self.projection = _Holder()
        self.projection.linear1 = nn.Linear(cfg["hidden_size"], cfg["projection_dim"])
        self.projection.linear2 = nn.Linear(cfg["projection_dim"], cfg["projection_dim"])
        self.embed_dim = cfg["projection_dim"]
        self._names = ops.text_clap_param_names(cfg["num_hidden_layers"])
        if pretrained is not None:
            self.load_state_dict(pretrained[1], strict=True)

    @staticmethod
    def _local_pretrained(model_type):
        """(configuration entries, state dict) of a ``ClapModel`` that resolves locally, else None.  Never touches the network."""
        if not model_type:
            return None
        try:
            from transformers import ClapModel
            clap = ClapModel.from_pretrained(model_type, local_files_only=True)
        except Exception:                                   # noqa: BLE001 - not cached / no such directory / no transformers
            return None
        tc = clap.config.text_config
        keys = ("vocab_size", "hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size", "max_position_embeddings",
                "layer_norm_eps", "pad_token_id", "hidden_dropout_prob", "attention_probs_dropout_prob")
        cfg = {k: getattr(tc, k) for k in keys}
        cfg["projection_dim"] = clap.config.projection_dim
        st = {"model." + k: v for k, v in clap.text_model.state_dict().items()}
        st.update({"projection." + k: v for k, v in clap.text_projection.state_dict().items()})
        return cfg, st

    def load_state_dict(self, state_dict, *a, **k):
        state_dict = dict(state_dict)
        for name in ("model.embeddings.position_ids", "model.embeddings.token_type_ids"):       # optional in checkpoints
            state_dict.setdefault(name, self.state_dict()[name])
        return super().load_state_dict(state_dict, *a, **k)

    def _params(self):
        own = dict(self.named_parameters())
        return [own[n] for n in self._names]

    def forward(self, input_dict: Dict):
        ids, mask = input_dict["input_ids"], input_dict["attention_mask"]
        shape = tuple(np.shape(ids))
        L = shape[-1]
        if not 2 <= L <= self.MAX_TOKENS:                   # before any launch
            raise ValueError(f"LaionClapEncoder: {L} tokens per phrase; the attention kernel serves 2 ... {self.MAX_TOKENS} tokens "
                             "and there is no eager fallback")
        if tuple(np.shape(mask)) != shape:
            raise ValueError(f"LaionClapEncoder: input_ids {shape} and attention_mask {tuple(np.shape(mask))} differ in shape")
        mask = torch.as_tensor(mask)
        if not mask.is_cuda:
            m = mask.reshape(-1, L) != 0
            if bool((m[:, 1:] & ~m[:, :-1]).any()):
                raise ValueError("LaionClapEncoder: attention_mask must be a right-padded prefix (ones, then zeros); the attention "
                                 "kernel reads only the number of valid keys per row")
        cfg = self.config
        table = self.model.embeddings.word_embeddings.weight
        ids = _ids_to_device(ids, table).reshape(-1, L)
        mask = mask.long().to(table.device).reshape(-1, L).contiguous()
        params = self._params()
        p_h = float(cfg["hidden_dropout_prob"]) if self.training else 0.0
        p_a = float(cfg["attention_probs_dropout_prob"]) if self.training else 0.0
        seed = ops.new_seed() if (p_h > 0.0 or p_a > 0.0) else 0
        heads, eps, pad = int(cfg["num_attention_heads"]), float(cfg["layer_norm_eps"]), int(cfg["pad_token_id"])
        if ops.DIRECT_GRADS:
            tok, seq = ops.TextClapFunction.apply(ids, mask, heads, eps, pad, p_h, p_a, seed, *params)
        else:
            need = torch.is_grad_enabled() and any(p.requires_grad for p in params)
            tok, seq, _ = torch.ops.tag.text_clap(ids, mask, params, heads, eps, pad, p_h, p_a, seed, need)
        lead = shape[:-1]
        return {"seq_emb": seq.view(*lead, seq.shape[-1]), "token_emb": tok.view(*lead, L, tok.shape[-1])}


#: BertConfig defaults of "bert-base-uncased"
BERT_DEFAULTS = dict(vocab_size=30522, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
                     max_position_embeddings=512, type_vocab_size=2, layer_norm_eps=1e-12, pad_token_id=0,
                     hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
#: the shape of sentence-transformers/all-MiniLM-L6-v2
MINILM_DEFAULTS = dict(BERT_DEFAULTS, hidden_size=384, num_hidden_layers=6, intermediate_size=1536)
_BERT_INDEX_BUFFERS = ("model.embeddings.position_ids", "model.embeddings.token_type_ids")


def _bert_model(cfg):
    """The parameter tree of Hugging Face's ``BertModel`` (names only; the arithmetic is torch.ops.tag.text_bert): the tree of the
    CLAP text model with BERT's embedding tables -- ``type_vocab_size`` token types, positions WITHOUT a padding index -- and
    without the two index buffers, which BertModel keeps out of its state dict."""
    from .hf_modeling_grounding import _text_model
    m = _text_model(cfg)
    D = cfg["hidden_size"]
    emb = m.embeddings
    emb.token_type_embeddings = nn.Embedding(cfg["type_vocab_size"], D)
    emb.position_embeddings = nn.Embedding(cfg["max_position_embeddings"], D)
    del emb._buffers["position_ids"], emb._buffers["token_type_ids"]
    return m


def _local_bert(path):
    """(configuration entries, state dict under ``model.``) of a ``BertModel`` that resolves locally, else None.  Never touches
    the network."""
    if not path:
        return None
    try:
        from transformers import BertModel
        bert = BertModel.from_pretrained(path, local_files_only=True)
    except Exception as e:                                  # noqa: BLE001 - not cached / no such directory / no transformers
        warnings.warn(f"{path!r} did not resolve to a local BertModel ({type(e).__name__}); the model is built from its "
                      "configuration and RANDOMLY initialised", stacklevel=3)
        return None
    hc = bert.config
    if getattr(hc, "hidden_act", "gelu") != "gelu" or getattr(hc, "position_embedding_type", "absolute") != "absolute":
        raise ValueError(f"{path}: hidden_act {hc.hidden_act!r} / position_embedding_type "
                         f"{getattr(hc, 'position_embedding_type', None)!r}; the HIP path serves erf-GELU and absolute positions")
    cfg = {k: getattr(hc, k) for k in BERT_DEFAULTS}
    if cfg["pad_token_id"] is None:
        cfg["pad_token_id"] = 0
    return cfg, {"model." + k: v for k, v in bert.state_dict().items()}


class _BertBase(nn.Module):
    """What Bert and SentenceBert share: the parameter tree under Hugging Face's ``BertModel`` names as ``self.model``,
    ``dummy_param`` (models/text_encoder.py:275,300), the input checks and the call of torch.ops.tag.text_bert."""

    MAX_TOKENS = ops.TEXT_CLAP_MAX_L

    def _build(self, defaults, pretrained, config):
        cfg = dict(defaults)
        cfg.update(pretrained[0] if pretrained is not None else (config or {}))
        if cfg["num_hidden_layers"] < 1:
            raise ValueError(f"{type(self).__name__}: num_hidden_layers must be >= 1")
        ops.text_bert_check(cfg["hidden_size"], cfg["num_attention_heads"], T=cfg["type_vocab_size"])
        self.config = cfg
        self.model = _bert_model(cfg)
        self.dummy_param = nn.Parameter(torch.zeros(1))
        self.embed_dim = cfg["hidden_size"]
        self._names = ops.text_bert_param_names(cfg["num_hidden_layers"], pooler=False)
        self._register_load_state_dict_pre_hook(self._drop_index_buffers)
        if pretrained is not None:
            st = dict(pretrained[1])
            st["dummy_param"] = self.dummy_param.detach()
            self.load_state_dict(st, strict=True)
        else:
            self._init_weights(self.model)

    @staticmethod
    def _drop_index_buffers(state_dict, prefix, *_):
        """Load pre-hook: the ``position_ids`` / ``token_type_ids`` index buffers are optional in checkpoints.  It runs under
        whatever prefix this module has, so a checkpoint of a whole model loads strictly through the parent as well."""
        for name in _BERT_INDEX_BUFFERS:
            state_dict.pop(prefix + name, None)

    @staticmethod
    def _init_weights(model, std=0.02):
        """BertPreTrainedModel._init_weights: N(0, 0.02^2) matrices and tables, zero biases, LayerNorm at 1 / 0, a zero pad row."""
        for m in model.modules():
            if isinstance(m, (nn.Linear, nn.Embedding)):
                nn.init.normal_(m.weight, mean=0.0, std=std)
                if isinstance(m, nn.Linear):
                    nn.init.zeros_(m.bias)
                elif m.padding_idx is not None:
                    with torch.no_grad():
                        m.weight[m.padding_idx].zero_()
            elif isinstance(m, nn.LayerNorm):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)

    def _params(self):
        own = dict(self.named_parameters())
        return [own[n] for n in self._names]

    def _encode(self, ids, type_ids, mask, pool_mode, norm):
        """ids / type_ids (or None) / mask of one shape (..., L), any dtype, host or device -> token_emb (..., L, D),
        seq_emb (..., D), the int64 device mask (..., L)."""
        name = type(self).__name__
        shape = tuple(np.shape(ids))
        L = shape[-1]
        cfg = self.config
        if not 2 <= L <= self.MAX_TOKENS:                   # before any launch
            raise ValueError(f"{name}: {L} tokens per phrase; the attention kernel serves 2 ... {self.MAX_TOKENS} tokens and there "
                             "is no eager fallback")
        if L > cfg["max_position_embeddings"]:
            raise ValueError(f"{name}: {L} tokens per phrase but max_position_embeddings is {cfg['max_position_embeddings']}")
        for what, t in (("attention_mask", mask), ("token_type_ids", type_ids)):
            if t is not None and tuple(np.shape(t)) != shape:
                raise ValueError(f"{name}: input_ids {shape} and {what} {tuple(np.shape(t))} differ in shape")
        mask = torch.as_tensor(mask)
        if not mask.is_cuda:
            m = mask.reshape(-1, L) != 0
            if bool((m[:, 1:] & ~m[:, :-1]).any()):
                raise ValueError(f"{name}: attention_mask must be a right-padded prefix (ones, then zeros); the attention kernel "
                                 "reads only the number of valid keys per row")
        table = self.model.embeddings.word_embeddings.weight
        if type_ids is not None:
            type_ids = torch.as_tensor(type_ids)
            if not type_ids.is_cuda and type_ids.numel():
                lo, hi = int(type_ids.min()), int(type_ids.max())
                if lo < 0 or hi >= cfg["type_vocab_size"]:
                    raise ValueError(f"{name}: token_type_ids span [{lo}, {hi}], type_vocab_size is {cfg['type_vocab_size']}")
            type_ids = type_ids.long().to(table.device).reshape(-1, L).contiguous()
        ids = _ids_to_device(ids, table).reshape(-1, L)
        mask = mask.long().to(table.device).reshape(-1, L).contiguous()
        params = self._params()
        p_h = float(cfg["hidden_dropout_prob"]) if self.training else 0.0
        p_a = float(cfg["attention_probs_dropout_prob"]) if self.training else 0.0
        seed = ops.new_seed() if (p_h > 0.0 or p_a > 0.0) else 0
        heads, eps, pad = int(cfg["num_attention_heads"]), float(cfg["layer_norm_eps"]), int(cfg["pad_token_id"])
        if ops.DIRECT_GRADS:
            tok, seq = ops.TextBertFunction.apply(ids, type_ids, mask, heads, eps, pad, pool_mode, norm, p_h, p_a, seed, *params)
        else:
            need = torch.is_grad_enabled() and any(p.requires_grad for p in params)
            tok, seq, _ = torch.ops.tag.text_bert(ids, type_ids, mask, params, heads, eps, pad, pool_mode, norm, p_h, p_a, seed, need)
        lead = shape[:-1]
        return tok.view(*lead, L, tok.shape[-1]), seq.view(*lead, seq.shape[-1]), mask.view(shape)


class Bert(_BertBase):
    """models/text_encoder.py:271-293: Hugging Face ``BertModel`` with ``[CLS]`` pooling, TRAINABLE on the HIP text tower.
    ``forward(input_dict)`` reads ``input_ids``, ``token_type_ids`` and ``attention_mask`` -- any leading shape (flattened like the
    other text encoders), any dtype (the reference's runner stages them as float, hence its ``.long()``) -- and returns ``seq_emb``
    = ``last_hidden_state[:, 0]`` (..., D), ``token_emb`` = ``last_hidden_state`` (..., L, D) and ``attention_mask``.

    ``self.model`` only HOLDS the parameters, under ``BertModel``'s names (``model.embeddings.*``, ``model.encoder.layer.N.*``,
    ``model.pooler.dense.*``), next to ``dummy_param``: a reference checkpoint loads with ``load_state_dict(strict=True)``; the
    ``position_ids`` / ``token_type_ids`` index buffers are optional there.  The arithmetic runs in ``torch.ops.tag.text_bert``:
    BertEmbeddings and the pooling in csrc/text_bert.hip, the encoder stack shared with LaionClapEncoder.  The pooler and
    ``dummy_param`` take no part in it and receive no gradient.

    ``model_name``: a directory or a name that resolves WITHOUT the network (``local_files_only=True``) -- its weights and
    configuration are copied; otherwise (with a warning when a name was given) the model is built from ``BERT_DEFAULTS`` (BERT-base)
    updated by ``config`` and initialised as ``BertPreTrainedModel`` does (N(0, 0.02^2), LayerNorm 1 / 0).  ``embed_dim`` = ``hidden_size``.

    Limits (ValueError before any launch, there is no eager fallback): 2 <= L <= 64 tokens and L <= max_position_embeddings;
    head_dim 16, 32 or a multiple of 64; hidden_size <= 1024; at most 16 token types; erf-GELU and absolute positions;
    ``attention_mask`` a right-padded PREFIX (a host-resident mask is checked, a device-resident one is trusted); host-resident
    ``token_type_ids`` outside the table raise ValueError, device-resident ones are clamped and raise the sticky flag of
    ``ops.check_async_errors``.  Dropout (train mode): Hugging Face's four sites with the project's counter-based keep masks, as in
    LaionClapEncoder."""

    def __init__(self, model_name: str = None, config: dict = None):
        super().__init__()
        self.model_name = model_name
        self._build(BERT_DEFAULTS, _local_bert(model_name), config)

    def load_pretrained(self, pretrained, output_fn):       # models/text_encoder.py:278-279
        pass

    def forward(self, input_dict: Dict):
        tok, seq, mask = self._encode(input_dict["input_ids"], input_dict["token_type_ids"], input_dict["attention_mask"],
                                      ops.TEXT_BERT_POOL_MODES["cls"], ops.TEXT_BERT_NORMS["none"])
        return {"seq_emb": seq, "token_emb": tok, "attention_mask": mask}


class SentenceBert(_BertBase):
    """models/text_encoder.py:296-308: a sentence-transformers BERT model -- transformer, ``Pooling`` (mean or cls), optional
    ``Normalize`` -- TRAINABLE on the HIP text tower, WITHOUT the ``sentence_transformers`` package.

    ``model_type``: a LOCAL sentence-transformers directory: the transformer at its root or under ``0_Transformer/``, the pooling
    choice from ``1_Pooling/config.json`` (any mode but mean / cls raises ValueError), a ``Normalize`` entry from ``modules.json``,
    ``max_seq_length`` from ``sentence_bert_config.json``.  Without a directory the model is built from ``MINILM_DEFAULTS``
    (all-MiniLM-L6-v2's shape) updated by ``config``, with ``pooling`` / ``normalize`` as given, initialised as in ``Bert`` (with a
    warning when a name was given).

    ``forward(text)``: a list of strings is tokenised with the directory's tokenizer (``self.tokenizer``, which can be injected),
    padded to the batch's longest phrase and truncated at ``min(max_seq_length, 64)``; a dict with ``input_ids`` /
    ``attention_mask`` (and ``token_type_ids`` if present) is accepted as well, so that the class also works inside ``BiEncoder``.
    -> ``seq_emb`` pooled and normalised as configured, ``token_emb`` the last hidden state.  Limits and dropout as in ``Bert``.
    Parity with the ``sentence_transformers`` package itself is NOT pinned by a test (the package is not a dependency)."""

    def __init__(self, model_type: str = None, config: dict = None, pooling: str = "mean", normalize: bool = True):
        super().__init__()
        self.model_type = model_type
        self.max_seq_length = self.MAX_TOKENS
        self.tokenizer = None
        self._tokenizer_dir = None
        pretrained = None
        if model_type and os.path.isdir(model_type):
            pooling, normalize, self.max_seq_length, root = self._read_directory(model_type)
            pretrained = _local_bert(root)
            if pretrained is None:
                raise ValueError(f"SentenceBert: no BERT transformer could be read from {root}")
            self._tokenizer_dir = root
        elif model_type:
            warnings.warn(f"{model_type!r} is not a local sentence-transformers directory; the model is built from its "
                          "configuration and RANDOMLY initialised", stacklevel=2)
        if pooling not in ops.TEXT_BERT_POOL_MODES:
            raise ValueError(f"SentenceBert: pooling {pooling!r}; 'mean' and 'cls' exist")
        self.pooling, self.normalize = pooling, bool(normalize)
        self._build(MINILM_DEFAULTS, pretrained, config)

    @staticmethod
    def _read_directory(path):
        """-> (pooling, normalize, max_seq_length, the transformer's directory) of a sentence-transformers directory."""
        def read(*parts):
            f = os.path.join(path, *parts)
            if not os.path.isfile(f):
                return None
            with open(f) as fh:
                return json.load(fh)
        modules = read("modules.json") or []
        kinds = {str(m.get("type", "")).rsplit(".", 1)[-1]: m.get("path", "") for m in modules}
        root = os.path.join(path, kinds.get("Transformer", "")) if kinds.get("Transformer") else path
        if not os.path.isfile(os.path.join(root, "config.json")) and os.path.isfile(os.path.join(path, "0_Transformer", "config.json")):
            root = os.path.join(path, "0_Transformer")
        pool = read(kinds.get("Pooling") or "1_Pooling", "config.json") or {"pooling_mode_mean_tokens": True}
        on = sorted(k[len("pooling_mode_"):] for k, v in pool.items() if k.startswith("pooling_mode_") and v is True)
        if on == ["mean_tokens"]:
            pooling = "mean"
        elif on == ["cls_token"]:
            pooling = "cls"
        else:
            raise ValueError(f"SentenceBert: pooling modes {on} of {path}; exactly one of mean_tokens / cls_token is served")
        sb = {}
        for d in (root, path):
            sb = sb or read(os.path.relpath(d, path), "sentence_bert_config.json") or {}
        return pooling, "Normalize" in kinds, int(sb.get("max_seq_length") or SentenceBert.MAX_TOKENS), root

    def _tokenize(self, text):
        if self.tokenizer is None:
            if self._tokenizer_dir is None:
                raise RuntimeError("SentenceBert: strings need a tokenizer; none came with the model (set .tokenizer)")
            from transformers import AutoTokenizer
            self.tokenizer = AutoTokenizer.from_pretrained(self._tokenizer_dir, local_files_only=True)
        return self.tokenizer(list(text), padding=True, truncation=True, max_length=min(self.max_seq_length, self.MAX_TOKENS),
                              return_tensors="pt")

    def forward(self, text):
        tokens = text if isinstance(text, Mapping) else self._tokenize(text)
        norm = ops.TEXT_BERT_NORMS["normalize" if self.normalize else "none"]
        tok, seq, _ = self._encode(tokens["input_ids"], tokens.get("token_type_ids"), tokens["attention_mask"],
                                   ops.TEXT_BERT_POOL_MODES[self.pooling], norm)
        return {"seq_emb": seq, "token_emb": tok}
