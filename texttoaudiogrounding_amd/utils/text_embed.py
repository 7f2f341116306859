"""Phrase embeddings from the project's own BERT encoders: what the reference gets from a SentenceTransformer
(utils/data/create_text_embedding/prepare_phrase_sbert.py) or from the text side of a trained audio-text retrieval model
(prepare_phrase_clap.py), as ``{phrase: float32 vector}`` tables for the device clustering / label-map tools.

* ``PhraseEmbedder(encoder, tokenizer)``: strings -> (N, E) float32 in input order.  Everything is tokenised once, sorted by token
  count and cut into batches that are padded only to each batch's own longest phrase: a padded token costs a full GEMM row in
  every layer, and the result for the valid tokens does not depend on the padding (the attention core masks the keys beyond a
  phrase's length; tests/test_gpu_text_bert.py).  The reference pads every batch to ``max_text_length``.
* ``RetrievalTextEncoder``: ``text_encoder.model.*`` (a ``Bert`` with [CLS] pooling) and ``text_proj.*`` of
  ``audio_text_retrieval_models.AudioTextClip``; ``with_proj`` is one GEMM and the retrieval model's normalisation
  ``x / (|x| + 1e-7)`` clipped to +-1e3.  The audio side (Cnn14, ResNet38, AST) is out of scope: its keys are dropped.
"""
import json
import os

import numpy as np
import torch
import torch.nn as nn

from .. import ops
from ..models.text_encoder import BERT_DEFAULTS, Bert


class PhraseEmbedder:
    """``encode(list[str]) -> np.float32 (N, E)`` in input order, forward-only (``no_grad``: nothing is saved).

    encoder: a module whose ``forward(dict)`` takes ``input_ids`` / ``token_type_ids`` / ``attention_mask`` (B, L) and returns
    ``seq_emb`` (B, E): ``Bert``, ``SentenceBert``, ``RetrievalTextEncoder``.  tokenizer: a Hugging Face tokenizer (called with
    ``truncation=True, max_length=..., padding=False``).  batch_tokens: the largest batch, in PADDED tokens (phrases x the batch's
    longest phrase); max_length: the truncation length, at most the tower's 64."""

    def __init__(self, encoder, tokenizer, batch_tokens=16384, max_length=64):
        if batch_tokens < 2:
            raise ValueError("PhraseEmbedder: batch_tokens must be >= 2")
        if not 2 <= max_length <= ops.TEXT_CLAP_MAX_L:
            raise ValueError(f"PhraseEmbedder: max_length {max_length}; the tower serves 2 ... {ops.TEXT_CLAP_MAX_L} tokens")
        self.encoder, self.tokenizer = encoder, tokenizer
        self.batch_tokens, self.max_length = int(batch_tokens), int(max_length)
        self.pad_id = int(getattr(tokenizer, "pad_token_id", None) or 0)

    @staticmethod
    def plan(lengths, batch_tokens):
        """Token counts -> the batches as lists of input indices: ascending token count (ties in input order), each batch as many
        phrases as fit ``phrases x longest <= batch_tokens`` (at least one)."""
        order = sorted(range(len(lengths)), key=lambda i: (lengths[i], i))
        batches, cur = [], []
        for i in order:
            if cur and (len(cur) + 1) * lengths[i] > batch_tokens:       # sorted: lengths[i] is the batch's longest
                batches.append(cur)
                cur = []
            cur.append(i)
        if cur:
            batches.append(cur)
        return batches

    def tokenize(self, phrases):
        """-> (input_ids, token_type_ids) as lists of lists, unpadded, truncated at max_length."""
        enc = self.tokenizer(list(phrases), truncation=True, max_length=self.max_length, padding=False)
        ids = [list(x) for x in enc["input_ids"]]
        types = [list(x) for x in enc["token_type_ids"]] if "token_type_ids" in enc else [[0] * len(x) for x in ids]
        return ids, types

    def batch(self, ids, types, index):
        """The padded batch of the phrases ``index``: a dict of (B, L) int64 tensors, L the batch's longest phrase (>= 2)."""
        L = max(2, max(len(ids[i]) for i in index))
        B = len(index)
        out = {"input_ids": torch.full((B, L), self.pad_id, dtype=torch.long), "token_type_ids": torch.zeros(B, L, dtype=torch.long),
               "attention_mask": torch.zeros(B, L, dtype=torch.long)}
        for r, i in enumerate(index):
            n = len(ids[i])
            out["input_ids"][r, :n] = torch.as_tensor(ids[i], dtype=torch.long)
            out["token_type_ids"][r, :n] = torch.as_tensor(types[i], dtype=torch.long)
            out["attention_mask"][r, :n] = 1
        return out

    def encode(self, phrases):
        phrases = list(phrases)
        if not phrases:
            return np.zeros((0, int(getattr(self.encoder, "embed_dim", 0))), dtype=np.float32)
        ids, types = self.tokenize(phrases)
        out = None
        with torch.no_grad():
            for index in self.plan([len(x) for x in ids], self.batch_tokens):
                emb = self.encoder(self.batch(ids, types, index))["seq_emb"]
                emb = emb.detach().float().cpu().numpy()
                if out is None:
                    out = np.empty((len(phrases), emb.shape[-1]), dtype=np.float32)
                out[index] = emb
        return out


def _bert_config_from_state(state, prefix):
    """BertModel's shape read off a state dict (everything but the number of heads)."""
    g = lambda k: state[prefix + k]                          # noqa: E731
    layers = 1 + max(int(k[len(prefix + "encoder.layer."):].split(".")[0]) for k in state if k.startswith(prefix + "encoder.layer."))
    V, D = g("embeddings.word_embeddings.weight").shape
    return dict(vocab_size=V, hidden_size=D, num_hidden_layers=layers,
                intermediate_size=g("encoder.layer.0.intermediate.dense.weight").shape[0],
                max_position_embeddings=g("embeddings.position_embeddings.weight").shape[0],
                type_vocab_size=g("embeddings.token_type_embeddings.weight").shape[0])


class RetrievalTextEncoder(nn.Module):
    """The text side of ``audio_text_retrieval_models.AudioTextClip``: ``text_encoder`` (``Bert``, [CLS] pooling; state-dict keys
    ``text_encoder.model.*``) and ``text_proj`` (``nn.Linear(hidden, shared_dim)``).  ``forward(tokens)`` -> ``seq_emb``: the
    [CLS] embedding, or with ``with_proj`` ``text_proj`` of it normalised as the retrieval model does (``x / (|x| + 1e-7)`` clipped
    to +-1e3; forward-only), and ``token_emb``."""

    def __init__(self, config: dict = None, shared_dim: int = 1024, with_proj: bool = False, model_type: str = None):
        super().__init__()
        self.text_encoder = Bert(model_type, config)
        self.text_proj = nn.Linear(self.text_encoder.embed_dim, shared_dim)
        if shared_dim > 1024:
            raise ValueError(f"RetrievalTextEncoder: shared_dim {shared_dim}; the row kernels serve at most 1024 channels")
        self.with_proj = bool(with_proj)
        self.embed_dim = shared_dim if with_proj else self.text_encoder.embed_dim
        self.dropped_keys = 0

    def load_retrieval_state_dict(self, state):
        """Load ``AudioTextClip.state_dict()``: the ``audio_encoder.*``, ``audio_proj.*`` and ``logit_scale`` keys are dropped
        (-> how many), everything else must match exactly."""
        keep = {k: v for k, v in state.items()
                if not (k.startswith("audio_encoder.") or k.startswith("audio_proj.") or k == "logit_scale")}
        self.dropped_keys = len(state) - len(keep)
        keep.setdefault("text_encoder.dummy_param", self.text_encoder.dummy_param.detach())
        self.load_state_dict(keep, strict=True)
        return self.dropped_keys

    @classmethod
    def from_experiment(cls, experiment_path, with_proj=False, device="cuda"):
        """``<experiment_path>/models/config.json`` + ``models/trained_model.pth["state_dict"]`` -> (encoder on ``device`` in eval
        mode, tokenizer resolved LOCALLY from ``tokenizer_type``, the configuration).  The BERT shape is read off the checkpoint;
        the number of heads from the locally resolved ``model_type`` configuration, else hidden_size / 64."""
        from transformers import AutoConfig, AutoTokenizer
        with open(os.path.join(experiment_path, "models", "config.json")) as f:
            config = json.load(f)
        ckpt = torch.load(os.path.join(experiment_path, "models", "trained_model.pth"), map_location="cpu", weights_only=False)
        state = ckpt["state_dict"]
        bert = dict(BERT_DEFAULTS, **_bert_config_from_state(state, "text_encoder.model."))
        model_type = config["model"]["text_encoder"]["args"].get("model_type")
        try:
            hc = AutoConfig.from_pretrained(model_type, local_files_only=True)
            bert.update(num_attention_heads=hc.num_attention_heads, layer_norm_eps=hc.layer_norm_eps,
                        pad_token_id=hc.pad_token_id if hc.pad_token_id is not None else 0)
        except Exception:                                    # noqa: BLE001 - not cached: BERT's head_dim 64
            bert["num_attention_heads"] = max(1, bert["hidden_size"] // 64)
        model = cls(bert, state["text_proj.weight"].shape[0], with_proj)
        dropped = model.load_retrieval_state_dict(state)
        print(f"RetrievalTextEncoder: dropped {dropped} audio-side keys of {len(state)}")
        tokenizer_type = config["data_loader"]["collate_fn"]["args"]["tokenizer_type"]
        tokenizer = AutoTokenizer.from_pretrained(tokenizer_type, local_files_only=True)
        return model.to(device).eval(), tokenizer, config

    def forward(self, tokens):
        out = self.text_encoder({"input_ids": tokens["input_ids"], "token_type_ids": tokens.get("token_type_ids"),
                                 "attention_mask": tokens["attention_mask"]})
        seq = out["seq_emb"]
        if self.with_proj:
            if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
                raise ValueError("RetrievalTextEncoder: with_proj is forward-only (normalisation 2 has no backward); use no_grad")
            lead, D = seq.shape[:-1], seq.shape[-1]
            x = seq.reshape(-1, D).contiguous()
            R, E = x.shape[0], self.text_proj.out_features
            y = ops.gemm(x, self.text_proj.weight.detach(), R, E, D, transB=True, bias=self.text_proj.bias.detach())
            seq, _ = ops.text_bert_pool_forward(y.view(R, 1, E), None, ops.TEXT_BERT_POOL_MODES["cls"], ops.TEXT_BERT_NORMS["retrieval"])
            seq = seq.view(*lead, E)
        return {"seq_emb": seq, "token_emb": out["token_emb"]}
