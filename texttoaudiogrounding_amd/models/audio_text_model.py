"""Model composition (mirror of BiEncoder, models/audio_text_model.py:16-98 in the reference) and the early-fusion grounding
models CrossCnn8_Rnn (models/audio_text_model.py:571-840) and CrossCDur (models/audio_text_model.py:461-568), and the
class-mapping baseline AudioTagging (models/audio_text_model.py:405-458); the weakly supervised MultiTextBiEncoder (:101-229) and
MultiTextBiEncoderWithAlign (:232-402); the sentence-level AudioTextAlignByWord / ByPhrase (:843-976) and AudioTextCrossAlignByPhrase
(:979-1073)."""
import sys
from typing import Optional

import torch
import torch.nn as nn

from .. import ops
from .. import engine, torch_ops
from .audio_encoder import _MelFrontendBuffers, htk_mel_filterbank, slaney_mel_filterbank
from .augmentation import SpecAugmentation
from .panns import init_bn, init_layer
from .utils import init_weights


class BiEncoder(nn.Module):
    def __init__(self, audio_encoder: nn.Module, text_encoder: nn.Module, match_fn: nn.Module, shared_dim: int,
                 cross_encoder: Optional[nn.Module] = None, add_proj: bool = False, upsample: bool = False,
                 freeze_audio_encoder: bool = False, freeze_text_encoder: bool = False,
                 pretrained: Optional[str] = None):
        super().__init__()
        self.audio_encoder = audio_encoder
        self.text_encoder = text_encoder
        self.match_fn = match_fn
        self.cross_encoder = cross_encoder
        if audio_encoder.embed_dim != text_encoder.embed_dim or add_proj:
            self.audio_proj = nn.Linear(audio_encoder.embed_dim, shared_dim)
            self.text_proj = nn.Linear(text_encoder.embed_dim, shared_dim)
        self.interpolate_ratio = self.audio_encoder.downsample_ratio
        self.upsample = upsample
        if pretrained is not None and type(self) is BiEncoder:
            self.load_pretrained(pretrained)
        if freeze_audio_encoder:
            for p in self.audio_encoder.parameters():
                p.requires_grad = False
        if freeze_text_encoder:
            for p in self.text_encoder.parameters():
                p.requires_grad = False

    def load_pretrained(self, ckpt_path, output_fn=print):
        state = torch.load(ckpt_path, map_location="cpu")
        state = state.get("model", state)
        own = self.state_dict()
        matched = {k: v for k, v in state.items() if k in own and own[k].shape == v.shape}
        output_fn(f"BiEncoder: loading {len(matched)}/{len(own)} tensors from {ckpt_path}")
        own.update(matched)
        self.load_state_dict(own)

    def forward(self, input_dict):
        audio_output = self.audio_encoder(input_dict)
        audio_emb = audio_output["embedding"]
        text_emb = self.text_encoder(input_dict)
        forward_dict = {"audio_emb": audio_emb, "text_emb": text_emb, "audio_len": audio_output["length"]}
        if "text_len" in input_dict:
            forward_dict["text_len"] = input_dict["text_len"]
        if self.cross_encoder is not None:
            forward_dict.update(self.cross_encoder(forward_dict))
            text_emb = forward_dict["text_emb"]
        if hasattr(self, "audio_proj"):
            forward_dict["audio_emb"] = ops.LinearFunction.apply(forward_dict["audio_emb"], self.audio_proj.weight,
                                                                 self.audio_proj.bias)
            if "seq_emb" in text_emb:
                text_emb["seq_emb"] = ops.LinearFunction.apply(text_emb["seq_emb"], self.text_proj.weight,
                                                               self.text_proj.bias)
            if self.cross_encoder is not None and "token_emb" in text_emb:
                text_emb["token_emb"] = ops.LinearFunction.apply(text_emb["token_emb"], self.text_proj.weight,
                                                                 self.text_proj.bias)
            # without a cross-encoder token_emb is not projected: no head consumes it (text_level='seq')
        frame_sim = self.match_fn(forward_dict)
        length = audio_output["length"]
        if self.interpolate_ratio != 1 and self.upsample:
            # F.interpolate(mode="linear", align_corners=False) x interpolate_ratio (models/audio_text_model.py:90-97)
            frame_sim = ops.UpsampleLinearFunction.apply(frame_sim, self.interpolate_ratio)
            length = length * self.interpolate_ratio
        return {"frame_sim": frame_sim, "length": length}


class MultiTextBiEncoder(BiEncoder):
    """Weakly supervised variant (mirror of models/audio_text_model.py:101-229 in the reference): every clip comes with N
    phrases; frame_sim (B,T',N) is pooled over time into clip_sim (B,N).  The audio embedding is NOT expanded to
    (B*N,T',D): the grouped head (ops.MatchGroupFunction) scores the N phrases of a clip against the same rows."""

    def __init__(self, audio_encoder: nn.Module, text_encoder: nn.Module, match_fn: nn.Module, shared_dim: int,
                 text_forward_keys: "list[str]", cross_encoder: Optional[nn.Module] = None, pooling: str = "linear_softmax",
                 add_proj: bool = False, upsample: bool = False, freeze_audio_encoder: bool = False,
                 freeze_text_encoder: bool = False, safe_size: Optional[int] = None, pretrained: Optional[str] = None,
                 output_fn=print):
        super().__init__(audio_encoder=audio_encoder, text_encoder=text_encoder, match_fn=match_fn, shared_dim=shared_dim,
                         cross_encoder=cross_encoder, add_proj=add_proj, upsample=upsample,
                         freeze_audio_encoder=freeze_audio_encoder, freeze_text_encoder=freeze_text_encoder)
        self.text_forward_keys = list(text_forward_keys)
        if "text_len" not in self.text_forward_keys:
            self.text_forward_keys.append("text_len")
        if pooling not in ops.POOL_MODES:
            raise Exception(f"Unsupported pooling {pooling}")         # the reference raises at forward time (:215)
        self.pooling = pooling
        self.safe_size = safe_size          # chunking knob of the reference: unnecessary here (no expansion)
        if pretrained is not None and type(self) is MultiTextBiEncoder:
            self.load_pretrained(pretrained, output_fn)

    def _pool(self, sim, B, N, length):
        len_dev = torch.as_tensor(length).long().to(sim.device).contiguous()
        # linear_softmax / max / mean / exp_softmax _with_lens over the valid frames (models/audio_text_model.py:205-215)
        clip_sim = ops.SimPoolFunction.apply(sim.view(B * N, -1, 1), len_dev, None, N, 1, ops.POOL_MODES[self.pooling],
                                             -1).view(B, N)
        if self.interpolate_ratio != 1 and self.upsample:                                    # models/audio_text_model.py:216-224
            sim = ops.UpsampleLinearFunction.apply(sim, self.interpolate_ratio)
            length = length * self.interpolate_ratio
        frame_sim = sim.view(B, N, -1).transpose(1, 2)                                       # (B, T', N)
        return {"frame_sim": frame_sim, "clip_sim": clip_sim, "length": length}

    def _encode(self, input_dict):
        """One audio pass and one text pass (models/audio_text_model.py:148-162): the audio embedding behind ``audio_proj`` and the
        text encoder's output over the B*N flattened phrases -- shared by the phrase-level head and, in
        MultiTextBiEncoderWithAlign, the sentence-level one."""
        audio_output = self.audio_encoder(input_dict)
        audio_emb = audio_output["embedding"]
        if hasattr(self, "audio_proj"):
            audio_emb = ops.LinearFunction.apply(audio_emb, self.audio_proj.weight, self.audio_proj.bias)
        text_forward_dict = {}
        for key in self.text_forward_keys:
            x = torch.as_tensor(input_dict[key])
            text_forward_dict[key] = x.reshape(x.shape[0] * x.shape[1], *x.shape[2:])
        text_emb = self.text_encoder(text_forward_dict)
        return audio_output, audio_emb, text_forward_dict, text_emb

    def _phrase_general(self, audio_emb, length, text_len, text_emb, B, N):
        """The reference's own data flow (models/audio_text_model.py:164-203): the audio embedding repeated for the N phrases
        of its clip, (B*N)-row cross-encoder and head.  Taken with a cross-encoder or a head other than the grouped
        DotProduct; ``safe_size`` chunking is unnecessary (the heads are row kernels, nothing is materialised per chunk)."""
        forward_dict = {"audio_emb": ops.GroupExpandFunction.apply(audio_emb, N), "text_emb": text_emb,
                        "audio_len": torch.as_tensor(length).repeat_interleave(N), "text_len": text_len}
        if self.cross_encoder is not None:
            forward_dict.update(self.cross_encoder(forward_dict))
        if hasattr(self, "text_proj"):
            text_emb = forward_dict["text_emb"]
            for k in ("seq_emb", "token_emb"):
                if k in text_emb:
                    text_emb[k] = ops.LinearFunction.apply(text_emb[k], self.text_proj.weight, self.text_proj.bias)
        sim = self.match_fn(forward_dict)                                                     # (B*N, T')
        return self._pool(sim.contiguous(), B, N, length)

    def _phrase_level(self, audio_output, audio_emb, text_forward_dict, text_emb, general=False):
        """frame_sim (B,T',N) and clip_sim (B,N).  ``text_emb`` is left as the text encoder returned it: the general path works
        on a shallow copy of the dict (the reference clones the tensors, :288), so a projection replaces entries of the copy."""
        from .match import DotProduct
        B = audio_emb.size(0)
        N = text_forward_dict[self.text_forward_keys[0]].shape[0] // B
        length = audio_output["length"]
        if (general or self.cross_encoder is not None or not isinstance(self.match_fn, DotProduct) or self.match_fn.l2norm
                or self.match_fn.text_level != "seq"):
            return self._phrase_general(audio_emb, length, text_forward_dict["text_len"], dict(text_emb), B, N)
        seq = text_emb["seq_emb"]
        if hasattr(self, "text_proj"):
            seq = ops.LinearFunction.apply(seq, self.text_proj.weight, self.text_proj.bias)
        sim = ops.MatchGroupFunction.apply(audio_emb, seq, N, self.match_fn.scale)            # (B*N, T')
        return self._pool(sim, B, N, length)

    def _forward_general(self, input_dict):
        return self._phrase_level(*self._encode(input_dict), general=True)

    def forward(self, input_dict):
        return self._phrase_level(*self._encode(input_dict))


class MultiTextBiEncoderWithAlign(MultiTextBiEncoder):
    """MultiTextBiEncoder plus a sentence-level score (mirror of models/audio_text_model.py:232-402): from ONE audio pass and ONE
    text pass, the phrase-level frame_sim / clip_sim of the parent and ``sentence_sim`` (B,B) = sentence_pooling(align_fn(audio_emb,
    seq_emb of every clip's positive phrases)), for MultipleLossSum over a clip-level and a sentence-level objective.

    The positives of clip i are its first ``label[i].sum()`` phrases.  The reference gathers and pads them to the longest count;
    here align_fn sees all N phrases of every clip and the pooling masks the columns at and beyond ``text_len = label.sum(1)``
    (every sim_pooling reducer does, in both directions) -- the same sentence_sim with no gather, and no device-to-host copy of
    the counts.  With ``output_matrix`` (evaluation / inspection) the operand is cut to the reference's max(count) columns and
    the phrases beyond a clip's count are zeroed first, so ``sim_matrix`` is the reference's, padded columns included; that path
    does read the counts back.  As in the reference, align_fn takes the PROJECTED audio embedding and the UNPROJECTED seq_emb, so
    with ``add_proj`` and unequal sizes its assert fails, and the sentence branch never sees the cross-encoder.

    A clip without a positive phrase divides by zero in the reference: a host-resident ``label`` with such a row raises
    ValueError before anything is launched; a device-resident one is not read back -- its row of sentence_sim is then NaN / inf
    for the mean reducers, as in the reference."""

    def __init__(self, audio_encoder, text_encoder, match_fn, align_fn, sentence_pooling, shared_dim, text_forward_keys,
                 cross_encoder=None, phrase_pooling="linear_softmax", add_proj=False, upsample=False,
                 freeze_audio_encoder=False, freeze_text_encoder=False, safe_size=None):
        super().__init__(audio_encoder, text_encoder, match_fn, shared_dim, text_forward_keys, cross_encoder, phrase_pooling,
                         add_proj, upsample, freeze_audio_encoder, freeze_text_encoder, safe_size)
        self.align_fn = align_fn
        self.sentence_pooling = sentence_pooling

    def forward(self, input_dict):
        sentence = self.training or "label" in input_dict
        if sentence:
            label = torch.as_tensor(input_dict["label"])
            if not label.is_cuda and bool((label.sum(1) < 1).any()):
                raise ValueError("MultiTextBiEncoderWithAlign: every clip needs at least one positive phrase (a row of `label` "
                                 "sums to 0; the sentence-level mean over its phrases would divide by zero)")
        audio_output, audio_emb, text_forward_dict, text_emb = self._encode(input_dict)
        output = self._phrase_level(audio_output, audio_emb, text_forward_dict, text_emb)
        if not sentence:
            return output
        B = audio_emb.size(0)
        seq_emb = text_emb["seq_emb"]
        seq_emb = seq_emb.reshape(B, seq_emb.shape[0] // B, *seq_emb.shape[1:])               # (B, N, D), unprojected (:366-369)
        phrases_num = label.sum(1).long()
        output_matrix = input_dict.get("output_matrix", False)
        if output_matrix:
            # the matrix as the reference returns it: max(count) columns, the phrases beyond a clip's count as ZERO rows (what
            # pad_sequence leaves there); reads the counts back.  sentence_sim does not depend on those columns
            width = int(phrases_num.max())
            keep = torch.arange(width, device=seq_emb.device)[None, :] < phrases_num.to(seq_emb.device)[:, None]
            seq_emb = (seq_emb[:, :width] * keep[..., None].to(seq_emb.dtype)).contiguous()
        sim_matrix = self.align_fn(audio_emb, seq_emb)
        output["sentence_sim"] = self.sentence_pooling({"sim": sim_matrix, "audio_len": audio_output["length"],
                                                        "text_len": phrases_num})
        if output_matrix:
            output["sim_matrix"] = sim_matrix
        return output


class AudioTextAlignByWord(nn.Module):
    """Word-level weak alignment (mirror of models/audio_text_model.py:843-904): every clip's frames against every clip's
    WORD embeddings -- (projected) token_emb -> align.DotProduct (B,B,T',n_word) -> sim_pooling -> (B,B)."""

    def __init__(self, audio_encoder, text_encoder, match_fn, sim_pooling, shared_dim, add_proj=False,
                 freeze_audio_encoder=False, freeze_text_encoder=False):
        super().__init__()
        self.audio_encoder, self.text_encoder, self.match_fn, self.sim_pooling = audio_encoder, text_encoder, match_fn, sim_pooling
        if audio_encoder.embed_dim != text_encoder.embed_dim or add_proj:
            self.audio_proj = nn.Linear(audio_encoder.embed_dim, shared_dim)
            self.text_proj = nn.Linear(text_encoder.embed_dim, shared_dim)
        if freeze_audio_encoder:
            for p in self.audio_encoder.parameters():
                p.requires_grad = False
        if freeze_text_encoder:
            for p in self.text_encoder.parameters():
                p.requires_grad = False

    def forward(self, input_dict):
        audio_output = self.audio_encoder(input_dict)
        audio_emb = audio_output["embedding"]
        if hasattr(self, "audio_proj"):
            audio_emb = ops.LinearFunction.apply(audio_emb, self.audio_proj.weight, self.audio_proj.bias)
        word_emb = self.text_encoder(input_dict)["token_emb"]
        if hasattr(self, "text_proj"):
            word_emb = ops.LinearFunction.apply(word_emb, self.text_proj.weight, self.text_proj.bias)
        sim_matrix = self.match_fn(audio_emb, word_emb.contiguous())
        sim = self.sim_pooling({"sim": sim_matrix, "audio_len": audio_output["length"], "text_len": input_dict["text_len"]})
        output = {"sim": sim}
        if input_dict.get("output_matrix", False):
            output["sim_matrix"] = sim_matrix
        return output


class AudioTextAlignByPhrase(nn.Module):
    """Weakly supervised alignment (mirror of models/audio_text_model.py:907-976 in the reference): every clip against
    every clip's phrases -- align.DotProduct (B,B,T',N) -> sim_pooling -> (B,B) for MaxMarginRankingLoss."""

    def __init__(self, audio_encoder, text_encoder, match_fn, sim_pooling, shared_dim, cross_encoder=None, add_proj=False,
                 freeze_audio_encoder=False, freeze_text_encoder=False):
        super().__init__()
        self.audio_encoder, self.text_encoder, self.match_fn = audio_encoder, text_encoder, match_fn
        self.cross_encoder, self.sim_pooling = cross_encoder, sim_pooling        # stored and never applied, as in the reference (:925, :936-976)
        if audio_encoder.embed_dim != text_encoder.embed_dim or add_proj:
            self.audio_proj = nn.Linear(audio_encoder.embed_dim, shared_dim)
            self.text_proj = nn.Linear(text_encoder.embed_dim, shared_dim)
        if freeze_audio_encoder:
            for p in self.audio_encoder.parameters():
                p.requires_grad = False
        if freeze_text_encoder:
            for p in self.text_encoder.parameters():
                p.requires_grad = False

    def forward(self, input_dict):
        audio_output = self.audio_encoder(input_dict)
        audio_emb = audio_output["embedding"]
        text_key = input_dict["text_key"]
        phrases_emb = self.text_encoder({"text": input_dict[text_key], "text_len": input_dict[f"{text_key}_len"]})
        phrases_num = [int(v) for v in input_dict[f"{text_key}_num"]]
        seq_emb = torch.split(phrases_emb["seq_emb"], phrases_num, dim=0)
        seq_emb = nn.utils.rnn.pad_sequence(seq_emb, batch_first=True)          # (B, max_num, D)
        if hasattr(self, "audio_proj"):                                         # the reference declares but never applies them
            pass
        sim_matrix = self.match_fn(audio_emb, seq_emb.contiguous())
        sim = self.sim_pooling({"sim": sim_matrix, "audio_len": audio_output["length"], "text_len": phrases_num})
        output = {"sim": sim}
        if input_dict.get("output_matrix", False):
            output["sim_matrix"] = sim_matrix
        return output


class AudioTextCrossAlignByPhrase(nn.Module):
    """Sentence-level weak alignment WITH a cross-encoder (mirror of models/audio_text_model.py:979-1073): every clip of the
    batch is cross-encoded against every phrase of the batch, the token-level head scores each (clip, phrase, frame) and
    sim_pooling reduces the (B,B,T',N) matrix to the (B,B) ``sim`` of MaxMarginRankingLoss / InfoNceLoss / the triplet losses.
    Same constructor as the reference: ``add_proj`` is positional and creates nothing.

    Two paths, chosen by ``self.fused`` (None = automatic, True = demand the fused one, False = the loop):

    * fused -- ``cross_encoder`` is this package's CrossAttentionGating, ``match_fn`` is match.DotProduct(text_level="token",
      l2norm=False) and csrc/cross_pairs.hip serves (L, D): ONE ops.CrossPairsFunction call; nothing of B*P*T*D elements exists.
    * loop -- the reference's data flow with the existing modules: per clip, its audio expanded to the P phrases, the
      cross-encoder, the head, the scatter into the zero matrix.  Any cross-encoder and any token-level head."""

    def __init__(self, audio_encoder, text_encoder, match_fn, sim_pooling, shared_dim, add_proj, cross_encoder=None,
                 freeze_audio_encoder=False, freeze_text_encoder=False):
        super().__init__()
        self.audio_encoder, self.text_encoder, self.match_fn = audio_encoder, text_encoder, match_fn
        self.cross_encoder, self.sim_pooling = cross_encoder, sim_pooling
        self.fused = None
        if freeze_audio_encoder:
            for p in self.audio_encoder.parameters():
                p.requires_grad = False
        if freeze_text_encoder:
            for p in self.text_encoder.parameters():
                p.requires_grad = False

    def _fusable(self, L, D):
        from .cross_encoder import CrossAttentionGating
        from .match import DotProduct
        ce, mf = self.cross_encoder, self.match_fn
        return (type(ce) is CrossAttentionGating and type(mf) is DotProduct and mf.text_level == "token" and not mf.l2norm
                and tuple(ce.attn.h2attn.weight.shape) == (D, 2 * D) and ops.cross_pairs_served(L, D))

    def _loop(self, audio_emb, length, token_emb, text_len, phrases_num, T, N):
        B, P = audio_emb.size(0), token_emb.size(0)
        rows = []
        for i in range(B):
            c_o = self.cross_encoder({"audio_emb": ops.GroupExpandFunction.apply(audio_emb[i:i + 1].contiguous(), P),
                                      "text_emb": {"token_emb": token_emb}, "audio_len": [int(length[i])] * P,
                                      "text_len": text_len})
            sim_i = self.match_fn(c_o)                                         # (P, T)
            blocks = []
            for s in torch.split(sim_i, phrases_num, dim=0):                   # clip j's (pnum[j], T) -> (T, N), zero-padded
                blocks.append(torch.nn.functional.pad(s.transpose(0, 1), (0, N - s.shape[0])))
            rows.append(torch.stack(blocks))
        return torch.stack(rows)                                               # (B, B, T, N)

    def forward(self, input_dict):
        audio_output = self.audio_encoder(input_dict)
        audio_emb = audio_output["embedding"]
        text_key = input_dict["text_key"]
        text_len = input_dict[f"{text_key}_len"]
        token_emb = self.text_encoder({"text": input_dict[text_key], "text_len": text_len})["token_emb"]
        phrases_num = [int(v) for v in input_dict[f"{text_key}_num"]]
        length = audio_output["length"]
        if not audio_emb.is_cuda or not token_emb.is_cuda:
            raise RuntimeError(f"AudioTextCrossAlignByPhrase: expected embeddings on the MI355X (cuda) device, got "
                               f"{audio_emb.device} / {token_emb.device}; the HIP path has no CPU fallback")
        T, N = int(max(length)), max(phrases_num)
        if audio_emb.size(1) != T:
            raise RuntimeError(f"AudioTextCrossAlignByPhrase: the audio encoder returned {audio_emb.size(1)} frames but "
                               f"max(length) = {T}; sim_matrix has max(length) frames and the two must agree")
        L, D = token_emb.size(1), audio_emb.size(2)
        fusable = self._fusable(L, D)
        if self.fused and not fusable:
            raise RuntimeError("AudioTextCrossAlignByPhrase: fused = True needs this package's CrossAttentionGating, "
                               "match.DotProduct(text_level='token', l2norm=False) and a shape cross_pairs.hip serves "
                               f"(L = {L}, D = {D})")
        if fusable and self.fused is not False:
            ce = self.cross_encoder
            sim_matrix = ops.CrossPairsFunction.apply(audio_emb, length, token_emb, text_len, phrases_num,
                                                      ce.attn.h2attn.weight, ce.attn.h2attn.bias, ce.attn.v,
                                                      ce.gating.fc_u.weight, ce.gating.fc_u.bias, ce.gating.fc_s.weight,
                                                      ce.gating.fc_s.bias, self.match_fn.scale)
        else:
            sim_matrix = self._loop(audio_emb, length, token_emb, text_len, phrases_num, T, N)
        sim = self.sim_pooling({"sim": sim_matrix, "audio_len": length, "text_len": phrases_num})
        return {"sim": sim, "sim_matrix": sim_matrix}


class ConvTextBlock(nn.Module):
    """PANNs conv block with the text added between BatchNorm and ReLU (models/audio_text_model.py:571-636): the reference's
    parameters and state-dict keys (conv1, conv2 without bias; bn1, bn2; fc_text).  Inside CrossCnn8_Rnn the whole-model node
    reads them; ``forward`` is the block on its own."""

    def __init__(self, in_channels, out_channels, text_emb_dim):
        super().__init__()
        self.conv1 = nn.Conv2d(in_channels, out_channels, kernel_size=(3, 3), stride=(1, 1), padding=(1, 1), bias=False)
        self.conv2 = nn.Conv2d(out_channels, out_channels, kernel_size=(3, 3), stride=(1, 1), padding=(1, 1), bias=False)
        self.bn1 = nn.BatchNorm2d(out_channels)
        self.bn2 = nn.BatchNorm2d(out_channels)
        self.fc_text = nn.Linear(text_emb_dim, out_channels)
        self.init_weight()

    def init_weight(self):
        init_layer(self.conv1)
        init_layer(self.conv2)
        init_layer(self.fc_text)
        init_bn(self.bn1)
        init_bn(self.bn2)

    def forward(self, audio, text, pool_size=(2, 2), pool_type="avg"):
        """audio NCHW (B, Cin, T, F), text (B, text_emb_dim) -> (B, C, T/ph, F/pw)."""
        if pool_type not in ops.POOL_TYPES:
            raise Exception("Incorrect argument!")
        ph, pw = (pool_size, pool_size) if isinstance(pool_size, int) else (int(pool_size[0]), int(pool_size[1]))
        if (ph, pw) not in ops.POOL_SIZES:
            raise RuntimeError(f"ConvTextBlock: pool_size {(ph, pw)} has no kernel instance (built: {sorted(ops.POOL_SIZES)})")
        t = ops.LinearFunction.apply(text, self.fc_text.weight, self.fc_text.bias)
        for m in (self.bn1, self.bn2):
            if m.training:
                m.num_batches_tracked += 1
        x = audio.permute(0, 2, 3, 1).contiguous()               # channels-last (plumbing copy)
        y = ops.ConvTextBlockFunction.apply(x, t, (self.bn1, self.bn2), ph, pw, ops.POOL_TYPES[pool_type], self.conv1.weight,
                                            self.bn1.weight, self.bn1.bias, self.conv2.weight, self.bn2.weight, self.bn2.bias)
        return y.permute(0, 3, 1, 2).contiguous()


class CrossCnn8_Rnn(nn.Module):
    """Early-fusion grounding model (models/audio_text_model.py:639-840): the phrase embedding e = text_encoder(...)["seq_emb"]
    enters every conv layer as a per-(clip, channel) bias (conv_block{i}.fc_text(e)), fc1 (fc1_text(e)) and the GRU output
    (rnn_text(e)); frame_sim (B, T', 1) = clamp(sigmoid(fc_output(.)), 1e-7, 1).  Same constructor, submodule names and
    state-dict keys as the reference (plus the two melspec buffers, as Cnn8Rnn).  Below the text encoder and the six text
    linears the model is ONE operator, tag::cross_cnn8rnn (ops.CrossCnn8RnnFunction).  fp32 only."""

    def __init__(self, sample_rate, text_encoder, freeze_cnn=False, freeze_bn=False, upsample=False):
        super().__init__()
        self.text_encoder = text_encoder
        self.interpolate_ratio = 4
        self.downsample_ratio = 4
        self.upsample = upsample
        self.freeze_cnn = freeze_cnn
        self.freeze_bn = freeze_bn
        self.hop_length = int(0.010 * sample_rate)
        self.win_length = int(0.032 * sample_rate)
        self.n_fft = self.win_length
        if self.n_fft not in (1024, 2048):
            raise ValueError(f"the HIP log-mel frontend supports n_fft 1024/2048 (sample_rate 32000/64000), got {self.n_fft}")
        f_max = 14000 if sample_rate == 32000 else int(sample_rate / 2)
        self.melspec_extractor = _MelFrontendBuffers(
            torch.hann_window(self.win_length),
            slaney_mel_filterbank(self.n_fft // 2 + 1, 50.0, float(f_max), 64, sample_rate))
        self.spec_augmenter = SpecAugmentation(time_drop_width=64, time_stripes_num=2, freq_drop_width=8, freq_stripes_num=2)
        self.text_emb_dim = text_encoder.embed_dim
        self.bn0 = nn.BatchNorm2d(64)
        self.conv_block1 = ConvTextBlock(1, 64, self.text_emb_dim)
        self.conv_block2 = ConvTextBlock(64, 128, self.text_emb_dim)
        self.conv_block3 = ConvTextBlock(128, 256, self.text_emb_dim)
        self.conv_block4 = ConvTextBlock(256, 512, self.text_emb_dim)
        self.fc1 = nn.Linear(512, 512, bias=True)
        self.fc1_text = nn.Linear(self.text_emb_dim, 512)
        self.rnn = nn.GRU(512, 256, bidirectional=True, batch_first=True)
        self.rnn_text = nn.Linear(self.text_emb_dim, 512)
        self.fc_output = nn.Linear(512, 1)
        self.dropout_p = (0.2, 0.5)     # F.dropout sites of the reference forward (:757-766, :812)
        self.init_weight()
        if self.freeze_cnn:
            for param in self.parameters():
                param.requires_grad = False
            for param in self.rnn.parameters():
                param.requires_grad = True

    def init_weight(self):
        init_bn(self.bn0)
        init_layer(self.fc1)
        init_layer(self.fc1_text)
        init_layer(self.rnn_text)
        init_layer(self.fc_output)

    def load_pretrained(self, pretrained, output_fn=sys.stdout.write, training=True, cnn_only=False):
        """Shape-matched merge of a checkpoint (models/audio_text_model.py:709-736); ``cnn_only`` in training drops every key that
        starts with ``rnn``, ``fc1`` or ``fc_output`` (so ``rnn_text.*`` and ``fc1_text.*`` too, as the reference's prefix
        test does)."""
        state_dict = pretrained if isinstance(pretrained, dict) else torch.load(pretrained, map_location="cpu")
        if "model" in state_dict:
            state_dict = state_dict["model"]
        model_dict = self.state_dict()
        pretrained_dict = {k: v for k, v in state_dict.items() if k in model_dict and model_dict[k].shape == v.shape}
        if cnn_only and training:
            pretrained_dict = {k: v for k, v in pretrained_dict.items()
                               if not (k.startswith("rnn") or k.startswith("fc1") or k.startswith("fc_output"))}
        output_fn(f"Loading pretrained keys {pretrained_dict.keys()}")
        model_dict.update(pretrained_dict)
        self.load_state_dict(model_dict, strict=True)

    def train(self, mode: bool = True):
        super().train(mode=mode)
        if self.freeze_bn:
            for m in self.modules():
                if m.__class__.__name__.find("BatchNorm") != -1:
                    m.eval()
        return self

    @property
    def window(self):
        return self.melspec_extractor.spectrogram.window

    @property
    def mel_fb(self):
        return self.melspec_extractor.mel_scale.fb

    def _blocks(self):
        return [getattr(self, f"conv_block{i}") for i in range(1, 5)]

    def _flat_params(self):
        ps = [self.bn0.weight, self.bn0.bias]
        for blk in self._blocks():
            ps += [blk.conv1.weight, blk.bn1.weight, blk.bn1.bias, blk.conv2.weight, blk.bn2.weight, blk.bn2.bias]
        ps += [self.fc1.weight, self.fc1.bias]
        for sfx in ("", "_reverse"):
            ps += [getattr(self.rnn, f"weight_ih_l0{sfx}"), getattr(self.rnn, f"weight_hh_l0{sfx}"),
                   getattr(self.rnn, f"bias_ih_l0{sfx}"), getattr(self.rnn, f"bias_hh_l0{sfx}")]
        ps += [self.fc_output.weight, self.fc_output.bias]
        return ps

    def _check_args(self, waveform, specaug, mixup_lambda):
        """Train-mode augmentation arguments, checked before any launch: () or (stripes,) on the device."""
        self._last_specaug = None
        if not self.training:
            return ()
        if mixup_lambda is not None:
            raise ValueError("CrossCnn8_Rnn: mixup is not supported. The reference's do_mixup halves the clips while the text "
                             "embedding keeps one row per clip, so B text rows would meet B/2 clips (a silent broadcast at "
                             "B = 2, an error for B >= 4); pass mixup_lambda=None")
        if not specaug:
            return ()
        frames = waveform.shape[1] // self.hop_length + 1
        stripes = self.spec_augmenter.draw(waveform.shape[0], frames, self.bn0.num_features)
        self._last_specaug = stripes
        return (torch_ops.stage_to_device(stripes, waveform.device, torch.int32),)

    def forward(self, input_dict):
        ops.check_cross_precision()
        waveform = input_dict["waveform"]
        augment = self._check_args(waveform, input_dict["specaug"], input_dict.get("mixup_lambda", None))
        e = self.text_encoder(input_dict)["seq_emb"]
        texts = [ops.LinearFunction.apply(e, blk.fc_text.weight, blk.fc_text.bias) for blk in self._blocks()]
        texts += [ops.LinearFunction.apply(e, self.fc1_text.weight, self.fc1_text.bias),
                  ops.LinearFunction.apply(e, self.rnn_text.weight, self.rnn_text.bias)]
        if self.training and not self.freeze_bn:
            ops.bump_bn_counters(self, [self.bn0, *(b.bn1 for b in self._blocks()), *(b.bn2 for b in self._blocks())])
        params = self._flat_params()
        need = torch.is_grad_enabled() and any(t.requires_grad for t in list(params) + texts)
        prev, engine._RECORDING = engine._RECORDING, torch.is_grad_enabled()
        try:
            prob = torch.ops.tag.cross_cnn8rnn(waveform, texts, params, torch_ops.encoder_token(self), need, *augment)
        finally:
            engine._RECORDING = prev
            torch_ops._ENC_HANDOVER[0] = None
        length = torch.div(torch.as_tensor(input_dict["waveform_len"]), self.hop_length, rounding_mode="floor") + 1
        length = torch.div(length, self.interpolate_ratio, rounding_mode="floor")
        if self.interpolate_ratio != 1 and self.upsample:
            prob = ops.UpsampleLinearFunction.apply(prob.squeeze(2), self.interpolate_ratio).unsqueeze(2)
            length = length * self.interpolate_ratio
        return {"frame_sim": prob, "length": length}


class CDurTextBlock(nn.Module):
    """CDur block with the text added to the raw conv output (models/audio_text_model.py:461-479):
    leaky_0.1(conv(bn(x)) + fc_text(text)[:, :, None, None]); the reference's submodules and state-dict keys (bn, conv without
    bias, activation, fc_text).  Inside CrossCDur the whole-model node reads them; ``forward`` is the block on its own."""

    def __init__(self, cin, cout, text_emb_dim, kernel_size=3, padding=1):
        super().__init__()
        if kernel_size != 3 or padding != 1:
            raise ValueError("CDurTextBlock: the HIP conv kernels are 3x3 / pad 1")
        self.bn = nn.BatchNorm2d(cin)
        self.conv = nn.Conv2d(cin, cout, kernel_size, padding=padding, bias=False)
        self.activation = nn.LeakyReLU(0.1, True)
        self.fc_text = nn.Linear(text_emb_dim, cout)

    def forward(self, x, text):
        """x NCHW (B, Cin, T, F), text (B, text_emb_dim) -> (B, Cout, T, F).  Shapes: those the biased conv kernels serve
        (Cin 1 with F a multiple of 4; Cin 32 | 128 -> Cout 128 with F 16 | 4)."""
        t = ops.LinearFunction.apply(text, self.fc_text.weight, self.fc_text.bias)
        if self.bn.training:
            self.bn.num_batches_tracked += 1
        xl = x.permute(0, 2, 3, 1).contiguous()                  # channels-last (plumbing copy)
        y = ops.CDurTextBlockFunction.apply(xl, t, self.bn, self.bn.weight, self.bn.bias, self.conv.weight)
        return y.permute(0, 3, 1, 2).contiguous()


class CrossCDur(nn.Module):
    """Early-fusion grounding model on the CDur CRNN (models/audio_text_model.py:482-568): the phrase embedding
    e = text_encoder(...)["seq_emb"] enters every conv layer as a per-(clip, channel) bias on the raw conv output
    (block{i}.fc_text(e)) and the GRU output (fc_text(e)); frame_sim (B, T') = clamp(sigmoid(fc_output(.)), 1e-7, 1), 2-D.
    Same constructor, attributes, submodule names and state-dict keys as the reference (plus the two melspec buffers, as
    CrnnEncoder).  Below the text encoder and the six text linears the model is ONE operator, tag::cross_cdur
    (ops.CrossCDurFunction).  fp32 only.  The forward reads neither ``specaug`` nor ``mixup_lambda`` (the reference's does not).

    Reference quirk, mirrored: the constructor ends with ``self.apply(init_weights)``, which runs over the text encoder too --
    an nn.Embedding inside it is re-drawn (kaiming-uniform, models/utils.py:5-20), whatever its own constructor did."""

    def __init__(self, sample_rate, text_encoder, upsample=False):
        super().__init__()
        self.text_encoder = text_encoder
        self.n_fft = 2048
        self.win_length = 40 * sample_rate // 1000
        self.hop_length = 20 * sample_rate // 1000
        if self.win_length > self.n_fft:
            raise ValueError("win_length must not exceed n_fft=2048")
        self.melspec_extractor = _MelFrontendBuffers(
            torch.hann_window(self.win_length),
            htk_mel_filterbank(self.n_fft // 2 + 1, 0.0, float(sample_rate // 2), 64, sample_rate))
        self.text_emb_dim = text_encoder.embed_dim
        self.block1 = CDurTextBlock(1, 32, self.text_emb_dim)
        self.pool1 = nn.LPPool2d(4, (2, 4))
        self.block2 = CDurTextBlock(32, 128, self.text_emb_dim)
        self.block3 = CDurTextBlock(128, 128, self.text_emb_dim)
        self.pool2 = nn.LPPool2d(4, (2, 4))
        self.block4 = CDurTextBlock(128, 128, self.text_emb_dim)
        self.block5 = CDurTextBlock(128, 128, self.text_emb_dim)
        self.pool3 = nn.LPPool2d(4, (1, 4))
        self.dropout = nn.Dropout(0.3)
        self.dropout_p = 0.3
        self.gru = nn.GRU(self.get_rnn_input_dim(), 128, bidirectional=True, batch_first=True)
        self.fc_text = nn.Linear(self.text_emb_dim, 256)
        self.fc_output = nn.Linear(256, 1)
        self.apply(init_weights)
        self.interpolate_ratio = 4
        self.upsample = upsample

    def get_rnn_input_dim(self):
        """Channels x mel bins after the three pools (the reference probes it with a dummy forward): 128 x (64 // 64)."""
        return self.block5.conv.out_channels * (64 // 4 // 4 // 4)

    window = property(lambda self: self.melspec_extractor.spectrogram.window)
    mel_fb = property(lambda self: self.melspec_extractor.mel_scale.fb)

    def _blocks(self):
        return [getattr(self, f"block{i}") for i in range(1, 6)]

    def _bn_modules(self):
        return [b.bn for b in self._blocks()]

    def _flat_params(self):
        ps = []
        for b in self._blocks():
            ps += [b.bn.weight, b.bn.bias, b.conv.weight]
        for sfx in ("", "_reverse"):
            ps += [getattr(self.gru, f"weight_ih_l0{sfx}"), getattr(self.gru, f"weight_hh_l0{sfx}"),
                   getattr(self.gru, f"bias_ih_l0{sfx}"), getattr(self.gru, f"bias_hh_l0{sfx}")]
        ps += [self.fc_output.weight, self.fc_output.bias]
        return ps

    def forward(self, input_dict):
        ops.check_cross_cdur_precision()
        waveform = input_dict["waveform"]
        e = self.text_encoder(input_dict)["seq_emb"]
        texts = [ops.LinearFunction.apply(e, b.fc_text.weight, b.fc_text.bias) for b in self._blocks()]
        texts.append(ops.LinearFunction.apply(e, self.fc_text.weight, self.fc_text.bias))
        if self.training:
            ops.bump_bn_counters(self, self._bn_modules())
        params = self._flat_params()
        need = torch.is_grad_enabled() and any(t.requires_grad for t in list(params) + texts)
        prev, engine._RECORDING = engine._RECORDING, torch.is_grad_enabled()
        try:
            prob = torch.ops.tag.cross_cdur(waveform, texts, params, torch_ops.encoder_token(self), need)
        finally:
            engine._RECORDING = prev
            torch_ops._ENC_HANDOVER[0] = None
        length = torch.div(torch.as_tensor(input_dict["waveform_len"]), self.hop_length, rounding_mode="floor") + 1
        length = torch.div(length, self.interpolate_ratio, rounding_mode="floor")
        if self.interpolate_ratio != 1 and self.upsample:
            prob = ops.UpsampleLinearFunction.apply(prob, self.interpolate_ratio)
            length = length * self.interpolate_ratio
        return {"frame_sim": prob, "length": length}


class AudioTagging(nn.Module):
    """The class-mapping baseline (mirror of models/audio_text_model.py:405-458 in the reference; trained by
    python_scripts/training/mapping_to_class/run_strong.py / run_weak.py): phrases are mapped to a fixed set of sound
    classes, the audio encoder is followed by fc_output + sigmoid, and the frame probabilities (B,T',C) are pooled over
    the valid frames into clip probabilities (B,C).  Also the shape of the tagging checkpoints the encoders are
    pre-trained from (``backbone.*`` keys).  Below the encoder the forward is ONE node (ops.TaggingHeadFunction: the
    GEMM with the sigmoid in its epilogue, then a class-innermost pooling pass); no clamp on the sigmoid, as in the
    reference."""

    def __init__(self, audio_encoder, classes_num, pooling="linear_softmax"):
        super().__init__()
        self.backbone = audio_encoder
        self.fc_output = nn.Linear(audio_encoder.embed_dim, classes_num)
        self.pooling = pooling

    def load_pretrained(self, pretrained, output_fn, training=True, cnn_only=False):
        if isinstance(pretrained, dict):
            state_dict = pretrained
        else:
            state_dict = torch.load(pretrained, map_location="cpu")
        if "model" in state_dict:
            state_dict = state_dict["model"]
        model_dict = self.state_dict()
        pretrained_dict = {k: v for k, v in state_dict.items() if (k in model_dict) and (model_dict[k].shape == v.shape)}
        if cnn_only and training:
            pretrained_dict = {k: v for k, v in pretrained_dict.items()
                               if not k.startswith(("backbone.rnn", "backbone.fc1", "fc_output"))}
        output_fn(f"Loading pretrained keys {pretrained_dict.keys()}")
        model_dict.update(pretrained_dict)
        self.load_state_dict(model_dict, strict=True)

    def forward(self, input_dict):
        if self.pooling not in ops.POOL_MODES:
            raise Exception(f"Unsupported pooling {self.pooling}")
        output = self.backbone(input_dict)
        embedding = output["embedding"]
        ops.check_tagging_precision(embedding)
        length = output["length"]
        len_dev = torch.as_tensor(length).long().to(embedding.device).contiguous()
        prob, clip_prob = ops.TaggingHeadFunction.apply(embedding, self.fc_output.weight, self.fc_output.bias, len_dev,
                                                        ops.POOL_MODES[self.pooling])
        return {"frame_sim": prob, "clip_sim": clip_prob, "length": length}
