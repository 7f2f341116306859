"""Plain torch statements of align.ExpNegL2 and of the tail of MultiTextBiEncoderWithAlign, in the dtype and on the device of
their inputs (fp64 on the CPU = the truth of the tests; fp32 = the yardstick of their tolerance and of tools/with_align_bench.py).
Gradients come from autograd.  tests/test_with_align_cpu.py pins both to the imported reference (tests/golden/with_align.npz).

The reference's ExpNegL2 writes its score into a float32 CPU ``torch.zeros`` whatever goes in, so its "fp64" result is rounded
to fp32; the statement here keeps the dtype of its inputs."""
import torch
import torch.nn.functional as F

from oracle import tag_oracle as O


def exp_neg_l2(audio, text):
    """audio (B,T,D), text (B,N,D) -> out (B,B,T,N), out[a,i,t,j] = exp(-||normalize(audio[a,t]) - normalize(text[i,j])||_2).
    The differences are formed by broadcasting (B,1,T,1,D) - (1,B,1,N,D); torch.norm's backward gives 0 at distance 0."""
    an = F.normalize(audio, dim=-1)
    tn = F.normalize(text, dim=-1)
    diff = an[:, None, :, None, :] - tn[None, :, None, :, :]
    return torch.exp(-torch.norm(diff, dim=-1))


def with_align_tail(audio_emb, seq_emb, length, label, n_text, phrase_pooling="linear_softmax", align="expnegl2",
                    sentence_pooling=("mean", "mean"), scale=True):
    """What MultiTextBiEncoderWithAlign computes behind its encoders (no projections, no cross-encoder): audio_emb (B,T,D),
    seq_emb (B*N,D), length (B,), label (B,N) ->
      frame_sim (B,T,N), clip_sim (B,N)   match.DotProduct(text_level="seq") of every clip against its own N phrases, pooled over
                                          the valid frames;
      sim_matrix (B,B,T,max_num), sentence_sim (B,B)   the first label[i].sum() phrases of clip i are its positives, padded with
                                          zero rows to the longest count AS THE REFERENCE DOES (pad_sequence), scored by the align
                                          function against every clip's frames and pooled over the valid frames and phrases."""
    B, T, D = audio_emb.shape
    a = audio_emb.unsqueeze(1).expand(-1, n_text, -1, -1).reshape(B * n_text, T, D)
    fs = O.match_dot_product(a, seq_emb, scale=scale)
    frame_sim = fs.reshape(B, n_text, T).transpose(1, 2)
    clip_sim = O.SEQ_POOL[phrase_pooling](frame_sim, length)
    phrases_num = label.sum(1).long().tolist()
    seq = seq_emb.reshape(B, n_text, D)
    padded = torch.nn.utils.rnn.pad_sequence([seq[i, :phrases_num[i]] for i in range(B)], batch_first=True)
    if align == "expnegl2":
        sim_matrix = exp_neg_l2(audio_emb, padded)
    else:
        sim_matrix = O.align_dot_product(audio_emb, padded, **align)
    sentence_sim = O.sim_pooling(sim_matrix, length, phrases_num, *sentence_pooling)
    return {"frame_sim": frame_sim, "clip_sim": clip_sim, "sim_matrix": sim_matrix, "sentence_sim": sentence_sim}


def clip_plus_sentence_loss(out, label, margin=0.1):
    """MultipleLossSum(["clip", "sentence"], [1, 1], clip=ClipBceLoss(), sentence=MaxMarginRankingLoss(margin, sim_key="sentence_sim"))."""
    return O.clip_bce_loss(out["clip_sim"], label) + O.max_margin_ranking_loss(out["sentence_sim"], margin, 1.0)
