"""Plain-torch restatement of the class-mapping baseline's head (AudioTagging.forward below its encoder, the four
*_with_lens poolings, ClipBceLoss / MaskedFrameBceLoss / ClipMaskedFrameBceLoss) and the seeded inputs of the fixture
tests/golden/audio_tagging.npz -- shared by the script that makes the fixture (which asserts that this restatement equals
the imported reference to 1e-13 in fp64) and by the tests, which use it in fp64 at sizes the fixture does not cover.
Nothing here touches the reference or the HIP path."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import tag_oracle as O

POOLINGS = ("linear_softmax", "max", "mean", "exp_softmax")
HEAD_SHAPE = (4, 37, 64, 24)              # (B, T, E, C) of the head-level fixture case
HEAD_SEED = 3301
FRAME_WEIGHT = 0.7
MODELS = {"cnn8rnn": dict(classes=527, embed=512, hop=320, state_seed=41, fc_seed=43, batch_seed=45),
          "crnn": dict(classes=300, embed=256, hop=640, state_seed=47, fc_seed=49, batch_seed=51)}
MODEL_SAMPLES = 48000                     # 1.5 s at 32 kHz


def draw_head_case(seed=HEAD_SEED, shape=HEAD_SHAPE):
    """Seeded head inputs (fp32): embedding ~ N(0,1), weight ~ N(0,1) 2/sqrt(E), bias ~ N(0, 0.5^2), strong labels
    Bernoulli(0.3), weak labels Bernoulli(0.3), class mask Bernoulli(0.5), lengths in [T/3, T] with clip 0 at T and the
    last clip at 1."""
    B, T, E, C = shape
    g = torch.Generator().manual_seed(seed)
    case = {"embedding": torch.randn(B, T, E, generator=g),
            "weight": torch.randn(C, E, generator=g) * (2.0 / math.sqrt(E)),
            "bias": 0.5 * torch.randn(C, generator=g),
            "strong_label": (torch.rand(B, T, C, generator=g) < 0.3).float(),
            "weak_label": (torch.rand(B, C, generator=g) < 0.3).float(),
            "strong_label_mask": (torch.rand(B, C, generator=g) < 0.5).float()}
    length = torch.randint(max(1, T // 3), T + 1, (B,), generator=g)
    length[0] = T
    if B > 1:
        length[-1] = 1
    case["length"] = length
    return case


def length_mask(length, T):
    return torch.arange(T)[None, :] < torch.as_tensor(length).long()[:, None]


def pool(prob, length, pooling, argmax=None):
    """models/utils.py:49-84 over the frames < length[b]; ``argmax`` (B,C) imposes the frame the max is taken at."""
    B, T, C = prob.shape
    m = length_mask(length, T).to(prob.dtype).unsqueeze(-1)
    lens = torch.as_tensor(length).to(prob.dtype).view(B, 1)
    if pooling == "mean":
        return (prob * m).sum(1) / lens
    if pooling == "linear_softmax":
        return (prob * prob * m).sum(1) / (prob * m).sum(1)
    if pooling == "exp_softmax":
        e = torch.exp(prob) * m
        return (e * prob).sum(1) / e.sum(1)
    if pooling == "max":
        if argmax is not None:
            return prob.gather(1, torch.as_tensor(argmax).long().view(B, 1, C)).squeeze(1)
        return prob.masked_fill(m == 0, float("-inf")).max(1)[0]
    raise Exception(f"Unsupported pooling {pooling}")


def head(embedding, weight, bias, length, pooling, argmax=None):
    prob = torch.sigmoid(embedding @ weight.t() + bias)
    return prob, pool(prob, length, pooling, argmax)


def clip_bce(clip, label):
    return F.binary_cross_entropy(clip, label)


def masked_frame_bce(prob, label, length, cls_mask=None):
    B, T, C = prob.shape
    bce = F.binary_cross_entropy(prob, label, reduction="none")
    m = length_mask(torch.as_tensor(length).clamp(1, T), T).to(prob.dtype).unsqueeze(-1)
    if cls_mask is not None:
        m = m * cls_mask.to(prob.dtype).unsqueeze(1)
    else:
        m = m.expand(B, T, C)
    return (bce * m).sum() / m.sum()


def clip_masked_frame_bce(prob, clip, weak_label, strong_label, length, cls_mask, frame_weight):
    return (1 - frame_weight) * clip_bce(clip, weak_label) + frame_weight * masked_frame_bce(prob, strong_label, length,
                                                                                             cls_mask)


def head_case_results(case, pooling, dtype, frame_weight=FRAME_WEIGHT, argmax=None):
    """Forward, the three losses and the gradients of the mixed loss for one pooling -> dict of detached tensors."""
    x = case["embedding"].to(dtype).clone().requires_grad_(True)
    w = case["weight"].to(dtype).clone().requires_grad_(True)
    b = case["bias"].to(dtype).clone().requires_grad_(True)
    prob, clip = head(x, w, b, case["length"], pooling, argmax)
    weak, strong, mask = (case[k].to(dtype) for k in ("weak_label", "strong_label", "strong_label_mask"))
    l_clip = clip_bce(clip, weak)
    l_frame = masked_frame_bce(prob, strong, case["length"], mask)
    l_mix = (1 - frame_weight) * l_clip + frame_weight * l_frame
    l_mix.backward()
    return {"frame_sim": prob.detach(), "clip_sim": clip.detach(), "loss_clip": l_clip.detach(),
            "loss_frame": l_frame.detach(), "loss_mix": l_mix.detach(), "dembedding": x.grad, "dweight": w.grad,
            "dbias": b.grad}


# ---- model level: seeded weights and inputs (no weight tensors in the fixture, only checksums) ----
def model_state(kind):
    """fp32 state dict of AudioTagging(encoder, classes) keyed by the reference's names: the oracle's seeded encoder state
    with ``audio_encoder.`` renamed to ``backbone.`` and a seeded fc_output."""
    cfg = MODELS[kind]
    if kind == "cnn8rnn":
        st = O.init_state(seed=cfg["state_seed"], logit_gain=2.0)
    else:
        st = O.init_crnn_state(seed=cfg["state_seed"], embed_dim=cfg["embed"])
    out = {"backbone." + k[len("audio_encoder."):]: v for k, v in st.items() if k.startswith("audio_encoder.")}
    g = torch.Generator().manual_seed(cfg["fc_seed"])
    out["fc_output.weight"] = torch.randn(cfg["classes"], cfg["embed"], generator=g) * (2.0 / math.sqrt(cfg["embed"]))
    out["fc_output.bias"] = 0.5 * torch.randn(cfg["classes"], generator=g)
    return out


def model_batch(kind):
    cfg = MODELS[kind]
    return O.synthetic_batch(2, MODEL_SAMPLES, seed=cfg["batch_seed"], ragged=True, hop=cfg["hop"])


def checksum(t):
    t = torch.as_tensor(t).detach().double().flatten()
    return [float(t.sum()), float(t.abs().max()), float(t[:: max(1, t.numel() // 7)][:7].sum())]


def state_checksum(st):
    return np.array([c for k in sorted(st) if st[k].is_floating_point() for c in checksum(st[k])])


def encoder_forward(kind, st, waveform, waveform_len):
    """The oracle's encoder (eval mode) on a ``backbone.``-keyed state."""
    fn = O.cnn8rnn_forward if kind == "cnn8rnn" else O.crnn_forward
    return fn(st, waveform, waveform_len, training=False, prefix="backbone.")
