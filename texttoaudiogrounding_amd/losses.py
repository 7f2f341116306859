"""FrameBceLoss behind the reference interface (losses.py:11-35 in the reference)."""
import math
from typing import Dict

import numpy as np
import torch
import torch.nn as nn

from . import ops
from . import torch_ops  # noqa: F401  (registers torch.ops.tag.*)


class FrameBceLoss(nn.Module):
    def forward(self, output: Dict):
        frame_sim = output["frame_sim"]
        if frame_sim.ndim == 3 and frame_sim.size(2) == 1:
            frame_sim = frame_sim.squeeze(2)
        return self.forward_tensor(frame_sim, output["label"], output["length"])

    def forward_tensor(self, frame_sim, label, length):
        Tt = min(frame_sim.size(1), label.size(1))
        if frame_sim.size(1) != label.size(1):
            raise RuntimeError("frame_sim and label must be aligned first (Runner.forward does it)")
        length = torch.as_tensor(length).long().to(frame_sim.device).contiguous()
        return torch.ops.tag.frame_bce(frame_sim, label.to(frame_sim.device).float(), length, Tt)


class ClipBceLoss(nn.Module):
    """losses.py:38-43 in the reference: F.binary_cross_entropy(clip_sim, label) -- the mean over the (B,N) clip matrix,
    evaluated by the frame-BCE kernels with every row of full length."""

    def forward(self, output: Dict):
        return self.forward_tensor(output["clip_sim"], output["label"])

    def forward_tensor(self, prob, label):
        B, N = prob.shape
        length = torch.full((B,), N, dtype=torch.long, device=prob.device)
        return torch.ops.tag.frame_bce(prob.contiguous(), label.to(prob.device).float().contiguous(), length, N)


class MaxMarginRankingLoss(nn.Module):
    """losses.py:226-264 in the reference (triplet ranking over the (B,B) clip-vs-caption matrix)."""

    def __init__(self, margin=1, fix_norm=True, lamda1=1, sim_key="sim"):
        super().__init__()
        self.fix_norm, self.margin, self.lamda1, self.sim_key = fix_norm, margin, lamda1, sim_key

    def forward(self, x):
        return ops.MaxMarginFunction.apply(x[self.sim_key], self.margin, self.lamda1, self.fix_norm)


class InfoNceLoss(nn.Module):
    """losses.py:267-281 in the reference: symmetric cross-entropy of sim / tau against the diagonal of the (B,B) matrix."""

    def __init__(self, tau=0.07):
        super().__init__()
        self.tau = tau

    def forward(self, output: Dict):
        return torch.ops.tag.infonce(output["sim"], float(self.tau))


class _TripletLoss(nn.Module):
    mode = None

    def __init__(self, margin=1.0):
        super().__init__()
        self.margin = margin

    def forward(self, output: Dict):
        return torch.ops.tag.triplet(output["sim"], ops.TRIPLET_MODES[self.mode], float(self.margin), None, None)


class MaxTripletLoss(_TripletLoss):
    """losses.py:285-315 in the reference: the hardest negative of every row and of every column of the (B,B) matrix."""
    mode = "max"


class WeightedTripletLoss(_TripletLoss):
    """losses.py:355-417 in the reference (polyloss): for every row of sim and of sim^T whose hardest negative q violates the
    margin against the positive p, clamp(0.2 p^2 - 0.7 p + 0.5, 0) + clamp(0.9 q^2 - 0.4 q + 0.03, 0); total / B."""
    mode = "weighted"


class RandomTripletLoss(_TripletLoss):
    """losses.py:319-351 in the reference: one negative per row, drawn on the host exactly as the reference draws it
    (np.random.randint(n, size=n) for s_index, then again for a_index: a seeded numpy stream gives the reference's draws)
    and uploaded as int32."""
    mode = "random"

    def forward(self, output: Dict):
        sim = output["sim"]
        n = sim.size(0)
        s_index = np.random.randint(n, size=n)
        a_index = np.random.randint(n, size=n)
        s_index, a_index = (torch_ops.stage_to_device(torch.from_numpy(v), sim.device, torch.int32) for v in (s_index, a_index))
        return torch.ops.tag.triplet(sim, ops.TRIPLET_MODES[self.mode], float(self.margin), s_index, a_index)


class MilNceLoss(nn.Module):
    """losses.py:46-56 in the reference: mean_b[LSE_n(clip_sim / tau) - LSE_n(clip_sim * label / tau)] over (B,N)."""

    def __init__(self, tau=1.0) -> None:
        super().__init__()
        self.tau = tau

    def forward(self, output: Dict):
        clip_sim = output["clip_sim"]
        return torch.ops.tag.milnce(clip_sim, output["label"].to(clip_sim.device).float(), float(self.tau))


def _clip_bce(output: Dict, mode, c0=0.0, c1=0.0, c2=0.0, aux=None):
    clip_sim = output["clip_sim"]
    label = output["label"].to(clip_sim.device).float()
    return torch.ops.tag.clip_bce(clip_sim, label, aux, ops.CLIP_BCE_MODES[mode], float(c0), float(c1), float(c2))


def _clip_counts(output: Dict):
    """output["counts"] (B,N), numpy or tensor, as SamplePhrasesCountDataset fills it with neg_samp_stratg == "similarity"
    (any other strategy leaves empty lists there)."""
    counts, clip_sim = output["counts"], output["clip_sim"]
    if not torch.is_tensor(counts):
        counts = np.asarray(counts)
    if tuple(counts.shape) != tuple(clip_sim.shape):
        raise ValueError(f"counts {tuple(counts.shape)}: expected clip_sim's shape {tuple(clip_sim.shape)} (the dataset "
                         f"fills counts only with neg_samp_stratg == 'similarity')")
    return counts


def _clip_aux(value, clip_sim):
    """A host (or device) table formed by the reference's own expression -> fp32 (B,N) on clip_sim's device."""
    return torch_ops.stage_to_device(torch.as_tensor(value).expand(clip_sim.shape), clip_sim.device, torch.float32)


class FocalClipBceLoss(nn.Module):
    """losses.py:59-72 in the reference: mean of -alpha (1-p)^gamma y ln p - (1-alpha) p^gamma (1-y) ln(1-p) over (B,N).
    The logarithms are clamped at -100 and the derivative's denominators guarded as in binary_cross_entropy, so the loss and
    its gradient are finite at clip_sim == 0 and == 1 (the reference is NaN/inf there)."""

    def __init__(self, gamma=2, alpha=0.25) -> None:
        super().__init__()
        self.gamma = gamma
        self.alpha = alpha

    def forward(self, output: Dict):
        return _clip_bce(output, "focal", self.gamma, self.alpha)


class ClipBceLossFreqWeight(nn.Module):
    """losses.py:75-87 in the reference: binary_cross_entropy weighted by (C / (C + counts))^gamma on the positives (label != 0)
    and by 1 on the negatives.  The weight is formed by the reference's expression on whatever holds counts (fp64 on the host
    for numpy) and cast to fp32; the where(label == 0, 1, .) is the kernel's."""

    def __init__(self, C, gamma) -> None:
        super().__init__()
        self.C = C
        self.gamma = gamma

    def forward(self, output: Dict):
        counts = _clip_counts(output)
        weight = (self.C / (self.C + counts))**self.gamma
        return _clip_bce(output, "freq_weight", aux=_clip_aux(weight, output["clip_sim"]))


class SymmetricClipBceLoss(nn.Module):
    """losses.py:90-104 in the reference: bce(clip_sim, label) + bce(clamp(label, eps, 1 - eps), clip_sim); a and b are stored
    and unused, as there."""

    def __init__(self, a=1, b=1, eps=1e-3) -> None:
        super().__init__()
        self.a = a
        self.b = b
        self.eps = eps

    def forward(self, output: Dict):
        return _clip_bce(output, "symmetric", self.eps)


class OriginSymmetricClipBceLoss(nn.Module):
    """losses.py:107-122 in the reference: a * bce(clip_sim, label) - b * A * mean(label (1 - clip_sim) + (1 - label) clip_sim),
    A = ln eps."""

    def __init__(self, a=1, b=1, eps=1e-3) -> None:
        super().__init__()
        self.a = a
        self.b = b
        self.A = math.log(eps)

    def forward(self, output: Dict):
        return _clip_bce(output, "origin_symmetric", self.a, self.b, self.A)


class PriorAdjustedClipBceLoss(nn.Module):
    """losses.py:125-143 in the reference: bce(q, label) with q = p pi^tau / (p pi^tau + (1 - p) (1 - pi)^tau) and the prior
    pi = counts / data_size in (0,1), formed on whatever holds counts and cast to fp32.  data_size: a scalar or anything that
    broadcasts against (B,N)."""

    def __init__(self, data_size, tau=1) -> None:
        super().__init__()
        self.data_size = data_size
        self.tau = tau

    def forward(self, output: Dict):
        counts = _clip_counts(output)
        prior = counts / self.data_size
        return _clip_bce(output, "prior_adjusted", self.tau, aux=_clip_aux(prior, output["clip_sim"]))


class VectorQuantizeLoss(nn.Module):
    """losses.py:213-223 in the reference: vq_weight * output["vq_loss"] + loss_fn(output)."""

    def __init__(self, loss_fn, vq_weight=1.0):
        super().__init__()
        self.loss_fn = loss_fn
        self.vq_weight = vq_weight

    def forward(self, output):
        return self.vq_weight * output["vq_loss"] + self.loss_fn(output)

    def get_separate_loss(self, output):
        return {"cls_loss": self.loss_fn(output), "vq_loss": output["vq_loss"]}


class MultipleLossSum(nn.Module):
    """losses.py:420-440 in the reference: sum_k weights[k] * names[k], where a name already present in the output dict is
    taken as a ready value and any other is the sub-loss registered under it."""

    def __init__(self, names, weights, **loss_fns):
        super().__init__()
        self.names = names
        self.weights = weights
        for name, loss_fn in loss_fns.items():
            self.add_module(name, loss_fn)

    def forward(self, output: Dict):
        tot_loss = 0
        for name, weight in zip(self.names, self.weights):
            loss = output[name] if name in output else getattr(self, name)(output)
            tot_loss = tot_loss + weight * loss
        return tot_loss


class ClipFrameBceLoss(nn.Module):
    """losses.py:186-210 in the reference: (1 - w) * ClipBceLoss(clip_sim, weak_label) + w * FrameBceLoss(frame_sim (B,T,N),
    strong_label (B,T,N), length).  The 3-D frame term equals the 2-D kernel over rows (b, n) of length[b] (the mask count
    is sum_b len_b * N either way), so the (B,T,N) view of MultiTextBiEncoder's (B*N,T) scores is used as it lies."""

    def __init__(self, frame_weight, clip_label_key="weak_label", clip_prob_key="clip_sim", frame_label_key="strong_label",
                 frame_prob_key="frame_sim"):
        super().__init__()
        self.clip_loss_fn, self.frame_loss_fn = ClipBceLoss(), FrameBceLoss()
        self.frame_weight = frame_weight
        self.clip_label_key, self.clip_prob_key = clip_label_key, clip_prob_key
        self.frame_label_key, self.frame_prob_key = frame_label_key, frame_prob_key

    def forward(self, output: Dict):
        fs, lab = output[self.frame_prob_key], output[self.frame_label_key]
        B, T, N = fs.shape
        fs2 = fs.transpose(1, 2).reshape(B * N, T)                      # a view for MultiTextBiEncoder's output
        lab2 = lab.to(fs.device).float().transpose(1, 2).reshape(B * N, T).contiguous()
        length = torch.as_tensor(output["length"]).long().to(fs.device).repeat_interleave(N).contiguous()
        frame = torch.ops.tag.frame_bce(fs2.contiguous(), lab2, length, T)
        clip = self.clip_loss_fn.forward_tensor(output[self.clip_prob_key], output[self.clip_label_key])
        return (1 - self.frame_weight) * clip + self.frame_weight * frame


class MaskedFrameBceLoss(nn.Module):
    """losses.py:157-170 in the reference, for the class-mapping baseline: frame BCE over frame_sim / strong_label (B,T,C),
    masked by the clip lengths and by strong_label_mask (B,C): sum(bce * len_mask * cls_mask) / sum(len_mask * cls_mask).
    The reference is defined when max(length) == T; here every length in [1, T] is served.  One pass over the native
    layout (tag_masked_frame_bce_*); frame_sim / strong_label truncated in time by the runner are read as views."""

    def forward(self, output: Dict):
        fs = output["frame_sim"]
        lab = output["strong_label"].to(fs.device).float()
        mask = output["strong_label_mask"].to(fs.device).float().contiguous()
        length = torch.as_tensor(output["length"]).long().to(fs.device).contiguous()
        return torch.ops.tag.masked_frame_bce(fs, lab, length, mask)


class ClipMaskedFrameBceLoss(nn.Module):
    """losses.py:173-183 in the reference: (1 - w) * ClipBceLoss(clip_sim, weak_label) + w * MaskedFrameBceLoss."""

    def __init__(self, frame_weight):
        super().__init__()
        self.clip_loss_fn = ClipBceLoss()
        self.frame_loss_fn = MaskedFrameBceLoss()
        self.frame_weight = frame_weight

    def forward(self, output: Dict):
        return (1 - self.frame_weight) * self.clip_loss_fn.forward_tensor(output["clip_sim"], output["weak_label"]) + \
            self.frame_weight * self.frame_loss_fn(output)
