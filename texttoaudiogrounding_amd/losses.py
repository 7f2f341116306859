"""FrameBceLoss behind the reference interface (losses.py:11-35 in the reference)."""
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
