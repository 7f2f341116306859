"""Cross-batch frame x text similarity (mirror of models/align.py:7-64 in the reference)."""
import torch
import torch.nn as nn

from .. import torch_ops  # noqa: F401  (registers torch.ops.tag.*)


class DotProduct(nn.Module):
    def __init__(self, l2norm=False, scaled=False) -> None:
        super().__init__()
        self.l2norm = l2norm
        self.scaled = scaled

    def forward(self, audio: torch.Tensor, text: torch.Tensor, **kwargs):
        a_bs, _, a_dim = audio.size()
        t_bs, _, t_dim = text.size()
        assert a_bs == t_bs
        assert a_dim == t_dim
        return torch.ops.tag.align_dot(audio, text, bool(self.l2norm), bool(self.scaled))


class ExpNegL2(nn.Module):
    """exp(-||normalize(audio) - normalize(text)||) for every (clip, frame) x (clip, phrase) pair, (B,B,T,N).  The result stays on
    the device of its inputs; the reference writes it into a CPU ``torch.zeros``."""

    def forward(self, audio: torch.Tensor, text: torch.Tensor):
        a_bs, _, a_dim = audio.size()
        t_bs, _, t_dim = text.size()
        assert a_bs == t_bs
        assert a_dim == t_dim
        return torch.ops.tag.align_expnegl2(audio, text)
