"""SpecAugment with torchlibrosa's interface (torchlibrosa augmentation.py: ``DropStripes`` / ``SpecAugmentation``), which the
reference's Cnn8Rnn applies to the bn0 output in train mode (models/audio_encoder.py:126-131,192-195).

The stripes are drawn on the host from torch's global CPU generator with exactly torchlibrosa's calls, in its order (time
dropper over every clip, then the frequency dropper), so a run seeded with ``torch.manual_seed`` drops the same stripes as the
reference.  ``draw`` returns them as a table; the zeros are written by the HIP kernels of csrc/augment.hip -- inside the fused
encoder (Cnn8Rnn.forward passes the table to tag::cnn8rnn_encoder) or through ``forward`` for a model composed by its user.
No parameters and no buffers: state-dict keys are unchanged.
"""
import torch
import torch.nn as nn


class DropStripes(nn.Module):
    """``stripes_num`` stripes of random width in [0, drop_width) per clip along ``dim`` (2: frames, 3: mel bins)."""

    def __init__(self, dim, drop_width, stripes_num):
        super().__init__()
        if dim not in (2, 3):
            raise ValueError(f"DropStripes: dim must be 2 (time) or 3 (frequency), got {dim}")
        self.dim = dim
        self.drop_width = drop_width
        self.stripes_num = stripes_num

    def draw(self, batch_size, total_width):
        """int32 (batch_size, stripes_num, 2) rows [bgn, width], drawn as torchlibrosa's transform_slice draws them: per clip,
        per stripe, ``distance = randint(0, drop_width)``, then ``bgn = randint(0, total_width - distance)`` (torch's
        global generator; a width that leaves no room raises as it does there)."""
        out = torch.empty(batch_size, self.stripes_num, 2, dtype=torch.int32)
        for n in range(batch_size):
            for k in range(self.stripes_num):
                distance = torch.randint(low=0, high=self.drop_width, size=(1,))[0]
                bgn = torch.randint(low=0, high=total_width - distance, size=(1,))[0]
                out[n, k, 0], out[n, k, 1] = int(bgn), int(distance)
        return out

    def forward(self, input):
        if input.dim() != 4:
            raise ValueError(f"DropStripes expects (batch, channels, time, freq), got {tuple(input.shape)}")
        if not self.training:
            return input
        from ..functions import SpecAugmentFunction
        stripes = self.draw(input.shape[0], input.shape[self.dim]).to(input.device)
        if self.dim == 2:
            return SpecAugmentFunction.apply(input, stripes, self.stripes_num)
        return SpecAugmentFunction.apply(input, stripes, 0)


class SpecAugmentation(nn.Module):
    """Time stripes, then frequency stripes (torchlibrosa's SpecAugmentation)."""

    def __init__(self, time_drop_width, time_stripes_num, freq_drop_width, freq_stripes_num):
        super().__init__()
        self.time_dropper = DropStripes(dim=2, drop_width=time_drop_width, stripes_num=time_stripes_num)
        self.freq_dropper = DropStripes(dim=3, drop_width=freq_drop_width, stripes_num=freq_stripes_num)

    def draw(self, batch_size, time_steps, freq_bins):
        """The stripe table of one call: int32 (batch_size, n_time + n_freq, 2) [bgn, width], time rows first."""
        return torch.cat([self.time_dropper.draw(batch_size, time_steps), self.freq_dropper.draw(batch_size, freq_bins)], 1)

    def forward(self, input):
        """(batch, channels, time, freq) fp32 on the device -> the same with the stripes zeroed (a new tensor; train mode only)."""
        if input.dim() != 4:
            raise ValueError(f"SpecAugmentation expects (batch, channels, time, freq), got {tuple(input.shape)}")
        if not self.training:
            return input
        from ..functions import SpecAugmentFunction
        stripes = self.draw(input.shape[0], input.shape[2], input.shape[3]).to(input.device)
        return SpecAugmentFunction.apply(input, stripes, self.time_dropper.stripes_num)
