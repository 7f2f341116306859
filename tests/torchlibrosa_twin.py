"""Test-side twin of torchlibrosa's SpecAugment (torchlibrosa augmentation.py: ``DropStripes``, ``SpecAugmentation``), which the
reference's Cnn8Rnn applies to its bn0 output (models/audio_encoder.py:126-131,192-195).  torchlibrosa is not a dependency of
this project; the twin restates its rule so that the package's stripe draw is pinned against it:

    per dropper (time, dim 2, first; then frequency, dim 3), per clip n = 0..B-1, per stripe:
        distance = torch.randint(low=0, high=drop_width, size=(1,))[0]
        bgn      = torch.randint(low=0, high=total_width - distance, size=(1,))[0]
        input[n][:, bgn:bgn + distance, :] = 0     (dim 2)   /   input[n][:, :, bgn:bgn + distance] = 0   (dim 3)

in place, from torch's global CPU generator, in train mode only.  ``record`` collects [bgn, distance] per stripe in draw order.
"""
import torch
import torch.nn as nn


class DropStripes(nn.Module):
    def __init__(self, dim, drop_width, stripes_num, record=None):
        super().__init__()
        assert dim in [2, 3]
        self.dim = dim
        self.drop_width = drop_width
        self.stripes_num = stripes_num
        self.record = record if record is not None else []

    def forward(self, input):
        assert input.ndimension() == 4
        if self.training is False:
            return input
        batch_size = input.shape[0]
        total_width = input.shape[self.dim]
        for n in range(batch_size):
            self.transform_slice(input[n], total_width)
        return input

    def transform_slice(self, e, total_width):
        for _ in range(self.stripes_num):
            distance = torch.randint(low=0, high=self.drop_width, size=(1,))[0]
            bgn = torch.randint(low=0, high=total_width - distance, size=(1,))[0]
            self.record.append((int(bgn), int(distance)))
            if self.dim == 2:
                e[:, bgn: bgn + distance, :] = 0
            elif self.dim == 3:
                e[:, :, bgn: bgn + distance] = 0


class SpecAugmentation(nn.Module):
    def __init__(self, time_drop_width, time_stripes_num, freq_drop_width, freq_stripes_num):
        super().__init__()
        self.time_record, self.freq_record = [], []
        self.time_dropper = DropStripes(dim=2, drop_width=time_drop_width, stripes_num=time_stripes_num,
                                        record=self.time_record)
        self.freq_dropper = DropStripes(dim=3, drop_width=freq_drop_width, stripes_num=freq_stripes_num,
                                        record=self.freq_record)

    def forward(self, input):
        x = self.time_dropper(input)
        x = self.freq_dropper(x)
        return x

    def table(self, batch_size):
        """The recorded stripes of the LAST forward as the package's table: int32 (B, n_time + n_freq, 2) [bgn, width]."""
        nt, nf = self.time_dropper.stripes_num, self.freq_dropper.stripes_num
        t = torch.tensor(self.time_record[-batch_size * nt:], dtype=torch.int32).view(batch_size, nt, 2) if nt else \
            torch.empty(batch_size, 0, 2, dtype=torch.int32)
        f = torch.tensor(self.freq_record[-batch_size * nf:], dtype=torch.int32).view(batch_size, nf, 2) if nf else \
            torch.empty(batch_size, 0, 2, dtype=torch.int32)
        return torch.cat([t, f], 1)
